"""The host side of the alpha likelihood curves (no GPU): fscl_amd_curve_support's interval on
hand-made curves and fscl_amd_curve_output's text."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import fscl_amd

NAN = math.nan


def curve(coarse, refine=(), null_logl=-100.0, chr_=0, pos=1234):
    """A record from (la, sm) pairs in evaluation order."""
    c = np.zeros(1, dtype=fscl_amd.CURVE_DTYPE)
    c["n_coarse"], c["n_refine"] = len(coarse), len(refine)
    for k, (la, sm) in enumerate(list(coarse) + list(refine)):
        c["la"][0, k], c["sm"][0, k] = la, sm
    c["pt"]["chr"], c["pt"]["sweep_pos"], c["pt"]["null_logl"] = chr_, pos, null_logl
    return c[0]


def test_single_peak(built):
    c = curve([(-6.0, -50.0), (-5.0, -41.0), (-4.0, -40.0), (-3.0, -41.5), (-2.0, -60.0)])
    assert fscl_amd.curve_support(c, 2.0) == (-5.0, -3.0, False, False)
    assert fscl_amd.curve_support(c, 1.0) == (-5.0, -4.0, False, False)
    assert fscl_amd.curve_support(c) == fscl_amd.curve_support(c, 2.0)


def test_drop_zero_is_the_argmax_alone(built):
    c = curve([(-6.0, -50.0), (-5.0, -41.0), (-4.0, -40.0), (-3.0, -41.5)])
    assert fscl_amd.curve_support(c, 0.0) == (-4.0, -4.0, False, False)
    with pytest.raises(ValueError):
        fscl_amd.curve_support(c, -1.0)
    with pytest.raises(ValueError):
        fscl_amd.curve_support(c, NAN)


def test_plateau_of_equal_maxima(built):
    """The argmax is the first maximum in evaluation order; the interval covers the plateau, also at drop 0."""
    c = curve([(-6.0, -50.0), (-5.0, -40.0), (-4.0, -40.0), (-3.0, -40.0), (-2.0, -60.0)])
    assert fscl_amd.curve_support(c, 0.0) == (-5.0, -3.0, False, False)
    assert fscl_amd.curve_support(c, 2.0) == (-5.0, -3.0, False, False)
    # evaluation order is not alpha order: the refine list's equal value at a lower alpha joins the run
    c = curve([(-5.0, -40.0), (-4.0, -60.0)], [(-5.5, -40.0), (-4.5, -70.0)])
    assert fscl_amd.curve_support(c, 0.0) == (-5.5, -5.0, True, False)


def test_open_ends(built):
    lo = curve([(-6.0, -40.0), (-5.0, -41.0), (-4.0, -50.0)])
    assert fscl_amd.curve_support(lo, 2.0) == (-6.0, -5.0, True, False)
    hi = curve([(-6.0, -50.0), (-5.0, -41.0), (-4.0, -40.0)])
    assert fscl_amd.curve_support(hi, 2.0) == (-5.0, -4.0, False, True)
    flat = curve([(-6.0, -40.5), (-5.0, -40.0), (-4.0, -40.25)])
    assert fscl_amd.curve_support(flat, 2.0) == (-6.0, -4.0, True, True)
    # a run that stops short of an end is closed there, whatever lies beyond
    gap = curve([(-6.0, -40.1), (-5.0, -50.0), (-4.0, -40.0), (-3.0, -50.0), (-2.0, -40.2)])
    assert fscl_amd.curve_support(gap, 2.0) == (-4.0, -4.0, False, False)


def test_nan_breaks_the_run(built):
    c = curve([(-7.0, -40.5), (-6.0, NAN), (-5.0, -40.4), (-4.0, -40.0), (-3.0, -40.3), (-2.0, NAN), (-1.0, -40.1)])
    assert fscl_amd.curve_support(c, 2.0) == (-5.0, -3.0, False, False)
    # a NaN never is the argmax, also when it comes first
    c = curve([(-6.0, NAN), (-5.0, -40.0)])
    assert fscl_amd.curve_support(c, 2.0) == (-5.0, -5.0, False, True)


def test_all_nan(built):
    c = curve([(-6.0, NAN), (-5.0, NAN)], [(-5.5, NAN)])
    assert fscl_amd.curve_support(c, 2.0) is None
    assert fscl_amd.curve_support(curve([]), 2.0) is None
    lo, hi, ol, oh = C.c_double(1.0), C.c_double(1.0), C.c_int(7), C.c_int(7)
    rec = np.array([c], dtype=fscl_amd.CURVE_DTYPE)
    r = fscl_amd.get_lib().fscl_amd_curve_support(rec.ctypes.data, 2.0, C.byref(lo), C.byref(hi), C.byref(ol), C.byref(oh))
    assert r == 0 and math.isnan(lo.value) and math.isnan(hi.value) and (ol.value, oh.value) == (0, 0)


def test_duplicate_alphas_are_one_candidate(built):
    """The coarse winner's alpha is in its own refine list again: kept once, so the run's
    neighbours are the distinct alphas on either side."""
    c = curve([(-6.0, -50.0), (-4.0, -40.0), (-2.0, -50.0)],
              [(-5.0, -41.0), (-4.5, -40.5), (-4.0, -40.0), (-3.5, -43.0), (-6.0, -50.0)])
    assert fscl_amd.curve_support(c, 2.0) == (-5.0, -4.0, False, False)
    assert fscl_amd.curve_support(c, 20.0) == (-6.0, -2.0, True, True)


def scan_with_names(names):
    lim = (fscl_amd.ChrLimitsT * len(names))()
    for k, nm in enumerate(names):
        lim[k].chr, lim[k].name = k, nm.encode()
    s = fscl_amd.ScanT()
    s.chr_limits, s.n_chromosomes = lim, len(names)
    return C.pointer(s), lim


def test_curve_output_text(built, tmp_path):
    scan, keep = scan_with_names(["chrA", "chrB"])
    a = curve([(math.log(1e-4), -120.0), (math.log(1e-2), -101.255), (math.log(1.0), -130.0)],
              [(math.log(1e-3), -102.0), (math.log(1e-2), -101.255), (math.log(0.1), -104.0)],
              null_logl=-110.0, chr_=1, pos=4321)
    b = curve([(math.log(1e-4), NAN), (math.log(1e-2), NAN)], null_logl=-5.0, chr_=0, pos=7)
    e = curve([(math.log(2.0), -3.0), (math.log(4.0), -2.5)], null_logl=-5.0, chr_=0, pos=99)
    cv = np.array([a, b, e], dtype=fscl_amd.CURVE_DTYPE)
    out = tmp_path / "alpha.txt"
    fscl_amd.curve_output(out, scan, cv, 2.0)
    nan = "%1.2f" % NAN
    assert out.read_text() == (
        "chrB\t4321\t1.000e-04\t-20.00\t-\n"
        "chrB\t4321\t1.000e-03\t16.00\t-\n"
        "chrB\t4321\t1.000e-02\t17.49\t*\n"
        "chrB\t4321\t1.000e-01\t12.00\t-\n"
        "chrB\t4321\t1.000e+00\t-40.00\t-\n"
        "chrB\t4321\tsupport\t1.000e-03\t1.000e-02\t0\t0\n"
        f"chrA\t7\t1.000e-04\t{nan}\t-\n"
        f"chrA\t7\t1.000e-02\t{nan}\t-\n"
        "chrA\t7\tsupport\tNA\tNA\t0\t0\n"
        "chrA\t99\t2.000e+00\t4.00\t-\n"
        "chrA\t99\t4.000e+00\t5.00\t*\n"
        "chrA\t99\tsupport\t2.000e+00\t4.000e+00\t1\t1\n")
    fscl_amd.curve_output(out, scan, cv[2:], 0.0, label="run7")
    assert out.read_text() == ("run7\tchrA\t99\t2.000e+00\t4.00\t-\n"
                               "run7\tchrA\t99\t4.000e+00\t5.00\t*\n"
                               "run7\tchrA\t99\tsupport\t4.000e+00\t4.000e+00\t0\t1\n")
    del keep


def test_exports_and_layout(built):
    L = fscl_amd.get_lib()
    for name in ("fsclg_curve_submit", "fsclg_curve_wait", "fsclg_curve_last_ms", "fsclg_curve_forced",
                 "fscl_amd_scan_curves", "fscl_amd_scan_point_curves", "fscl_amd_curve_runs"):
        assert hasattr(L, name)
    assert fscl_amd.CURVE_DTYPE.itemsize == 64 + 8 + 2 * 8 * 27
