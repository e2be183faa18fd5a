"""The host-only side of the expected terms under the model (fscl_amd/csrc/host/expect.c) and the
NumPy restatement the GPU tests compare with (tests/expect_ref.py): no GPU is touched here.
"""
from __future__ import annotations

import math

import mpmath  # noqa: F401  (test_reference_against_mpmath pins E_M1 and E_M2 with it: without it this file fails, never skips)
import numpy as np
import pytest

import expect_ref as er
import fscl_amd
import sample_ref as sr
from util import GOLD, run_cli, run_host_check


def swept_sites(name):
    """Every site of the input that some sweep governs within log(alpha d) <= LOG_AD_MAX, and its log_ad."""
    c = sr.case(name)
    E = er.expect_model(name)
    x, which = sr.site_log_ad(E.M, c.sweeps)
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero((which >= 0) & (x <= er.LOG_AD_MAX))
    return E, idx, x[idx]


@pytest.mark.parametrize("name", sr.CASE_NAMES)
def test_inputs_keep_every_class_clear_of_exp_thresholds(built, name):
    """No class of any input has a spline value within 1.0 of exp's underflow or overflow threshold, so "usable"
    cannot flip between the device and NumPy; and Gibbs' inequality holds on unfolded, non-ascertained sites."""
    E, idx, x = swept_sites(name)
    assert len(idx) >= 300
    for shift in (-3.0, -1.0, 0.0, 1.5):   # the alphas of the GPU tests (sites past the cut drop out)
        keep = x + shift <= er.LOG_AD_MAX
        mom = er.site_moments(E, idx[keep], x[keep] + shift)
        assert mom["y_margin"].min() > 1.0, (name, shift, mom["y_margin"].min())
        if name == "asc":
            continue
        ok = ~mom["degenerate"] & (E.M.folded[idx[keep]] == 0)
        assert ok.sum() >= 100
        # on the usable classes t_f = log p_f - log q_f (no ascertainment: the null values are log q_f), so with
        # p~ = p / S, q~ = q / Q over them sum p~ log(p~ / q~) >= 0 reads m1_s >= log(S / Q), and m1_0 <= log(S / Q)
        with np.errstate(all="ignore"):
            lsq = mom["logSQ"] + np.log1p(-mom["lost_s"]) - np.log1p(-mom["lost_0"])   # S, Q over the usable classes
        tol = 1e-9
        assert (mom["m1_s"][ok] >= lsq[ok] - tol).all(), name
        assert (mom["m1_0"][ok] <= lsq[ok] + tol).all(), name


def test_reference_against_mpmath(built):
    """E_M1 and E_M2 of tests/expect_ref.py: the restatement's greatest errors against 50-digit arithmetic over
    every 25th swept site of every input, relative to sum pi |t| and sum pi t^2."""
    w1 = w2 = 0.0
    for name in sr.CASE_NAMES:
        E, idx, x = swept_sites(name)
        idx, x = idx[::25], x[::25]
        mom = er.site_moments(E, idx, x)
        for j, i in enumerate(idx):
            if mom["degenerate"][j]:
                continue
            r = er.site_moments_mp(E, int(i), float(x[j]))
            for tag in ("s", "0"):
                w1 = max(w1, float(abs(mom[f"m1_{tag}"][j] - r[f"m1_{tag}"]) / r[f"scale1_{tag}"]))
                w2 = max(w2, float(abs(mom[f"m2_{tag}"][j] - r[f"m2_{tag}"]) / r[f"scale2_{tag}"]))
    print(f"greatest errors against mpmath: m1 {w1:.3e} (E_M1 {er.E_M1:.1e}), m2 {w2:.3e} (E_M2 {er.E_M2:.1e})")
    assert w1 <= er.E_M1 and w2 <= er.E_M2
    assert w1 >= er.E_M1 / 4 and w2 >= er.E_M2 / 4, "the recorded constants are the measured ones, not a loose cover"


def test_bins(built):
    L = fscl_amd.get_lib()
    xs = np.array([-25.0, -20.0, -19.999, -8.0, 3.999, 4.0, -20.0 + 24.0 / 24 * 5, np.nextafter(-15.0, -np.inf)])
    for nb in (1, 7, 24, 64):
        assert [L.fscl_amd_expect_bin(float(v), nb) for v in xs] == list(er.bin_of(xs, nb))
    assert L.fscl_amd_expect_bin(float("nan"), 24) == 0


def crafted():
    """Two requests, 3 bins: request 0 with the alpha list (own, other), bin 1 empty and a zero SD in bin 2;
    request 1 with an empty walk."""
    tot = np.zeros((3, 4), dtype=fscl_amd.EXPECT_DTYPE)
    tot[0, 0] = (2, 0, 1.5, 1.0, 0.25, -0.5, 1.0, 0.0, 0.0)
    tot[0, 2] = (1, 1, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    tot[0, 3] = (3, 1, 1.75, 1.0, 0.25, -0.5, 1.0, 1e-3, 0.0)
    tot[1, 3] = (5, 0, 0.0, 2.0, 1.0, 0.0, 1.0, 0.0, 0.0)
    hdr = np.zeros(3, dtype=fscl_amd.SITES_DTYPE)
    hdr["pt"]["chr"] = 0
    hdr["pt"]["sweep_pos"] = [1234, 1234, 777]
    req = np.zeros(2, dtype=fscl_amd.SITE_REQ_DTYPE)
    req["pos"] = [1234, 777]
    req["lalpha"] = [math.log(1e-4), math.log(2e-3)]
    return {"n_bins": 3, "req": req, "first": np.array([0, 2, 3], dtype=np.int32), "own": np.array([0, 0], dtype=np.int32),
            "la": np.array([math.log(1e-4), math.log(1e-2), math.log(2e-3)]), "hdr": hdr, "tot": tot}


@pytest.mark.parametrize("label", [None, "run7"])
def test_writer_byte_for_byte(built, tmp, label):
    c = sr.case("d2_3")
    name = c.sweep_names[0].split(":")[0]
    out = tmp / "e.txt"
    fscl_amd.expect_output(out, c.scan, crafted(), label)
    pre = f"{label}\t" if label else ""
    want = [
        f"{pre}{name}\t1234\t1.000e-04\tbin\t-20.0000\t-12.0000\t2\t3.0000\t2.0000\t1.0000\t1.0000\t-1.0000\t2.0000\t2.0000",
        f"{pre}{name}\t1234\t1.000e-04\tbin\t-4.0000\t4.0000\t1\t0.5000\t0.0000\t0.0000\tNA\t0.0000\t0.0000\tNA",
        f"{pre}{name}\t1234\t1.000e-04\tcurve\t1.000e-04\t3\t2.0000\t1.0000\t-1.0000\t2.0000\t1.8974",
        f"{pre}{name}\t1234\t1.000e-04\tcurve\t1.000e-02\t5\t4.0000\t2.0000\t0.0000\t2.0000\t2.0000",
        f"{pre}{name}\t1234\t1.000e-04\tsummary\t3\t1\t3.5000\t2.0000\t1.0000\t1.5000\t-1.0000\t2.0000\t2.2500\t1.000e-03\t0.000e+00",
        f"{pre}{name}\t777\t2.000e-03\tcurve\t2.000e-03\t0\t0.0000\t0.0000\t0.0000\t0.0000\tNA",
        f"{pre}{name}\t777\t2.000e-03\tsummary\t0\t0\t0.0000\t0.0000\t0.0000\tNA\t0.0000\t0.0000\tNA\t0.000e+00\t0.000e+00",
    ]
    assert out.read_text() == "\n".join(want) + "\n"


def test_refusals_before_any_device_work(built, monkeypatch):
    """n_bins and n_la outside 1 .. 64, a list not ascending or outside [-20, 4], an unknown chromosome, a log alpha
    outside the range, a result above $FSCL_AMD_EXPECT_CAP: each named, each before a device is opened (this test
    runs without one)."""
    c = sr.case("d2_3")
    ok = [(0, 5000, -9.0)]
    grid = list(np.linspace(-20.0, 4.0, 33))
    n_dev = fscl_amd.get_lib().fscl_amd_n_devices()

    def refused(match, req=ok, la=grid, **kw):
        with pytest.raises(ValueError, match=match):
            fscl_amd.scan_expect(c.scan, c.tables, c.fsp, req, la, **kw)

    refused("--expect-bins", n_bins=0)
    refused("--expect-bins", n_bins=65)
    refused("--expect-alphas", la=[])
    refused("--expect-alphas", la=list(np.linspace(-20.0, 4.0, 65)))
    refused("--expect-alphas", la=[-3.0, -3.0])
    refused("--expect-alphas", la=[-21.0, 0.0])
    refused("--expect-alphas", la=[0.0, float("nan")])
    refused("--expect-sweep: unknown chromosome", req=[(1, 5000, -9.0)])
    refused("--expect-sweep: unknown chromosome", req=[(-1, 5000, -9.0)])
    refused("--expect-sweep: alpha", req=[(0, 5000, 4.5)])
    refused("--expect-sweep: alpha", req=[(0, 5000, float("nan"))])
    monkeypatch.setenv("FSCL_AMD_EXPECT_CAP", "100000")
    assert fscl_amd.get_lib().fscl_amd_expect_cap() == 100000
    refused("FSCL_AMD_EXPECT_CAP", req=ok * 3)
    monkeypatch.delenv("FSCL_AMD_EXPECT_CAP")
    assert fscl_amd.get_lib().fscl_amd_expect_cap() == 1 << 30
    # before any device work: no device context has been opened by any of the calls above
    assert fscl_amd.get_lib().fscl_amd_n_devices() == n_dev


def test_host_check_under_sanitizers(built, tmp_path):
    """tools/expect_host_check.c: the table building, the bins, the refusals and the writer under ASan and UBSan, as
    a stand-alone program (no device library, nothing loaded into Python)."""
    run_host_check("expect_host_check", ["expect.c", "util.c"], tmp_path, [tmp_path])


# ------------------------------------------------------------------ the CLI's refusals
@pytest.mark.parametrize("args, msg", [
    (["--expect-top=2"], "need --expect-file"),
    (["--expect-bins=12"], "need --expect-file"),
    (["--expect-alphas=-20:4:9"], "need --expect-file"),
    (["--expect-sweep=chr1:5000:1e-4"], "need --expect-file"),
    (["--expect-file=E", "--no-scan"], "--expect-file with --no-scan needs explicit --expect-sweep"),
    (["--expect-file=E", "--expect-top=-1"], "--expect-top must be >= 0"),
    (["--expect-file=E", "--expect-top=x"], "--expect-top must be >= 0"),
    (["--expect-file=E", "--expect-bins=0"], "--expect-bins must be 1 .. 64"),
    (["--expect-file=E", "--expect-bins=65"], "--expect-bins must be 1 .. 64"),
    (["--expect-file=E", "--expect-alphas=-20:4:64"], "--expect-alphas must be LO:HI:N"),
    (["--expect-file=E", "--expect-alphas=-21:4:10"], "--expect-alphas must be LO:HI:N"),
    (["--expect-file=E", "--expect-alphas=2:1:10"], "--expect-alphas must be LO:HI:N"),
    (["--expect-file=E", "--expect-alphas=-20:4:10x"], "--expect-alphas must be LO:HI:N"),
    (["--expect-file=E", "--expect-sweep=chr1:5000:0"], "--expect-sweep=chr1:5000:0: expected chr:pos:alpha, alpha positive"),
    (["--expect-file=E", "--expect-sweep=chr1:5000:-1e-4"], "alpha positive"),
    (["--expect-file=E", "--expect-sweep=chr1:5000:100"], "natural log within [-20, 4]"),
    (["--expect-file=E", "--expect-sweep=chr1:5000:1e-10"], "natural log within [-20, 4]"),
    (["--expect-file=E", "--expect-sweep=chr1:5000"], "expected chr:pos:alpha"),
    (["--expect-file=E", "--expect-sweep=no-such-chromosome:5000:1e-4"], "unknown chromosome name"),   # once the data is loaded
    (["--expect-file=E", "--no-scan", "--expect-sweep=no-such-chromosome:5000:1e-4"], "unknown chromosome name"),
])
def test_cli_refusals(built, tmp_path, args, msg):
    """Refused before any device work (this test runs without a device): no file is written."""
    args = [a.replace("=E", f"={tmp_path / 'e.txt'}") if a.startswith("--expect-file") else a for a in args]
    r = run_cli(args, tmp_path, snp="g1.snp")
    assert r.returncode != 0 and msg in r.stderr + r.stdout, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "e.txt").exists() and not (tmp_path / "o.txt").exists()


def test_run_keyword_refusals(built):
    for kw in (dict(expect_top=-1), dict(expect_bins=0), dict(expect_bins=65), dict(expect_alphas=(-20.0, 4.0, 64)),
               dict(expect_alphas=(-21.0, 4.0, 5))):
        with pytest.raises(ValueError):
            fscl_amd.run(GOLD / "g1.snp", None, expect_file="unused.txt", **kw)
    for kw in (dict(expect_top=2), dict(expect_bins=12), dict(expect_sweeps=[(0, 5000, 1e-4)]), dict(expect_alphas=(-20.0, 4.0, 9))):
        with pytest.raises(ValueError):
            fscl_amd.run(GOLD / "g1.snp", None, **kw)
