"""The host side of the per-site likelihood terms (no GPU): fscl_amd_sites_summary and
fscl_amd_sites_output on hand-made headers and terms, and the CLI's refusals."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import fscl_amd
from util import GOLD, run_cli

NAN = math.nan
POS = [100 * (i + 1) for i in range(10)]           # ten sites of chromosome "chrA" ...
FREQ = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3]
DEPTH_P = [0, 1, 0, 1, 0, 0, 1, 1, 0, 0]           # ... of sample depths 20 and 12
FOLDED = [0, 0, 1, 0, 0, 1, 0, 0, 1, 0]
DEPTHS = [20, 12]


def fake_scan():
    snps = (fscl_amd.SnpT * len(POS))()
    for i, q in enumerate(snps):
        q.chr, q.pos, q.obs_freq, q.depth_p, q.folded = 0, POS[i], FREQ[i], DEPTH_P[i], FOLDED[i]
    lim = (fscl_amd.ChrLimitsT * 1)()
    lim[0].chr, lim[0].name, lim[0].start_index, lim[0].n_snps = 0, b"chrA", 0, len(POS)
    depths = (C.c_int * 2)(*DEPTHS)
    s = fscl_amd.ScanT()
    s.n_snps, s.snps, s.n_depths, s.sample_depths = len(POS), snps, 2, depths
    s.chr_limits, s.n_chromosomes = lim, 1
    return C.pointer(s), (snps, lim, depths)


def walks(*specs):
    """(headers, terms) from (nearest, nl, nr, sweep_pos, lalpha, clr, terms in walk order) each."""
    hdr = np.zeros(len(specs), dtype=fscl_amd.SITES_DTYPE)
    terms = []
    for h, (near, nl, nr, sweep, la, clr, t) in zip(hdr, specs):
        assert len(t) in (0, 1 + nl + nr)
        h["pt"]["chr"], h["pt"]["nearest_snp"], h["pt"]["sweep_pos"] = 0, near, sweep
        h["pt"]["lalpha"], h["pt"]["clr"] = la, clr
        h["nl"], h["nr"], h["len"], h["off"] = nl, nr, len(t), len(terms)
        terms += list(t)
    return hdr, np.array(terms, dtype=np.float64)


TIES = (4, 2, 3, 510, -2.0, 12.0, [1.5, 3.0, -0.25, 3.0, 0.5, -1.0])   # the greatest term twice: k = 1 and k = 3
NO_POSITIVE = (0, 0, 2, 90, -1.0, -6.0, [-1.0, 0.0, -2.0])             # clr <= 0
WITH_NAN = (9, 3, 0, 1003, -3.0, NAN, [NAN, 2.0, NAN, 1.0])            # a NaN term makes the sum, and clr, NaN
EMPTY = (5, 0, 0, 650, 9.0, 0.0, [])                                   # the nearest SNP already outside
ONE = (2, 0, 0, 301, -4.0, 0.0, [4.0])                                 # clr == 0: NA


def test_summary(built):
    scan, keep = fake_scan()
    s = fscl_amd.sites_summary(scan, *walks(TIES, NO_POSITIVE, WITH_NAN, EMPTY, ONE))
    assert s.dtype == fscl_amd.SITES_SUMMARY_DTYPE and len(s) == 5
    t = s[0]  # walk order: sites 4, 3, 2, 5, 6, 7; 3.0 at site 3 (k = 1) comes before 3.0 at site 5 (k = 3)
    assert (t["n_sites"], t["first_pos"], t["last_pos"], t["n_pos"], t["n_neg"]) == (6, 300, 800, 4, 2)
    assert (t["top_pos"], t["top_term"], t["top_share"]) == (400, 3.0, 0.5)
    assert t["n_half"] == 2  # 3.0 + 3.0 >= (3.0 + 3.0 + 1.5 + 0.5) / 2, 3.0 alone is not
    t = s[1]
    assert (t["n_sites"], t["first_pos"], t["last_pos"], t["n_pos"], t["n_neg"], t["n_half"]) == (3, 100, 300, 0, 2, 0)
    assert (t["top_pos"], t["top_term"]) == (200, 0.0) and math.isnan(t["top_share"])
    t = s[2]  # the NaNs count neither way and never are the greatest term
    assert (t["n_sites"], t["first_pos"], t["last_pos"], t["n_pos"], t["n_neg"], t["n_half"]) == (4, 700, 1000, 2, 0, 1)
    assert (t["top_pos"], t["top_term"]) == (900, 2.0) and math.isnan(t["top_share"])
    t = s[3]
    assert (t["n_sites"], t["first_pos"], t["last_pos"], t["n_pos"], t["n_neg"], t["top_pos"], t["n_half"]) == \
        (0, -1, -1, 0, 0, -1, 0)
    assert math.isnan(t["top_term"]) and math.isnan(t["top_share"])
    t = s[4]
    assert (t["n_sites"], t["top_pos"], t["top_term"], t["n_half"]) == (1, 300, 4.0, 1) and math.isnan(t["top_share"])
    del keep


def test_n_half_adds_in_descending_order(built):
    """Half of the positive sum is reached by the greatest terms first, wherever they lie in the walk;
    equal terms count in walk order, so the count does not depend on which of them is taken."""
    scan, keep = fake_scan()
    t = [0.5, 0.25, 8.0, -3.0, 0.25, 1.0, 2.0]   # positive sum 12: 8.0 alone reaches 6
    u = [1.0, 1.0, 1.0, 1.0, 1.0, -9.0, 1.0]     # positive sum 6: three of the six
    v = [0.0, -0.0, -1.0]                        # zeros are not positive
    s = fscl_amd.sites_summary(scan, *walks((4, 3, 3, 500, -2.0, 1.0, t), (4, 3, 3, 500, -2.0, 1.0, u),
                                            (1, 1, 1, 200, -2.0, 1.0, v)))
    assert s["n_half"].tolist() == [1, 3, 0] and s["n_pos"].tolist() == [6, 6, 0] and s["n_neg"].tolist() == [1, 1, 1]
    del keep


def log_ad(sweep, pos, la):
    return math.log(abs(sweep - pos)) + la


def test_output_text(built, tmp_path):
    """Rows in ascending site position (walk order is nearest, leftwards, rightwards), then the summary."""
    scan, keep = fake_scan()
    hdr, terms = walks(TIES, NO_POSITIVE, WITH_NAN, EMPTY, ONE)
    out = tmp_path / "sites.txt"
    fscl_amd.sites_output(out, scan, hdr, terms)
    nan = "%1.4f" % NAN

    def row(sweep, i, la, term):
        return (f"chrA\t{sweep}\t{POS[i]}\t{POS[i] - sweep}\t{FREQ[i]}\t{DEPTHS[DEPTH_P[i]]}\t{FOLDED[i]}\t"
                f"{log_ad(sweep, POS[i], la):1.4f}\t{term}\n")

    want = (row(510, 2, -2.0, "-0.2500") + row(510, 3, -2.0, "3.0000") + row(510, 4, -2.0, "1.5000") +
            row(510, 5, -2.0, "3.0000") + row(510, 6, -2.0, "0.5000") + row(510, 7, -2.0, "-1.0000") +
            "chrA\t510\tsummary\t6\t300\t800\t4\t2\t400\t3.0000\t0.5000\t2\n" +
            row(90, 0, -1.0, "-1.0000") + row(90, 1, -1.0, "0.0000") + row(90, 2, -1.0, "-2.0000") +
            "chrA\t90\tsummary\t3\t100\t300\t0\t2\t200\t0.0000\tNA\t0\n" +
            row(1003, 6, -3.0, "1.0000") + row(1003, 7, -3.0, nan) + row(1003, 8, -3.0, "2.0000") +
            row(1003, 9, -3.0, nan) +
            "chrA\t1003\tsummary\t4\t700\t1000\t2\t0\t900\t2.0000\tNA\t1\n"
            "chrA\t650\tsummary\t0\tNA\tNA\t0\t0\tNA\tNA\tNA\t0\n" +
            row(301, 2, -4.0, "4.0000") +
            "chrA\t301\tsummary\t1\t300\t300\t1\t0\t300\t4.0000\tNA\t1\n")
    assert out.read_text() == want
    fscl_amd.sites_output(out, scan, hdr[3:], terms, label="run7")
    assert out.read_text() == ("run7\tchrA\t650\tsummary\t0\tNA\tNA\t0\t0\tNA\tNA\tNA\t0\n"
                               "run7\t" + row(301, 2, -4.0, "4.0000") +
                               "run7\tchrA\t301\tsummary\t1\t300\t300\t1\t0\t300\t4.0000\tNA\t1\n")
    del keep


def test_terms_past_the_array_are_refused(built):
    scan, keep = fake_scan()
    hdr, terms = walks(TIES)
    with pytest.raises(ValueError):
        fscl_amd.sites_summary(scan, hdr, terms[:-1])
    del keep


def test_exports_and_layout(built):
    L = fscl_amd.get_lib()
    for name in ("fsclg_sites_submit", "fsclg_sites_wait", "fsclg_sites_last_ms", "fsclg_sites_cap",
                 "fscl_amd_scan_sites", "fscl_amd_scan_point_sites", "fscl_amd_sites_summary", "fscl_amd_sites_output"):
        assert hasattr(L, name)
    assert fscl_amd.SITES_DTYPE.itemsize == 64 + 24 and fscl_amd.SITE_REQ_DTYPE.itemsize == 16
    assert fscl_amd.SITES_SUMMARY_DTYPE.itemsize == 48


def test_sites_cap_env(built, monkeypatch):
    monkeypatch.delenv("FSCLG_SITES_CAP", raising=False)
    assert fscl_amd.sites_cap() == 1 << 22
    monkeypatch.setenv("FSCLG_SITES_CAP", "64")
    assert fscl_amd.sites_cap() == 64
    monkeypatch.setenv("FSCLG_SITES_CAP", "0")
    assert fscl_amd.sites_cap() == 1


def test_cli_refusals(built, tmp_path):
    r = run_cli([f"--sites-file={tmp_path / 's.txt'}", "--no-scan"], tmp_path)
    assert r.returncode != 0 and "--sites-file needs the scan" in r.stderr + r.stdout
    assert not (tmp_path / "s.txt").exists()
    r = run_cli([f"--sites-file={tmp_path / 's.txt'}", "--sites-top=-1"], tmp_path)
    assert r.returncode != 0 and "--sites-top must be >= 0" in r.stderr + r.stdout
    assert not (tmp_path / "s.txt").exists()
    with pytest.raises(ValueError):
        fscl_amd.run(GOLD / "g2.snp", None, sites_file=tmp_path / "s.txt", sites_top=-1)
