"""The host side of the projected p-values (no GPU): the NumPy restatement of tests/tail_ref.py against
scipy and mpmath, its own errors E_L and E_Q, the regime of every fixture of the GPU tests, the
--tail-file writer on crafted rows, the launch chunks, and the CLI's refusals."""
from __future__ import annotations

import ctypes as C
import math

import mpmath as mp
import numpy as np
import pytest
import scipy.stats as st

import fscl_amd
import tail_ref as tr
from util import GOLD, run_cli, run_host_check


def mp_logpdf(x: float, k: int, lam: float):
    h = k // 2
    x, lam = mp.mpf(float(x)), mp.mpf(float(lam))
    return (-(x + lam) / 2 - mp.log(2) + (h - 1) * mp.log(x / 2) - mp.loggamma(h) + mp.log(mp.hyp0f1(h, lam * x / 4)))


def mp_log10_q(x0: float, k: int, lam: float):
    """The Poisson double sum in plain 50-digit arithmetic (no scaling is needed there)."""
    h = k // 2
    a, b0 = mp.mpf(float(lam)) / 2, mp.mpf(float(x0)) / 2
    d, cum = mp.mpf(1), mp.mpf(0)
    for i in range(h):             # C_h = sum_{i < h} b0^i / i!
        cum += d
        d *= b0 / (i + 1)
    w, total = mp.mpf(1), mp.mpf(0)
    n = int(2 * max(float(a), math.sqrt(float(a * b0))) + 400)
    for j in range(n):             # d = b0^(h+j) / (h+j)!
        total += w * cum
        cum += d
        d *= b0 / (h + j + 1)
        w *= a / (j + 1)
    assert w * cum < total * mp.mpf(10) ** -40
    return (mp.log(total) - a - b0) / mp.log(10)


def test_reference_against_mpmath(built):
    """Measures E_L and E_Q and holds them to the constants of tail_ref.py."""
    mp.mp.dps = 50
    e_l, e_q, at_l, at_q = 0.0, 0.0, "", ""
    for c in tr.cases():
        if not c.small:
            continue
        x = c.samples[tr.positive(c.samples)].astype(np.float64)
        lams = {c.lam} | ({c.ref.lam} if c.ref.flag != tr.NOFIT else set())
        for lam in lams:
            if len(x):
                want = [mp_logpdf(v, c.k, lam) for v in x]
                err = abs(mp.mpf(tr.logl(x, c.k, lam)) - mp.fsum(want)) / mp.fsum(abs(w) for w in want)
                if float(err) > e_l:
                    e_l, at_l = float(err), c.name
            for x0 in {c.x0, 3.0}:
                if x0 > 0.0:
                    lq = mp_log10_q(x0, c.k, lam)
                    got = tr.log10_q(x0, c.k, lam)
                    assert math.isfinite(got)
                    err = abs(mp.mpf(got) - lq) / max(mp.mpf(1), abs(lq))
                    if float(err) > e_q:
                        e_q, at_q = float(err), c.name
    print(f"E_L measured {e_l:.3e} at {at_l}; E_Q measured {e_q:.3e} at {at_q}")
    assert 0.0 < e_l <= tr.E_L and tr.E_L <= 4.0 * e_l, (e_l, at_l)
    assert 0.0 < e_q <= tr.E_Q and tr.E_Q <= 4.0 * e_q, (e_q, at_q)


def test_reference_against_scipy(built):
    g = np.random.default_rng(5)
    for k in (2, 4, 6):
        for lam in (0.5, 30.0, 400.0):
            x = g.noncentral_chisquare(k, lam, 50).astype(np.float32).astype(np.float64)
            want = st.ncx2.logpdf(x, k, lam)
            got = tr.logpdf(x, k, lam)
            assert np.isfinite(want).all()
            assert np.allclose(got, want, rtol=1e-9, atol=1e-9), (k, lam, np.abs(got - want).max())
            for x0 in (0.1, float(k), lam + k, 2.0 * (lam + k) + 20.0, 1500.0):
                w = float(st.ncx2.logsf(x0, k, lam))
                q = tr.log10_q(x0, k, lam) / tr.LOG10E
                if math.isfinite(w) and w > -600.0:       # (scipy's own value is finite and not yet denormal)
                    assert abs(q - w) <= 1e-8 * max(1.0, abs(w)), (k, lam, x0, q, w)
                else:                                     # the far tail: scipy underflows, mpmath does not
                    mp.mp.dps = 50
                    w = float(mp_log10_q(x0, k, lam))
                    assert abs(q * tr.LOG10E - w) <= 64 * tr.E_Q * max(1.0, abs(w)), (k, lam, x0)
        # lam = 0 is the central chi-square
        x = g.chisquare(k, 50)
        assert np.allclose(tr.logpdf(x, k, 0.0), st.chi2.logpdf(x, k), rtol=1e-12, atol=1e-12)
        assert abs(tr.log10_q(7.5, k, 0.0) / tr.LOG10E - float(st.chi2.logsf(7.5, k))) < 1e-12
    far = tr.log10_q(1500.0, 2, 400.0)
    assert math.isfinite(far) and -80.0 < far < -75.0, far   # (e^-750 underflows; the tail is about 2e-78)
    assert tr.log10_q(0.0, 2, 30.0) == 0.0 and tr.log10_q(-3.0, 4, 30.0) == 0.0 and tr.log10_q(math.nan, 2, 1.0) == 0.0


def test_fixtures_are_in_their_regime(built):
    names = set()
    for c in tr.cases():
        f = c.ref
        names.add(c.name)
        assert f.flag == c.regime, (c.name, f.flag)
        assert f.m == len(c.samples)
        if f.flag == tr.NOFIT:
            assert f.m_pos < c.min_n and math.isnan(f.lam) and math.isnan(f.logl) and math.isnan(f.log10_q)
        elif f.flag == tr.CENTRAL:
            assert f.mean <= c.k - 1e-3 and f.lam == 0.0, (c.name, f.mean)
        else:
            assert f.mean >= c.k + 1e-3, (c.name, f.mean)
            x = c.samples[tr.positive(c.samples)]
            # the score changes sign across the final bracket, one step either side of lambda-hat
            assert f.lo <= f.lam <= f.hi
            assert tr.score(x, c.k, f.lo) >= 0.0 >= tr.score(x, c.k, f.hi), c.name
            assert f.hi - f.lo <= 1e-12 * max(1.0, f.lam)
    for k in (2, 4):
        assert {f"single_k{k}", f"w63_k{k}", f"w64_k{k}", f"w65_k{k}", f"far_k{k}", f"central_k{k}", f"zeros_k{k}",
                f"nans_k{k}"} <= names
    by = {c.name: c for c in tr.cases()}
    assert by["central_k2"].ref.flag == tr.CENTRAL and by["far_k2"].x0 == 1500.0 and by["w64_k2"].x0 == 0.0
    assert by["below_k2"].x0 < by["below_k2"].samples.min() and by["below_k2"].ref.log10_q > -1e-3
    assert math.isfinite(by["far_k2"].ref.log10_q) and -80.0 < by["far_k2"].ref.log10_q < -75.0
    assert by["mixed_k2"].ref.m == 65 and by["mixed_k2"].ref.m_pos == 60
    assert by["full_k2"].ref.m == 10000 and by["full_k2"].ref.m_pos == 8500
    _, off, _, fits = tr.batch()
    assert len(fits) == tr.BATCH_N and int(off[-1]) == sum(f.m for f in fits)
    flags = [f.flag for f in fits]
    assert min(flags.count(v) for v in (tr.FIT, tr.CENTRAL, tr.NOFIT)) >= 10
    for f in fits:   # no batch point passes or fails on a rounding of its flag
        if f.flag != tr.NOFIT:
            assert abs(f.mean - 2.0) >= 1e-3


POS = [1000, 2500, 4000, 900]
CLR = [12.345, 0.0, 250.5, 3.25]
PP = [7, 20, 0, 1]
PN = [1000, 20, 1000, 30]
CHR = [0, 0, 0, 1]


def fake_scan():
    pts = (fscl_amd.ScanPtT * 4)()
    for i, q in enumerate(pts):
        q.chr, q.sweep_pos, q.clr, q.permute_p, q.permute_n = CHR[i], POS[i], CLR[i], PP[i], PN[i]
    lim = (fscl_amd.ChrLimitsT * 2)()
    lim[0].chr, lim[0].name = 0, b"chrA"
    lim[1].chr, lim[1].name = 1, b"chrB"
    s = fscl_amd.ScanT()
    s.n_scan_pts, s.scan_pts, s.chr_limits, s.n_chromosomes = 4, pts, lim, 2
    return C.pointer(s), (pts, lim)


def test_output_format(built, tmp_path):
    scan, keep = fake_scan()
    fits = [tr.Fit(1000, 900, 5.0, 30.0, 3.1234567, -2000.0, -1.5, tr.FIT),
            tr.Fit(20, 20, 1.5, 3.0, 0.0, -30.0, 0.0, tr.CENTRAL),
            tr.Fit(1000, 800, 6.0, 28.0, 4.0, -2100.0, -203.4567, tr.FIT),
            tr.Fit(30, 4, 2.0, math.nan, math.nan, math.nan, math.nan, tr.NOFIT)]
    rows = np.zeros(4, dtype=fscl_amd.TAIL_DTYPE)
    for r, f in zip(rows, fits):
        r["m"], r["m_pos"], r["mean"], r["variance"], r["lambda"], r["logl"], r["log10_q"], r["flag"] = \
            f.m, f.m_pos, f.mean, f.variance, f.lam, f.logl, f.log10_q, f.flag
    out = tmp_path / "tail.txt"
    fscl_amd.tail_output(out, scan, rows, df=2)
    got = out.read_text().splitlines()
    assert got[0].split("\t")[:7] == ["chrA", "1000", "%1.2f" % CLR[0], "7", "1000", "900", "3.1235"]
    assert got[1] == "chrA\t2500\t0.00\t20\t20\t20\t0.0000\t0.750\t-0.000\t0.000\tcentral"
    assert got[2] == "chrA\t4000\t250.50\t0\t1000\t800\t4.0000\t1.400\t3.000\t203.554\tfit"
    assert got[3] == "chrB\t900\t3.25\t1\t30\t4\tNA\tNA\t1.477\tNA\tnofit"
    names = ["chrA", "chrA", "chrA", "chrB"]
    for i in range(4):
        assert got[i].split("\t") == tr.output_row(names[i], POS[i], CLR[i], PP[i], PN[i], fits[i], 2)
    fscl_amd.tail_output(out, scan, rows, df=4, label="run7")
    got4 = out.read_text().splitlines()
    for i in range(4):
        assert got4[i].split("\t") == tr.output_row(names[i], POS[i], CLR[i], PP[i], PN[i], fits[i], 4, "run7")
    # a variance that is not finite (one positive sample) prints NA in its own column alone
    rows[0]["variance"] = math.nan
    fscl_amd.tail_output(out, scan, rows, df=2)
    assert out.read_text().splitlines()[0].split("\t")[6:8] == ["3.1235", "NA"]
    # the summary: the calibration figure is the median over fitted points with permute_p >= 5
    s = fscl_amd.tail_summary(scan, rows, df=2)
    assert (s["n_fit"], s["n_central"], s["n_nofit"], s["n_calibration"]) == (2, 1, 1, 2)
    d0 = tr.log10_p_tail(fits[0]) - tr.log10_p_empirical(PP[0], PN[0])
    d1 = tr.log10_p_tail(fits[1]) - tr.log10_p_empirical(PP[1], PN[1])
    assert abs(s["calibration"] - 0.5 * (d0 + d1)) < 1e-12
    with pytest.raises(ValueError):
        fscl_amd.tail_output(out, scan, rows[:3])
    with pytest.raises(ValueError):
        fscl_amd.tail_output(out, scan, rows, df=3)
    with pytest.raises(OSError):
        fscl_amd.tail_output(tmp_path / "no_such_dir" / "t.txt", scan, rows)
    del keep


def test_exports_and_layout(built):
    L = fscl_amd.get_lib()
    for name in ("fsclg_tail_submit", "fsclg_tail_wait", "fsclg_tail_last_ms", "fscl_amd_tail_fit", "fscl_amd_tail_runs",
                 "fscl_amd_tail_output", "fscl_amd_tail_last_ms"):
        assert hasattr(L, name)
    assert fscl_amd.TAIL_DTYPE.itemsize == 56 and fscl_amd.TAIL_FLAGS == tr.FLAG_NAMES
    for bad in (0, 1, 3, -2, 2.5):
        with pytest.raises(ValueError):
            fscl_amd.tail_runs(np.zeros(1, np.float32), [0, 1], [1.0], df=bad)


def test_host_check_under_sanitizers(built, tmp_path):
    """tools/tail_host_check.c: the packing, chunking, summary and writer under ASan and UBSan, as a
    stand-alone program (no device library, nothing loaded into Python)."""
    run_host_check("tail_host_check", ["tail.c", "util.c"], tmp_path, [tmp_path])


def test_cli_refusals(built, tmp_path):
    t = tmp_path / "t.txt"
    for args, env, msg in (
            ([f"--tail-file={t}"], None, "--tail-file needs the permutation test"),
            ([f"--tail-file={t}", "--n-permute=0"], None, "--tail-file needs the permutation test"),
            ([f"--tail-file={t}", "--n-permute=5", "--no-scan"], None, "--tail-file needs the scan"),
            ([f"--tail-file={t}", "--n-permute=5"], {"WORLD_SIZE": "2", "RANK": "0"}, "--tail-file runs in one process"),
            ([f"--tail-file={t}", "--n-permute=5", "--tail-df=3"], None, "--tail-df must be an even integer >= 2"),
            ([f"--tail-file={t}", "--n-permute=5", "--tail-df=0"], None, "--tail-df must be an even integer >= 2"),
            ([f"--tail-file={t}", "--n-permute=5", "--tail-df=2.5"], None, "--tail-df must be an even integer >= 2"),
            ([f"--tail-file={t}", "--n-permute=5", "--tail-df=four"], None, "--tail-df must be an even integer >= 2"),
            ([f"--tail-file={t}", "--n-permute=5", "--tail-min-n=0"], None, "--tail-min-n must be >= 1")):
        r = run_cli(args, tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr + r.stdout, (args, r.returncode, r.stderr[-400:])
        assert not t.exists() and not (tmp_path / "o.txt").exists()
    with pytest.raises(ValueError):
        fscl_amd.run(GOLD / "g2.snp", None, tail_file=t)
    with pytest.raises(ValueError):
        fscl_amd.run(GOLD / "g2.snp", None, n_permute=5, tail_file=t, tail_df=3)
