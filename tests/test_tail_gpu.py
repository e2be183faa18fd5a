"""The projected-tail fit on the GPU (tail_kernel through fsclg_tail_submit, fscl_amd_tail_runs,
fscl_amd_tail_fit) against the NumPy restatement of tests/tail_ref.py.

Per point: flag, m and m_pos equal the reference's; logl is the reference's l at the device's own
lambda-hat within max(64 E_L, m 2^-52) sum |log f_i|; that l is no lower than the reference's own
maximum by more than the same; log10_q is the reference's at the device's lambda-hat within
max(64 E_Q, m 2^-52) max(1, |log10 Q|).  The fixtures' regimes are checked on the CPU
(tests/test_tail_host.py), so no case turns on a rounding of its flag.
The far-tail case, x0 = 1 500 over lambda = 400, has log10 Q = -77.3 (mpmath agrees; not the -200 first
guessed for it): e^-750 underflows in double all the same, and the value must come out finite.
"""
from __future__ import annotations

import math
import subprocess

import numpy as np
import pytest

import fscl_amd
import tail_ref as tr
from util import CLI, GOLD

pytestmark = pytest.mark.gpu


def runs(samples, offsets, x0, k, min_n):
    try:
        return fscl_amd.tail_runs(samples, offsets, x0, k, min_n)
    except RuntimeError as e:  # a device error: nothing more runs on the GPU in this session
        pytest.exit(f"tail_runs: {e}", returncode=3)


def check_point(name, row, samples, x0, k, want: tr.Fit):
    assert (int(row["flag"]), int(row["m"]), int(row["m_pos"])) == (want.flag, want.m, want.m_pos), name
    if want.m_pos:
        assert abs(row["mean"] - want.mean) <= want.m * 2.0 ** -52 * abs(want.mean), name
    else:
        assert math.isnan(row["mean"]), name
    if want.m_pos > 1:
        assert abs(row["variance"] - want.variance) <= 4 * want.m * 2.0 ** -52 * want.variance + 1e-300, name
    else:
        assert math.isnan(row["variance"]), name
    if want.flag == tr.NOFIT:
        assert math.isnan(row["lambda"]) and math.isnan(row["logl"]) and math.isnan(row["log10_q"]), name
        return
    lam = float(row["lambda"])
    assert (lam == 0.0) if want.flag == tr.CENTRAL else (lam > 0.0 and math.isfinite(lam)), (name, lam)
    x = samples[tr.positive(samples)]
    l_at = tr.logl(x, k, lam)
    tol = tr.tol_l(want)
    print(f"{name}: lambda {lam!r} (ref {want.lam!r}) logl err {abs(row['logl'] - l_at):.3e} tol {tol:.3e} "
          f"search {want.logl - l_at:.3e}")
    assert abs(row["logl"] - l_at) <= tol, (name, row["logl"], l_at, tol)              # the evaluation
    assert l_at >= want.logl - tol, (name, l_at, want.logl, tol)                        # the search
    lq = tr.log10_q(x0, k, lam)
    tq = tr.tol_q(want, lq)
    print(f"{name}: log10_q {row['log10_q']!r} ref {lq!r} tol {tq:.3e}")
    assert math.isfinite(row["log10_q"]) and abs(row["log10_q"] - lq) <= tq, (name, row["log10_q"], lq, tq)


GROUPS = sorted({(c.k, c.min_n) for c in tr.cases() if c.small})


@pytest.mark.parametrize("k,min_n", GROUPS)
def test_small_fixtures(built, k, min_n):
    cs = [c for c in tr.cases() if c.small and (c.k, c.min_n) == (k, min_n)]
    off = np.concatenate([[0], np.cumsum([len(c.samples) for c in cs])]).astype(np.uint64)
    rows = runs(np.concatenate([c.samples for c in cs]), off, [c.x0 for c in cs], k, min_n)
    assert rows.dtype == fscl_amd.TAIL_DTYPE and len(rows) == len(cs)
    for c, r in zip(cs, rows):
        check_point(c.name, r, c.samples, c.x0, k, c.ref)
    assert fscl_amd.tail_last_ms() > 0.0
    by = {c.name: r for c, r in zip(cs, rows)}
    if f"far_k{k}" in by:      # e^-750 underflows; the projection does not
        assert math.isfinite(by[f"far_k{k}"]["log10_q"]) and -82.0 < by[f"far_k{k}"]["log10_q"] < -73.0
        assert by[f"w64_k{k}"]["log10_q"] == 0.0                      # x0 = 0: p_tail = m_pos / m
        assert -1e-3 < by[f"below_k{k}"]["log10_q"] <= 0.0


def test_full_record(built):
    c = next(c for c in tr.cases() if c.name == "full_k2")
    rows = runs(c.samples, [0, len(c.samples)], [c.x0], c.k, c.min_n)
    check_point(c.name, rows[0], c.samples, c.x0, c.k, c.ref)
    assert fscl_amd.tail_last_ms() > 0.0


def test_batch_in_one_launch(built):
    samples, off, x0, fits = tr.batch()
    rows = runs(samples, off, x0, 2, 20)
    assert len(rows) == tr.BATCH_N
    for p, f in enumerate(fits):
        check_point(f"batch[{p}]", rows[p], samples[int(off[p]):int(off[p + 1])], float(x0[p]), 2, f)
    again = runs(samples, off, x0, 2, 20)
    assert again.tobytes() == rows.tobytes(), "two launches of one input differ"
    # chunked launches give the same rows (the cap counts floats; a point never splits)
    import os
    os.environ["FSCL_AMD_TAIL_CAP"] = "1000"
    try:
        chunked = runs(samples, off, x0, 2, 20)
    finally:
        del os.environ["FSCL_AMD_TAIL_CAP"]
    assert chunked.tobytes() == rows.tobytes()


def test_errors(built):
    x = np.ones(10, dtype=np.float32)
    for off, cnt in (([0, 20], None), ([5], [6]), ([0], [-1])):
        with pytest.raises(RuntimeError, match="code -1"):
            fscl_amd.tail_runs(x, off, [1.0], 2, 20, counts=cnt)
    rows = runs(x, [0, 10], [1.0], 2, 5)   # the context still works
    assert rows[0]["flag"] == tr.CENTRAL and rows[0]["m_pos"] == 10
    assert len(runs(np.zeros(0, np.float32), [0], [], 2, 20)) == 0


def tail_rows_of(scan, k, min_n, label=None):
    s = scan.contents
    recs = fscl_amd.tail_records(scan)
    want = []
    for i in range(s.n_scan_pts):
        q = s.scan_pts[i]
        f = tr.fit(recs[i], q.clr, k, min_n)
        want.append((tr.output_row(s.chr_limits[q.chr].name.decode(), q.sweep_pos, q.clr, q.permute_p, q.permute_n, f, k, label), f))
    return want


def compare_file(path, want, k, shift=0):
    got = [ln.split("\t") for ln in path.read_text().splitlines()]
    assert len(got) == len(want) > 0
    n_fit = 0
    for g, (w, f) in zip(got, want):
        lam_c, vr_c, pt_c = 6 + shift, 7 + shift, 9 + shift
        for c in range(len(w)):
            if c in (lam_c, vr_c, pt_c) and w[c] != "NA":
                # a fitted column: within the tolerance of the fit plus half a unit of the last printed digit
                digits = 4 if c == lam_c else 3
                tol = 0.5 * 10.0 ** -digits + 1e-9 * max(1.0, abs(float(w[c])))
                assert g[c] != "NA" and abs(float(g[c]) - float(w[c])) <= 2 * tol, (g, w)
            else:
                assert g[c] == w[c], (g, w)
        n_fit += f.flag == tr.FIT
    return n_fit


@pytest.mark.parametrize("mode", ["bisection", "grid"])
def test_cli_end_to_end(built, tmp_path, mode):
    out, tail, tail2 = tmp_path / "o.txt", tmp_path / "t.txt", tmp_path / "t2.txt"
    extra = ["--scan-mode=grid", "-g", "5000"] if mode == "grid" else []
    cmd = [str(CLI), "-f", str(GOLD / "g2.snp"), "-o", str(out), "--n-permute=30", f"--tail-file={tail}", "--prepend-label=L"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Tail fit: df 2" in r.stderr + r.stdout
    base = tmp_path / "base.txt"
    r = subprocess.run([str(CLI), "-f", str(GOLD / "g2.snp"), "-o", str(base), "--n-permute=30", "--prepend-label=L"] + extra,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == base.read_bytes(), "--tail-file changed the -o output"
    kw = dict(scan_mode="grid", small_grid_sp=5000) if mode == "grid" else {}
    scan = fscl_amd.run(GOLD / "g2.snp", tmp_path / "o2.txt", n_permute=30, tail_file=tail2, label="L", verbosity=0, **kw)
    assert (tmp_path / "o2.txt").read_bytes() == out.read_bytes()
    if mode == "bisection":
        plain = tmp_path / "plain.txt"
        fscl_amd.scan_output(plain, scan, False, 30, None)
        assert plain.read_bytes() == (GOLD / "g2_p30.out").read_bytes()
    assert tail2.read_bytes() == tail.read_bytes(), "run(tail_file=) and the CLI differ"
    want = tail_rows_of(scan, 2, 20, "L")
    compare_file(tail, want, 2, shift=1)
    # with a lower threshold more points are fitted; df = 4 goes through the same path
    rows = fscl_amd.tail_fit(scan, 4, 5)
    recs = fscl_amd.tail_records(scan)
    s = scan.contents
    n_fitted = 0
    for i in range(s.n_scan_pts):
        f = tr.fit(recs[i], s.scan_pts[i].clr, 4, 5)
        check_point(f"{mode}[{i}]", rows[i], recs[i], s.scan_pts[i].clr, 4, f)
        n_fitted += f.flag != tr.NOFIT
    assert n_fitted > 0
    summ = fscl_amd.tail_summary(scan, rows, 4, 5)
    assert summ["n_fit"] + summ["n_central"] + summ["n_nofit"] == s.n_scan_pts
