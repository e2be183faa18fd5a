"""fscl_amd_top_points (no GPU): the one peak selection of --surface-top, --jackknife-top, --expect-top and
--bootstrap-top, on a hand-built scan_t against a NumPy restatement of its rule; and run()'s two selections through
it (the bootstrap's peaks, the conditional scan's default given sweep) against the Python loops they replaced."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fscl_amd

NAN = float("nan")
# (chr, sweep_pos, clr, lalpha); lalpha > 0 marks the point the predicate rejects
POINTS = [
    (0, 1000, 5.0, -5.0),    # 0: 50 bp from point 1, which outranks it
    (0, 1050, 9.0, -5.0),    # 1
    (0, 5000, 7.0, -5.0),    # 2: ties with 3, scan order decides
    (0, 9000, 7.0, -5.0),    # 3
    (0, 12000, NAN, -5.0),   # 4: a NaN CLR is never picked
    (0, 12050, 0.5, -5.0),   # 5: next to the NaN point, which blocks nothing
    (1, 1000, 4.0, -5.0),    # 6: 50 bp from point 1, but on the other chromosome
    (1, 20000, 8.0, -5.0),   # 7: 80 bp below the rejected point 8, 160 bp from 9
    (1, 20080, 8.5, 1.0),    # 8: rejected; without the predicate it outranks and blocks 7 and 9
    (1, 20160, 6.0, -5.0),   # 9
    (1, 30000, 3.0, -5.0),   # 10
    (1, 30100, 2.0, -5.0),   # 11: exactly 100 bp from 10
    (1, 30201, 1.0, -5.0),   # 12: 201 bp from 10, 101 from 11
]


@pytest.fixture(scope="module")
def scan(built):
    pts = (fscl_amd.ScanPtT * len(POINTS))()
    for p, (c, pos, clr, la) in zip(pts, POINTS):
        p.chr, p.sweep_pos, p.clr, p.lalpha = c, pos, clr, la
    s = fscl_amd.ScanT()
    s.n_scan_pts, s.scan_pts, s.n_chromosomes = len(POINTS), pts, 2
    return C.pointer(s), pts  # (pts is kept alive with the scan)


def restated(top, spacing, ok=None):
    c, pos, clr, _ = (np.array(v) for v in zip(*POINTS))
    order = [i for i in np.argsort(-np.nan_to_num(clr, nan=-np.inf), kind="stable") if not np.isnan(clr[i])]
    chosen = []
    for i in order:
        if len(chosen) == top:
            break
        if any(c[j] == c[i] and abs(int(pos[i]) - int(pos[j])) <= spacing for j in chosen):
            continue
        if ok is not None and not ok[i]:
            continue
        chosen.append(int(i))
    return chosen


@pytest.mark.parametrize("spacing", [0, 49, 50, 100, 101])
@pytest.mark.parametrize("top", [0, 1, 4, len(POINTS), 100])
def test_matches_restatement(scan, top, spacing):
    s, _ = scan
    ok = [la <= 0.0 for _, _, _, la in POINTS]
    assert fscl_amd.top_points(s, top, spacing).tolist() == restated(top, spacing)
    assert fscl_amd.top_points(s, top, spacing, accept=lambda p: p.lalpha <= 0.0).tolist() == restated(top, spacing, ok)


def test_the_rule_case_by_case(scan):
    s, _ = scan
    every = fscl_amd.top_points(s, 100, 100).tolist()
    assert every == [1, 8, 2, 3, 6, 10, 12, 5]  # 0, 7, 9, 11 within 100 bp of a chosen point; 4 is NaN
    assert every.index(2) < every.index(3)  # equal CLRs keep scan order
    assert 4 not in every and 5 in every
    assert 0 not in every and 6 in every    # 50 bp apart: blocked on one chromosome, free across two
    kept = fscl_amd.top_points(s, 100, 100, accept=lambda p: p.lalpha <= 0.0).tolist()
    assert kept == [1, 7, 2, 3, 9, 6, 10, 12, 5]  # the rejected 8 is gone and blocks neither 7 nor 9
    assert fscl_amd.top_points(s, 0, 100).tolist() == []
    assert fscl_amd.top_points(s, 3, 100).tolist() == every[:3]
    assert fscl_amd.get_lib().fscl_amd_top_points(None, 1, 100, fscl_amd.TOP_ACCEPT_FN(), None) == -1
    assert fscl_amd.get_lib().fscl_amd_top_points(s, 1, 100, fscl_amd.TOP_ACCEPT_FN(), None) == -1


# ------------------------------------------------------------------ the selections of run()
# (chr, sweep_pos, clr, lalpha) for run()'s two peak selections: the bootstrap's (--bootstrap-top) and the
# conditional scan's default given sweep
RUN_POINTS = [
    (0, 1000, 6.0, -5.0),     # 0: ties with 2, scan order decides
    (0, 1300, 5.0, -4.0),     # 1: 300 bp from 0 on its chromosome
    (0, 9000, 6.0, -3.0),     # 2
    (0, 20000, NAN, -5.0),    # 3: a NaN CLR is never picked
    (0, 30000, 9.0, 800.0),   # 4: the greatest CLR, but exp(lalpha) overflows: the sampler would refuse it
    (0, 30100, 4.0, -2.0),    # 5: 100 bp from 4, which blocks nothing
    (1, 1000, 5.5, -6.0),     # 6: 0 bp from 0, on the other chromosome
    (1, 50000, 8.0, -800.0),  # 7: exp(lalpha) underflows to 0: refused
    (1, 50200, 7.0, NAN),     # 8: no alpha at all: refused
    (1, 70000, 3.0, 0.0),     # 9
]


def removed_bootstrap_loop(p, bootstrap_top, win):
    """The peak selection run() spelled out before it called top_points, kept here word for word."""
    boot_sw = []
    for i in sorted((i for i in range(len(p)) if p["clr"][i] == p["clr"][i]), key=lambda i: -p["clr"][i]):
        if len(boot_sw) >= int(bootstrap_top):
            break
        a = float(np.exp(p["lalpha"][i]))
        if any(c == p["chr"][i] and abs(int(p["sweep_pos"][i]) - q) <= win for c, q, _ in boot_sw) or \
                not (0.0 < a < np.inf):
            continue
        boot_sw.append((int(p["chr"][i]), int(p["sweep_pos"][i]), a))
    return boot_sw


@pytest.fixture(scope="module")
def run_scan(built):
    pts = (fscl_amd.ScanPtT * len(RUN_POINTS))()
    for p, (c, pos, clr, la) in zip(pts, RUN_POINTS):
        p.chr, p.sweep_pos, p.clr, p.lalpha = c, pos, clr, la
    s = fscl_amd.ScanT()
    s.n_scan_pts, s.scan_pts, s.n_chromosomes = len(RUN_POINTS), pts, 2
    return C.pointer(s), pts


@pytest.mark.filterwarnings("ignore:overflow encountered in exp")
@pytest.mark.parametrize("win", [0, 99, 100, 299, 300, 100000])
@pytest.mark.parametrize("top", [0, 1, 3, 5, len(RUN_POINTS), 100])
def test_bootstrap_selection_is_the_removed_loop(run_scan, top, win):
    s, _ = run_scan
    p = fscl_amd.points(s)
    idx = fscl_amd.top_points(s, top, win, accept=fscl_amd._sampler_takes_alpha)
    got = [(int(p["chr"][i]), int(p["sweep_pos"][i]), float(np.exp(p["lalpha"][i]))) for i in idx]
    assert got == removed_bootstrap_loop(p, top, win)
    assert not {4, 7, 8, 3} & set(idx.tolist())


def test_bootstrap_selection_case_by_case(run_scan):
    s, _ = run_scan
    take = fscl_amd._sampler_takes_alpha
    assert fscl_amd.top_points(s, 100, 300, accept=take).tolist() == [0, 2, 6, 5, 9]   # 1 is within 300 bp of 0
    assert fscl_amd.top_points(s, 100, 299, accept=take).tolist() == [0, 2, 6, 1, 5, 9]
    assert fscl_amd.top_points(s, 2, 0, accept=take).tolist() == [0, 2]                # the tie keeps scan order
    assert [take(q) for q in s.contents.scan_pts[:10]] == [True, True, True, True, False, True, True, False, False, True]


def test_conditional_default_is_the_removed_maximum(run_scan, scan):
    """top_points(scan, 1, 0) against the max(..., key=(clr, -i)) run() took its default given sweep with."""
    for s, _ in (run_scan, scan):
        p = fscl_amd.points(s)
        ok = [i for i in range(len(p)) if p["clr"][i] == p["clr"][i]]
        i = max(ok, key=lambda i: (p["clr"][i], -i))
        assert fscl_amd.top_points(s, 1, 0).tolist() == [i]
    pts = (fscl_amd.ScanPtT * 3)()
    for q, clr in zip(pts, (NAN, 2.0, 2.0)):
        q.clr = clr
    t = fscl_amd.ScanT()
    t.n_scan_pts, t.scan_pts, t.n_chromosomes = 3, pts, 1
    assert fscl_amd.top_points(C.pointer(t), 1, 0).tolist() == [1]   # the first of the tie, never the NaN
    t.n_scan_pts = 1
    assert fscl_amd.top_points(C.pointer(t), 1, 0).tolist() == []    # NaN alone: no default sweep, as `ok` was empty
