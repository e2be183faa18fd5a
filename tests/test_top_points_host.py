"""fscl_amd_top_points (no GPU): the one peak selection of --surface-top, --jackknife-top, --expect-top and
--bootstrap-top, on a hand-built scan_t against a NumPy restatement of its rule."""
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
