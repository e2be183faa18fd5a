"""The conditional sweep scan (include/fscl_amd.h, --conditional-file) restated in NumPy on tests/walk_ref.py.

Ownership by brute force over the sites (every site goes to the sweep of least distance, a tie to the lower
position, then to the first listed, the given sweeps listed before the candidate); the clipped value V from
walk_ref.walk_terms and seq_sum, the site indices taken from the returned part lengths; the given sweeps'
terms G, the base A (a sequential sum from +0.0 in ascending site index) and cond_clr = 2 ((V - N) - A).
"""
from __future__ import annotations

import math

import numpy as np

import walk_ref as wr


def init_point(pos, cs: int, cn: int, x: int, er: int):
    """init_scan_result's geometry (scan-chromosome.c:58-101) for a position x of the chromosome whose sites are
    pos[cs : cs + cn] of the concatenated, sorted-per-chromosome positions: (nearest, sweep_pos, window_start,
    window_end), global indices.  The de-collision compares a global index with the chromosome's count (Q3)."""
    a = pos[cs:cs + cn]
    i, j = 0, cn
    while j - i > 1:
        m = (i + j) // 2
        if a[m] < x:
            i = m
        else:
            j = m
    if j == cn:
        near = cn - 1
    elif (x - int(a[i])) < (int(a[j]) - x):
        near = i
    else:
        near = j
    near += cs
    k = near
    while k < cn and int(pos[k]) == x:
        x += 1
        k += 1
    z = cs + cn - 1
    if near - er < cs:
        ws, we = cs, min(cs + 2 * er, z)
    elif near + er > z:
        we, ws = z, max(z - 2 * er, cs)
    else:
        ws, we = near - er, near + er
    return near, x, ws, we


def owners(site_pos, sweeps):
    """Index into ``sweeps`` (positions, in list order) of the sweep that owns each site: brute force."""
    x = np.asarray(site_pos, dtype=np.int64)
    sw = np.asarray(sweeps, dtype=np.int64)
    best = np.zeros(len(x), dtype=np.int64)
    bd = np.abs(x - sw[0])
    for k in range(1, len(sw)):  # every site against every sweep, in list order
        d = np.abs(x - sw[k])
        take = (d < bd) | ((d == bd) & (sw[k] < sw[best]))
        best[take], bd[take] = k, d[take]
    return best


def clip(pos, cs: int, cn: int, given_pos, s: int):
    """(lo, hi), global site indices: the sites of the chromosome the candidate at s owns against the given sweeps
    at ``given_pos`` (listed before it); lo > hi when it owns none.  The owned sites are checked to be one interval."""
    if cn <= 0:
        return cs + 1, cs
    own = owners(pos[cs:cs + cn], list(given_pos) + [s]) == len(given_pos)
    idx = np.flatnonzero(own)
    if len(idx) == 0:
        return cs + 1, cs
    assert idx[-1] - idx[0] + 1 == len(idx), "the candidate's sites are not one interval"
    return cs + int(idx[0]), cs + int(idx[-1])


def walk_sites(pt: wr.Point, lens):
    """The global site index of each term of a walk, in walk order, from its (left, right) part lengths."""
    nl, nr = lens
    if nl < 0:
        return np.zeros(0, dtype=np.int64)
    k = pt.nearest_snp
    return np.concatenate([[k], np.arange(k - 1, k - 1 - nl, -1), np.arange(k + 1, k + 1 + nr)]).astype(np.int64)


def clipped_value(T: wr.Tables, pt: wr.Point, la: float, lo: int, hi: int, walk=None):
    """(V, the number of terms): the null sum plus the walk's terms whose sites lie in [lo, hi], in walk order.
    ``walk``: (terms, lens) of walk_terms(T, pt, la) when the caller has them."""
    t, lens = walk if walk is not None else wr.walk_terms(T, pt, la)
    idx = walk_sites(pt, lens)
    keep = (idx >= lo) & (idx <= hi)
    return wr.seq_sum(float(pt.null_logl), t[keep])[0], int(np.count_nonzero(keep))


def row_maximum(values, las):
    """The first strict maximum in list order from the (LOG_AD_MAX, -DBL_MAX) state: (lalpha, value)."""
    best, bla = -wr.DBL_MAX, wr.LOG_AD_MAX
    for v, a in zip(values, las):
        if v > best:
            best, bla = float(v), float(a)
    return bla, best


def given_terms(T: wr.Tables, pos, cs: int, cn: int, given, er: int):
    """G[cn]: for every site of the chromosome the term it has in the walk of the given sweep that owns it among
    ``given`` = [(pos, alpha)], at log alpha (math.log, the C library's), +0.0 where it is not in that walk."""
    g = np.zeros(cn, dtype=np.float64)
    if not given:
        return g
    own = owners(pos[cs:cs + cn], [q for q, _ in given])
    for k, (q, alpha) in enumerate(given):
        near, sweep, ws, we = init_point(pos, cs, cn, int(q), er)
        pt = wr.Point(near, sweep, ws, we, 0.0)
        t, lens = wr.walk_terms(T, pt, math.log(alpha))
        for site, term in zip(walk_sites(pt, lens), t):
            if own[site - cs] == k:
                g[site - cs] = term
    return g


def base(g, cs: int, lo: int, hi: int, ws: int, we: int):
    """(A, n): the strictly sequential sum of g over the sites of [lo, hi] inside [ws, we], ascending from +0.0."""
    a, b = max(lo, ws), min(hi, we)
    if a > b:
        return 0.0, 0
    with np.errstate(all="ignore"):
        return float(np.add.accumulate(np.concatenate([[0.0], g[a - cs:b - cs + 1]]))[-1]), b - a + 1


def cond_clr(v: float, n: float, a: float) -> float:
    with np.errstate(all="ignore"):
        return float(np.float64(2.0) * ((np.float64(v) - np.float64(n)) - np.float64(a)))
