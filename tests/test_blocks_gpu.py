"""The block sums of the likelihood surface (fsclg_blocks_submit) and the delete-one-block jackknife
(--jackknife-file) on the GPU.

Every block sum and count is compared by bit pattern (NaN equal to NaN) with tests/blocks_ref.py -- the
walk's terms of tests/walk_ref.py in ascending site index, grouped by block, each group summed from +0.0 --
on the record's own point; the golden case compares with the block folds of scan_sites' terms instead
(the existing kernel as an independent reference).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
import subprocess

import numpy as np
import pytest

import blocks_ref as br
import cond_ref as cr
import fscl_amd
import walk_ref as wr
from fscl_amd import synth
from util import CLI, GOLD

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
RAW = fscl_amd._POINT_RAW
CASE_ER = 5000  # above every window of walk_ref's geometry: each chromosome is one whole-chromosome window
E_ARG, E_STATE = -1, -3


class BlkT(C.Structure):  # fsclg_blocks_t
    _fields_ = [("block_bp", C.c_int32), ("b0", C.c_int32), ("nb", C.c_int32), ("pad", C.c_int32)]


def sentinel(n, dtype):
    a = np.zeros(max(n, 1), dtype=dtype)
    a.view(np.uint8)[:] = SENTINEL
    return a


def untouched(a):
    return (a.view(np.uint8) == SENTINEL).all()


def no_sentinel(pts, bs, cnt, what):
    w = pts.view(np.uint8).reshape(len(pts), -1).view(np.uint32)
    assert not (w == 0xA5A5A5A5).any(), f"{what}: a point was left unwritten"
    assert not (bs.view(np.uint64) == 0xA5A5A5A5A5A5A5A5).any(), f"{what}: a sum was left unwritten"
    assert not (cnt == 0xA5A5A5A5).any(), f"{what}: a count was left unwritten"


def grid(n, lo=-7.0, hi=wr.LOG_AD_MAX):
    """n ascending log alphas; from -7 up the walks of walk_ref's geometry (|d| < 2^14) end at different sites."""
    return [-3.0] if n == 1 else [hi if i == n - 1 else lo + i * ((hi - lo) / (n - 1)) for i in range(n)]


def device_guard(fn):
    """A device error ends the session: nothing more runs on the GPU after it."""
    @functools.wraps(fn)
    def run(*a, **kw):
        try:
            return fn(*a, **kw)
        except RuntimeError as e:
            pytest.exit(f"{fn.__name__}: {e}", returncode=3)
    return run


class BlkShim(wr.Shim):
    def __init__(self):
        super().__init__()
        L, vp = self.L, C.c_void_p
        L.fsclg_blocks_submit.restype = C.c_int
        L.fsclg_blocks_submit.argtypes = [vp, C.c_int, C.c_int, C.POINTER(wr.RunT), C.c_int, vp, C.c_int, C.POINTER(BlkT), C.c_int]
        L.fsclg_blocks_wait.restype, L.fsclg_blocks_wait.argtypes = C.c_int, [vp, C.c_int, vp, vp, vp]
        L.fsclg_blocks_last_ms.restype, L.fsclg_blocks_last_ms.argtypes = C.c_double, [vp, C.c_int]
        L.fsclg_surface_submit.restype = C.c_int
        L.fsclg_surface_submit.argtypes = [vp, C.c_int, C.c_int, C.POINTER(wr.RunT), C.c_int, vp, C.c_int, C.c_int]
        L.fsclg_surface_wait.restype, L.fsclg_surface_wait.argtypes = C.c_int, [vp, C.c_int, vp, vp]
        L.fsclg_slot_set_rows.restype, L.fsclg_slot_set_rows.argtypes = C.c_int, [vp, C.c_int, vp, vp]

    def submit(self, runs, las, blk, er, batch=0, slot=0):
        run = (wr.RunT * max(len(runs), 1))(*[wr.RunT(*r) for r in runs])
        la = np.ascontiguousarray(las, dtype=np.float64).reshape(max(len(runs), 1), -1)
        b = (BlkT * max(len(blk), 1))(*[BlkT(*q, 0) for q in blk])
        return self.L.fsclg_blocks_submit(self.ctx, batch, slot, run, len(runs), la.ctypes.data, la.shape[1], b, er)

    def set_null(self, N, n_chr, slot=0):
        nul = (C.c_double * n_chr)(*([N] * n_chr))
        self._ok(self.L.fsclg_slot_set_rows(self.ctx, slot, None, nul), "fsclg_slot_set_rows")

    def blocks(self, runs, las, blk, er, N, n_chr, batch=0, slot=0):
        """(points, [bs [count][nb][n_la] per run], [cnt ... per run]) on the uploaded rows set into `slot` with
        the whole-chromosome null sums N; the outputs are prefilled with a sentinel."""
        self.set_null(N, n_chr, slot)
        total, k = sum(r[3] for r in runs), len(las[0])
        nc = sum(r[3] * q[2] for r, q in zip(runs, blk)) * k
        pts, bs, cnt = sentinel(total, RAW), sentinel(nc, np.float64), sentinel(nc, np.uint32)
        self._ok(self.submit(runs, las, blk, er, batch, slot), "fsclg_blocks_submit")
        self._ok(self.L.fsclg_blocks_wait(self.ctx, batch, pts.ctypes.data, bs.ctypes.data, cnt.ctypes.data), "fsclg_blocks_wait")
        pts, bs, cnt = pts[:total], bs[:nc], cnt[:nc]
        no_sentinel(pts, bs, cnt, "blocks")
        obs, ocnt, o = [], [], 0
        for r, q in zip(runs, blk):
            m = r[3] * q[2] * k
            obs.append(bs[o:o + m].reshape(r[3], q[2], k))
            ocnt.append(cnt[o:o + m].reshape(r[3], q[2], k))
            o += m
        return pts, obs, ocnt

    def surface(self, runs, las, er, batch=0, slot=0):
        total, k = sum(r[3] for r in runs), len(las[0])
        run = (wr.RunT * len(runs))(*[wr.RunT(*r) for r in runs])
        la = np.ascontiguousarray(las, dtype=np.float64).reshape(len(runs), -1)
        pts, sm = sentinel(total, RAW), sentinel(total * k, np.float64)
        self._ok(self.L.fsclg_surface_submit(self.ctx, batch, slot, run, len(runs), la.ctypes.data, k, er), "fsclg_surface_submit")
        self._ok(self.L.fsclg_surface_wait(self.ctx, batch, pts.ctypes.data, sm.ctypes.data), "fsclg_surface_wait")
        return pts[:total], sm[:total * k].reshape(total, k)


@pytest.fixture(scope="module")
def shim(built):
    s = BlkShim()
    yield s
    s.close()


def case_chromosomes():
    """The 15 windows of walk_ref.geometry() as 15 chromosomes (as the curve tests take them)."""
    g, n = wr.geometry()
    start = [q.ws for q in g]
    return start, [b - a for a, b in zip(start, start[1:] + [n])]


def point_of(q):
    return wr.Point(int(q["nearest_snp"]), int(q["sweep_pos"]), int(q["window_start"]), int(q["window_end"]),
                    float(q["null_logl"]))


def same_arrays(got, want):
    """Equal by bit pattern, NaN equal to NaN."""
    g, w = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))


def check_blocks(pts, obs, ocnt, runs, las, blk, T, what, bad):
    """Every cell against blocks_ref on the record's own point; every count sum against the walk's length; the
    point against the fold of its own block sums."""
    p = 0
    for i, (r, q) in enumerate(zip(runs, blk)):
        la = las[i]
        for t in range(r[3]):
            pt = point_of(pts[p])
            wbs, wcnt = br.block_sums(T, pt, la, *q)
            ok = same_arrays(obs[i][t], wbs) & (ocnt[i][t] == wcnt)
            for j, k in zip(*np.nonzero(~ok)):
                bad.append(f"{what} run {i} position {t} block {j} la[{k}]: ({float(obs[i][t][j][k]).hex()}, {ocnt[i][t][j][k]}) != "
                           f"({float(wbs[j][k]).hex()}, {wcnt[j][k]})")
            for k, a in enumerate(la):
                nl, nr = wr.walk_terms(T, pt, float(a))[1]
                want_len = 0 if nl < 0 else 1 + nl + nr
                if int(ocnt[i][t][:, k].sum()) != want_len:
                    bad.append(f"{what} run {i} position {t} la[{k}]: {int(ocnt[i][t][:, k].sum())} terms != walk length {want_len}")
            v = br.fold(obs[i][t][None])[0]
            best, bla, bv = -wr.DBL_MAX, wr.LOG_AD_MAX, None
            with np.errstate(all="ignore"):
                for k, a in enumerate(la):
                    w = float(np.float64(v[k]) + np.float64(pt.null_logl))
                    if w > best:
                        best, bla, bv = w, float(a), float(v[k])
                clr = 2.0 * bv if bv is not None else float(np.float64(2.0) * (np.float64(best) - np.float64(pt.null_logl)))
            g = pts[p]
            if not (wr.same(float(g["lalpha"]), bla) and wr.same(float(g["sm_logl"]), best) and wr.same(float(g["clr"]), clr)):
                bad.append(f"{what} run {i} position {t}: point ({g['lalpha']!r}, {g['sm_logl']!r}, {g['clr']!r}) != "
                           f"({bla!r}, {best!r}, {clr!r})")
            p += 1


def same_geometry(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("chr", "nearest_snp", "sweep_pos", "window_start", "window_end", "n_snps"))


def shifted(T, shift):
    return dataclasses.replace(T, pos=(T.pos.astype(np.int64) + shift).astype(np.int32))


# ------------------------------------------------------------------ 1. block sizes, boundaries, list lengths
SIZES = [(bp, off) for bp in (2, 126, 128, 130) for off in (0, -1, 1)] + [(2 ** 30, 0)]


@pytest.mark.parametrize("case", range(len(SIZES)))
def test_block_sizes(shim, case):
    """Blocks of 1, 63, 64, 65 sites and one block for everything.  The sites are shifted so that a block
    boundary falls on the nearest SNP of one window (another one per case), one site left of it or one site
    right of it, and b0 puts that boundary in the middle of the nb blocks; the other 14 windows meet the
    same blocks elsewhere.  One position per window, on a site (even windows) or between two (odd ones)."""
    bp, off = SIZES[case]
    n_la = (1, 2, 33, 64)[case % 4]
    c = wr.cases()["edge-nonneg"]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    kk = 2 * (case % 7)  # an even window: its position is on the nearest SNP (an odd one's lies between two sites)
    anchor = wr.POS0 + wr.SPACING * (g[kk].near + off)
    shift = (-anchor) % bp if bp < 2 ** 30 else 0
    T = shifted(c.tables, shift)
    assert bp == 2 ** 30 or (int(T.pos[g[kk].near + off]) % bp == 0)
    runs = [(k, q.sweep + shift, 1, 1) for k, q in enumerate(g)]
    nb = 1 if bp == 2 ** 30 else (1024 if bp == 2 else 40)
    blk = [(bp, max(int(T.pos[g[kk].near + off]) // bp - nb // 2, 0) if bp < 2 ** 30 else 0, nb)] * len(runs)
    la, N, bad = grid(n_la), wr.N_TIE, []

    @device_guard
    def go():
        shim.upload(T, cs, cn)
        return shim.blocks(runs, [la] * len(runs), blk, CASE_ER, N, len(cs)), shim.surface(runs, [la] * len(runs), CASE_ER)
    (pts, obs, ocnt), (spts, _) = go()
    assert all(wr.same(float(q["null_logl"]), N) for q in pts) and [int(q["chr"]) for q in pts] == list(range(len(g)))
    assert same_geometry(pts, spts), "the points differ from the surface kernel's"
    assert int(pts[kk]["nearest_snp"]) == g[kk].near
    check_blocks(pts, obs, ocnt, runs, [la] * len(runs), blk, T, f"bp {bp} off {off}", bad)
    if 2 < bp < 2 ** 30 and n_la > 1:  # the anchored boundary is inside the blocks: both sides hold terms
        j = int(T.pos[g[kk].near + off]) // bp - blk[0][1]
        assert 0 < j < nb and ocnt[kk][0][j - 1, 0] > 0 and ocnt[kk][0][j, 0] > 0
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 2. unequal cuts, an empty walk
def sparse_tables():
    """300 sites every 1000 bp, cubic rows with random coefficients: a site's term depends on log(alpha d)."""
    rng = np.random.default_rng(321)
    n, nrow = 300, 24
    coef = rng.uniform(-1e-3, 1e-3, (nrow, wr.N_IV, 4))
    return wr.Tables((5000 + 1000 * np.arange(n)).astype(np.int32), rng.integers(0, nrow, n).astype(np.uint32), coef,
                     rng.uniform(-0.5, 0.5, nrow), wr.log_table())


@device_guard
def test_unequal_cuts_and_empty_walks(shim):
    """Alphas whose walks end in different blocks on either side; positions 500 bp from the nearest SNP, where
    every alpha above -2.2 has an empty walk: cnt 0 and bs +0.0 in every block."""
    T = sparse_tables()
    la = [wr.LOG_AD_MIN, -7.5, -6.9, -6.0, -5.0, -2.0, 3.5, wr.LOG_AD_MAX]
    at = [5000 + 1000 * 150 + 1, 5000 + 1000 * 150 + 500, 5000 + 1000 * 7 + 499, 5000 + 1000 * 150, 4000, 305_500]
    runs = [(0, x, 1, 1) for x in at]
    blk = [(7000, 5, 41)] * len(runs)
    N, bad = -321.25, []
    shim.upload(T)
    pts, obs, ocnt = shim.blocks(runs, [la] * len(runs), blk, 1000, N, 1)
    check_blocks(pts, obs, ocnt, runs, [la] * len(runs), blk, T, "sparse", bad)
    for k, a in enumerate(la):
        if a > -2.2:
            assert not ocnt[1][0][:, k].any() and (obs[1][0][:, k].view(np.uint64) == 0).all(), a
    assert ocnt[1][0][:, 0].sum() == 300
    ends = {(int(np.flatnonzero(ocnt[0][0][:, k])[0]), int(np.flatnonzero(ocnt[0][0][:, k])[-1])) for k in range(5)}
    assert len(ends) >= 4, f"the walks end in the same blocks: {ends}"
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 3. the clamp
@device_guard
def test_clamp_absorbs_both_sides(shim):
    """b0 and nb cover the middle third of the longest walk only: the first and the last block absorb the
    rest, no term is dropped."""
    c = wr.cases()["edge-nonneg"]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)]
    la, bad, blk = [-20.0, -6.5, -3.0], [], []
    for a, n in zip(cs, cn):  # (at CASE_ER a walk's window is its whole chromosome, the sites up to the next window's)
        lo, hi = int(c.tables.pos[a]), int(c.tables.pos[a + n - 1])
        third = max((hi - lo) // 3, 1)
        blk.append((100, (lo + third) // 100, max(third // 100, 1)))
    shim.upload(c.tables, cs, cn)
    pts, obs, ocnt = shim.blocks(runs, [la] * len(runs), blk, CASE_ER, wr.N_TIE, len(cs))
    check_blocks(pts, obs, ocnt, runs, [la] * len(runs), blk, c.tables, "clamp", bad)
    for k, n in enumerate(cn):
        assert int(ocnt[k][0][:, 0].sum()) == n
        if n > 600:
            assert ocnt[k][0][0, 0] > 100 and ocnt[k][0][-1, 0] > 100, k
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


def test_device_counters(shim):
    """One position per window of walk_ref's geometry with 5 alphas, the clamp test's blocks: the launch adds the
    walks' terms (the edge blocks absorb what lies beyond them), the sites of the points' windows (the null-sum
    elements) and 5 walks per position to the device counters."""
    c = wr.cases()["edge-nonneg"]
    T, N = c.tables, wr.N_TIE
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)]
    la, blk = grid(5), []
    terms = null = 0
    for k, q in enumerate(g):
        near, sweep, ws, we = cr.init_point(T.pos, cs[k], cn[k], q.sweep, CASE_ER)
        null += we - ws + 1
        for a in la:
            nl, nr = wr.walk_terms(T, wr.Point(near, sweep, ws, we, N), a)[1]
            terms += 0 if nl < 0 else 1 + nl + nr
        lo, hi = int(T.pos[cs[k]]), int(T.pos[cs[k] + cn[k] - 1])
        third = max((hi - lo) // 3, 1)
        blk.append((100, (lo + third) // 100, max(third // 100, 1)))

    @device_guard
    def go():
        shim.upload(T, cs, cn)
        c0 = shim.counters()
        shim.blocks(runs, [la] * len(runs), blk, CASE_ER, N, len(cs))
        return c0, shim.counters()
    c0, c1 = go()
    assert terms > 0 and tuple(b - a for a, b in zip(c0, c1)) == (terms, null, 5 * len(runs))


# ------------------------------------------------------------------ 4. exact terms
@device_guard
def test_exact_terms(shim):
    """Constant tables: a site's term is exactly c3[row].  Rows of +-1e300, NaN, +-inf and -0.0 beside ordinary
    ones: the fold from +0.0 (a block of -0.0 alone sums to +0.0) and the NaN propagation per block."""
    g, n = wr.geometry()
    cs, cn = case_chromosomes()
    c3 = np.array([0.5, -0.25, 1e300, -1e300, math.nan, math.inf, -math.inf, -0.0, 3.0 * 2.0 ** -60, -7.125])
    rng = np.random.default_rng(77)
    row = rng.choice([0, 1, 8, 9], size=n).astype(np.uint32)
    for k, q in enumerate(g):  # the specials near the nearest SNP of some windows, a window of -0.0 alone
        if k % 5 == 0:
            row[q.near:q.near + 7] = [2, 3, 3, 2, 7, 7, 0][:max(min(7, q.we - q.near + 1), 0)]
        if k % 5 == 1:
            row[max(q.near - 3, q.ws):q.near + 1] = [5, 7, 6, 4][-(q.near - max(q.near - 3, q.ws) + 1):]
        if k == 7:
            row[cs[k]:cs[k] + cn[k]] = 7
    T = wr.const_tables(c3, row)
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)]
    la, bad = [-20.0, -6.0, -1.0, 4.0], []
    blk = [(2, int(T.pos[q.near]) // 2 - 9, 20) for q in g]
    shim.upload(T, cs, cn)
    for N in (wr.N_TIE, math.nan, -math.inf):
        pts, obs, ocnt = shim.blocks(runs, [la] * len(runs), blk, CASE_ER, N, len(cs))
        check_blocks(pts, obs, ocnt, runs, [la] * len(runs), blk, T, f"N={N!r}", bad)
    assert (obs[7][0].view(np.uint64) == 0).all() and ocnt[7][0].sum() > 0       # -0.0 terms: +0.0 sums
    assert np.isnan(obs[6][0]).any() and np.isinf(obs[6][0]).any() and (np.abs(obs[0][0]) == 1e300).any()
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 5. against the surface
@device_guard
def test_against_the_surface(shim):
    """V + null_logl beside fsclg_surface's sm of the same runs: two summation orders of the same n terms
    differ by at most 2 n 2^-53 (|N| + sum |t_i|) (each order's error is below n u times the sum of the
    magnitudes, u = 2^-53, to first order; the factor 2 covers both and the second order)."""
    c = wr.cases()["big-quotient"]  # random rows of magnitude [0.5, 1.5)
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep - 1, 1, 3) for k, q in enumerate(g)]
    la, N, bad = grid(9), wr.N_TIE, []
    blk = [(128, int(c.tables.pos[q.ws]) // 128, (int(c.tables.pos[q.we]) - int(c.tables.pos[q.ws])) // 128 + 2) for q in g]
    shim.upload(c.tables, cs, cn)
    pts, obs, ocnt = shim.blocks(runs, [la] * len(runs), blk, CASE_ER, N, len(cs))
    spts, sm = shim.surface(runs, [la] * len(runs), CASE_ER)
    assert same_geometry(pts, spts)
    p = 0
    for i, r in enumerate(runs):
        for t in range(r[3]):
            v = br.fold(obs[i][t][None])[0]
            for k, a in enumerate(la):
                terms = wr.walk_terms(c.tables, point_of(pts[p]), float(a))[0]
                bound = 2.0 * len(terms) * 2.0 ** -53 * (abs(N) + float(np.abs(terms).sum()))
                got, want = float(v[k]) + N, float(sm[p][k])
                print(f"run {i} position {t} la[{k}]: |V + N - sm| = {abs(got - want):.3e}, bound {bound:.3e}, n = {len(terms)}")
                if not abs(got - want) <= bound:
                    bad.append(f"run {i} position {t} la[{k}]: V + N = {got!r}, surface {want!r}, bound {bound!r}")
            p += 1
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad)


# ------------------------------------------------------------------ helpers of the whole-library tests
def setup(snp):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    scan = fscl_amd.load_snp_input(snp)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp)
    fscl_amd.compute_snp_null_model(scan, fsp)
    return scan, tab


# ------------------------------------------------------------------ 6. a windowed chromosome
def test_windowed_chromosome(built, tmp):
    """eval_range below the chromosome's length: window_start and window_end clip the walk, the window null
    sums come from fsclg_slot_windows.  Chromosomes of 3 and 500 SNPs (whole-chromosome windows at eval_range
    300) and one of 2 000; runs that reach past both ends."""
    er = 300
    chrs = []
    for i, (k, length) in enumerate(((3, 150_000), (500, 500_000), (2000, 2_000_000))):
        chrs += synth.generate(n_chr=1, chr_len=length, snps_per_chr=k, n=16, seed=270 + i, chr_names=[f"t{i}"],
                               sweeps_per_chr=1 if k >= 500 else 0)
    snp = tmp / "win.snp"
    synth.write_snp_file(str(snp), chrs)
    scan, tab = setup(snp)
    s = scan.contents
    assert s.chr_limits[2].n_snps > 2 * er + 1
    runs = [(0, 0, 50_000, 4), (1, -20_000, 60_000, 10), (2, -30_000, 230_000, 10), (2, 1_000_000, 777, 3)]
    la = [grid(5, -20.0)] * len(runs)
    blk = [(20_000, 0, 9), (50_000, 2, 5), (100_000, 3, 12), (30_000, 30, 8)]
    total = sum(r[3] for r in runs)
    nc = sum(r[3] * q[2] for r, q in zip(runs, blk)) * 5
    pts, bs, cnt = fscl_amd.blocks_runs(scan, tab, runs, la, blk, er, pts=sentinel(total, RAW), bs=sentinel(nc, np.float64),
                                        cnt=sentinel(nc, np.uint32))
    no_sentinel(pts, bs, cnt, "windows")
    assert fscl_amd.blocks_last_ms() > 0.0
    spts, sm = fscl_amd.surface_runs(scan, tab, runs, la, er)
    assert same_geometry(pts, spts) and pts["null_logl"].tobytes() == spts["null_logl"].tobytes()
    assert (pts["n_snps"][-3:] == 2 * er + 1).all()
    obs, ocnt, o = [], [], 0
    for r, q in zip(runs, blk):
        m = r[3] * q[2] * 5
        obs.append(bs[o:o + m].reshape(r[3], q[2], 5))
        ocnt.append(cnt[o:o + m].reshape(r[3], q[2], 5))
        o += m
    bad = []
    check_blocks(pts, obs, ocnt, runs, la, blk, wr.OracleTables(snp).tables, "windows", bad)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 7. determinism
@device_guard
def test_same_bytes_on_every_batch_and_slot(shim):
    """Every batch and slot, other runs beside them, and one run against the same positions as several runs
    (other chunks) give the same bytes."""
    c = wr.cases()["ties-dense-odd"]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    N, la = wr.N_TIE, grid(9)
    A = [(k, q.sweep - 3, 2, 5) for k, q in enumerate(g)][3:9]
    bA = [(128, int(c.tables.pos[q.ws]) // 128 + 1, 7) for q in g][3:9]
    X, bX = [(0, g[0].sweep, 1, 3), (14, g[14].sweep - 40, 7, 19)], [(2, 2600, 3), (2 ** 30, 0, 1)]
    Y, bY = [(9, g[9].sweep, 1, 1), (2, g[2].sweep, 5, 0), (1, g[1].sweep - 9, 3, 17)], [(64, 90, 1024), (5, 0, 2), (130, 60, 30)]
    shim.upload(c.tables, cs, cn)
    other = grid(9, -19.0, 3.0)
    p0, s0, c0 = shim.blocks(A, [la] * len(A), bA, CASE_ER, N, len(cs), batch=0, slot=0)
    p1, s1, c1 = shim.blocks(A, [la] * len(A), bA, CASE_ER, N, len(cs), batch=3, slot=2)
    p2, s2, c2 = shim.blocks(X + A + Y, [other] * len(X) + [la] * len(A) + [other] * len(Y), bX + bA + bY, CASE_ER, N, len(cs),
                             batch=5, slot=1)
    nA, nX = sum(r[3] for r in A), sum(r[3] for r in X)
    assert p0.tobytes() == p1.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(s0 + c0, s1 + c1)), \
        "the bytes depend on the batch or slot"
    assert p0.tobytes() == p2[nX:nX + nA].tobytes() and \
        all(a.tobytes() == b.tobytes() for a, b in zip(s0 + c0, s2[len(X):len(X) + len(A)] + c2[len(X):len(X) + len(A)])), \
        "the bytes depend on the other requests of the call"
    # 17 positions as one run (nb 30: one position per chunk; nb 1: 16 per chunk) and as runs of 1, 5, 11
    for b in ((130, 60, 30), (2 ** 30, 0, 1)):
        r1 = [(1, g[1].sweep - 9, 3, 17)]
        r3 = [(1, g[1].sweep - 9, 3, 1), (1, g[1].sweep - 6, 3, 5), (1, g[1].sweep + 9, 3, 11)]
        q1, t1, d1 = shim.blocks(r1, [la], [b], CASE_ER, N, len(cs))
        q3, t3, d3 = shim.blocks(r3, [la] * 3, [b] * 3, CASE_ER, N, len(cs), batch=1)
        assert q1.tobytes() == q3.tobytes() and t1[0].tobytes() == b"".join(x.tobytes() for x in t3) and \
            d1[0].tobytes() == b"".join(x.tobytes() for x in d3), "the bytes depend on how the positions are chunked"
    bad = []
    check_blocks(p2, s2, c2, X + A + Y, [other] * len(X) + [la] * len(A) + [other] * len(Y), bX + bA + bY, c.tables, "mixed", bad)
    assert not bad, "\n".join(bad[:12])


# ------------------------------------------------------------------ 8. argument errors
def test_submit_argument_errors(shim):
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()

    @device_guard
    def go():
        shim.upload(wr.cases()["zero-exact"].tables, cs, cn)
        shim.set_null(wr.N_TIE, len(cs))
    go()
    ok, la, b = [(0, g[0].sweep, 1, 2)], grid(4), [(100, 3, 5)]
    for bad in ((0, 3, 5), (-1, 3, 5), (100, -1, 5), (100, 3, 0), (100, 3, 1025), (100, 3, -2)):
        assert shim.submit(ok, [la], [bad], CASE_ER) == E_ARG, bad                      # block_bp, b0, nb
    assert shim.submit(ok + ok, [la, la], b + [(100, 3, 1025)], CASE_ER) == E_ARG       # the second run's blocks
    assert shim.submit(ok, [la], [(2 ** 31 - 1, 2 ** 31 - 1, 1024)], CASE_ER) == 0      # (the bounds are formed in 64 bits)
    assert shim.L.fsclg_blocks_wait(shim.ctx, 0, sentinel(2, RAW).ctypes.data, sentinel(2 * 1024 * 4, np.float64).ctypes.data,
                                    sentinel(2 * 1024 * 4, np.uint32).ctypes.data) == 0
    assert shim.submit(ok, [[]], b, CASE_ER) == E_ARG                                   # n_la 0
    assert shim.submit(ok, [list(np.linspace(-20, 4, 65))], b, CASE_ER) == E_ARG        # n_la 65
    for lst in ([-20.5, 0.0], [0.0, 4.5], [0.0, math.nan], [1.0, 1.0], [2.0, 1.0], [-math.inf, 0.0]):
        assert shim.submit(ok, [lst], b, CASE_ER) == E_ARG, lst
    for run in ((0, 100, 0, 2), (0, 100, 1, -1), (-1, 100, 1, 1), (len(cs), 100, 1, 1), (0, 2 ** 31 - 10, 1, 1)):
        assert shim.submit([run], [la], b, CASE_ER) == E_ARG, run
    for batch, slot in ((-1, 0), (10, 0), (0, -1), (0, 8)):
        assert shim.submit(ok, [la], b, CASE_ER, batch, slot) == E_ARG, (batch, slot)
    assert shim.submit(ok, [la], b, -1) == E_ARG
    assert shim.submit([(0, g[0].sweep, 1, 300000)], [list(np.linspace(-20, 4, 64))], [(2, 0, 1024)], CASE_ER) == E_ARG  # too many cells
    out_p, out_s, out_c = sentinel(2, RAW), sentinel(2 * 5 * 4, np.float64), sentinel(2 * 5 * 4, np.uint32)
    args = (out_p.ctypes.data, out_s.ctypes.data, out_c.ctypes.data)
    assert shim.L.fsclg_blocks_wait(shim.ctx, 0, *args) == E_STATE                      # nothing submitted
    la_arr = np.array(la, dtype=np.float64)
    assert shim.L.fsclg_surface_submit(shim.ctx, 0, 0, (wr.RunT * 1)(wr.RunT(*ok[0])), 1, la_arr.ctypes.data, 4, CASE_ER) == 0
    assert shim.L.fsclg_blocks_wait(shim.ctx, 0, *args) == E_STATE                      # the batch holds surfaces
    assert shim.L.fsclg_surface_wait(shim.ctx, 0, sentinel(2, RAW).ctypes.data, sentinel(8, np.float64).ctypes.data) == 0
    assert shim.submit(ok, [la], b, CASE_ER) == 0
    assert shim.submit(ok, [la], b, CASE_ER) == E_STATE                                 # the batch is pending
    assert shim.L.fsclg_surface_wait(shim.ctx, 0, out_p.ctypes.data, out_s.ctypes.data) == E_STATE
    assert shim.L.fsclg_blocks_wait(shim.ctx, 0, None, None, None) == E_ARG             # (the batch stays submitted)
    assert untouched(out_p) and untouched(out_s) and untouched(out_c), "a refused call wrote"
    assert shim.L.fsclg_blocks_wait(shim.ctx, 0, *args) == 0
    no_sentinel(out_p, out_s, out_c, "after the argument errors")
    fresh = BlkShim()
    try:
        assert fresh.submit(ok, [la], b, CASE_ER) == E_STATE                            # no tables, no sites
    finally:
        fresh.close()


# ------------------------------------------------------------------ 9. golden data
def test_golden_g2(built):
    """g2.snp, the top 2 points, 2 positions either side, 5 alphas (and the fitted one), blocks of 20 000 bp:
    every bs is, bit for bit, the block fold of scan_sites' terms of the same walk; cnt their count; Python's
    jackknife_combine is blocks_ref's."""
    step, bp = 500, 20000
    scan, tab = setup(GOLD / "g2.snp")
    fscl_amd.scan_chromosome(scan, tab)
    pts = fscl_amd.points(scan)
    top = [int(i) for i in np.argsort(-pts["clr"], kind="stable")[:2]]
    req = [(int(pts["chr"][i]), int(pts["sweep_pos"][i]), 2 * step, step,
            fscl_amd.surface_alphas(wr.LOG_AD_MIN, wr.LOG_AD_MAX, 5, float(pts["lalpha"][i])), i) for i in top]
    bks = fscl_amd.scan_blocks(scan, tab, req, bp)
    assert len(bks) == 2 and fscl_amd.blocks_last_ms() > 0.0
    s = scan.contents
    pos_all = np.array([s.snps[i].pos for i in range(s.n_snps)], dtype=np.int64)
    bad = []
    for i, bk in enumerate(bks):
        h = bk.hdr
        n_pos, nb, n_la = bk.bs.shape
        assert n_pos == 5 and n_la in (5, 6) and int(h["block_bp"]) == bp and nb == int(h["nb"])
        # the blocks are those of the positions' windows: the clamp never bites
        assert int(h["b0"]) == int(pos_all[bk.pts["window_start"].min()]) // bp
        assert nb == int(pos_all[bk.pts["window_end"].max()]) // bp - int(h["b0"]) + 1
        sreq = [(int(h["chr"]), int(h["start_pos"]) + p * step, float(a)) for p in range(n_pos) for a in bk.la]
        hdr, terms = fscl_amd.scan_sites(scan, tab, sreq)
        for w, hd in enumerate(hdr):
            p, k = divmod(w, n_la)
            near, nl, ln = int(hd["pt"]["nearest_snp"]), int(hd["nl"]), int(hd["len"])
            t = terms[int(hd["off"]):int(hd["off"]) + ln]
            nr = ln - 1 - nl if ln else 0
            idx = np.concatenate([[near], near - np.arange(1, nl + 1), near + np.arange(1, nr + 1)]).astype(np.int64)[:ln]
            o = np.argsort(idx, kind="stable")
            t, idx = t[o], idx[o]
            j = pos_all[idx] // bp - int(h["b0"])
            assert ln == 0 or (0 <= j.min() and j.max() < nb), "the clamp bites"
            wbs, wcnt = br.fold_groups(t, j, nb)
            for b in np.flatnonzero(~(same_arrays(bk.bs[p, :, k], wbs) & (bk.cnt[p, :, k] == wcnt))):
                bad.append(f"peak {i} position {p} block {b} la[{k}]: ({float(bk.bs[p][b][k]).hex()}, {bk.cnt[p][b][k]}) != "
                           f"({float(wbs[b]).hex()}, {wcnt[b]})")
        blocks, summ = fscl_amd.jackknife_combine(bk.bs, bk.cnt, bk.sweep_pos, bk.la)
        bad += [f"peak {i}: {m}" for m in br.same_combine(blocks, summ, br.jackknife_combine(bk.bs, bk.cnt, bk.sweep_pos, bk.la))]
        assert int(summ["g"]) >= 2 and int(summ["ipos"]) >= 0
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


def test_two_devices_give_the_same_blocks(built, tmp):
    """The requests of test_golden_g2 on five scan points of g2, once on one device and once split over two:
    the same headers, points, sums, counts and file.  One request takes the 5-alpha grid alone (no g2 point's
    lalpha is a grid value), so of the 5-lists one device's share is empty; the four 6-lists go to both."""
    step, bp = 500, 20000
    scan, tab = setup(GOLD / "g2.snp")
    fscl_amd.scan_chromosome(scan, tab)
    pts = fscl_amd.points(scan)
    assert len(pts) >= 5
    las = [fscl_amd.surface_alphas(wr.LOG_AD_MIN, wr.LOG_AD_MAX, 5, float(pts["lalpha"][i])) for i in range(5)]
    las[2] = fscl_amd.surface_alphas(wr.LOG_AD_MIN, wr.LOG_AD_MAX, 5)
    assert [len(la) for la in las] == [6, 6, 5, 6, 6], "one 5-list between two pairs of 6-lists"
    req = [(int(pts["chr"][i]), int(pts["sweep_pos"][i]), 2 * step, step, las[i], i) for i in range(5)]

    def evaluate(path):
        bks = fscl_amd.scan_blocks(scan, tab, req, bp)
        fscl_amd.jackknife_output(path, scan, bks)
        return bks
    fscl_amd.set_devices([0, 0])
    try:
        two = evaluate(tmp / "two.txt")
        assert fscl_amd.get_lib().fscl_amd_n_devices() == 2
    finally:
        fscl_amd.set_device(0)
    one = evaluate(tmp / "one.txt")
    assert len(one) == len(two) == 5 and all(int(b.hdr["nb"]) > 1 for b in one), "several blocks per request"
    for a, b in zip(one, two):
        assert a.hdr.tobytes() == b.hdr.tobytes() and a.pts.tobytes() == b.pts.tobytes()
        assert a.bs.tobytes() == b.bs.tobytes() and a.cnt.tobytes() == b.cnt.tobytes()
    assert (tmp / "two.txt").read_bytes() == (tmp / "one.txt").read_bytes() and (tmp / "one.txt").stat().st_size > 0


# ------------------------------------------------------------------ 10. crafted influence
@device_guard
def test_crafted_influence(shim):
    """Constant tables, 40 sites every 2 bp, blocks of 10 sites.  At log alpha 2.0 a walk holds the sites within
    7 bp of the position (log 7 + 2 <= 4 < log 9 + 2).  Position A lies in block 1, whose sites have the term
    8.0, position B in block 3 (terms 0.5); each walk stays inside its block.  A carries the peak.  Deleting
    block 1 moves the argmax to B; deleting block 3 leaves it at A; blocks 0 and 2 hold no term.  So g = 2,
    theta = (B, A), and se_pos = sqrt(1/2 * 2 ((B - A) / 2)^2) = (B - A) / 2 = 20 bp, bias_pos the same."""
    n = 40
    row = np.zeros(n, dtype=np.uint32)
    row[10:20] = 1
    row[30:40] = 2
    T = wr.const_tables(np.array([0.25, 8.0, 0.5]), row)
    posA, posB = int(T.pos[14]), int(T.pos[34])
    la = [2.0]
    runs = [(0, posA, posB - posA, 2)]
    bp = 20
    b0 = int(T.pos[0]) // bp
    assert int(T.pos[0]) % bp == 0
    blk = [(bp, b0, 4)]
    shim.upload(T)
    pts, obs, ocnt = shim.blocks(runs, [la], blk, CASE_ER, -10.0, 1)
    bad = []
    check_blocks(pts, obs, ocnt, runs, [la], blk, T, "influence", bad)
    assert not bad, "\n".join(bad)
    bs, cnt = obs[0], ocnt[0]
    nA, nB = int(cnt[0, 1, 0]), int(cnt[1, 3, 0])
    assert nA == int(cnt[0].sum()) and nB == int(cnt[1].sum()) and nA == nB >= 1, "each walk lies within one block"
    assert float(bs[0, 1, 0]) == 8.0 * nA and float(bs[1, 3, 0]) == 0.5 * nB
    blocks, s = fscl_amd.jackknife_combine(bs, cnt, pts["sweep_pos"], la)
    assert not br.same_combine(blocks, s, br.jackknife_combine(bs, cnt, pts["sweep_pos"], la))
    assert int(s["ipos"]) == 0 and float(s["v"]) == 8.0 * nA and int(s["g"]) == 2
    assert [int(b["has_terms"]) for b in blocks] == [0, 1, 0, 1]
    assert int(blocks[1]["ipos"]) == 1 and float(blocks[1]["v"]) == 0.5 * nB      # without block 1: position B
    assert int(blocks[3]["ipos"]) == 0 and float(blocks[3]["v"]) == 8.0 * nA      # without block 3: position A stays
    # theta_b = posB, posA: mean (posA + posB) / 2, se^2 = 1/2 * 2 ((posB - posA) / 2)^2, se = (posB - posA) / 2
    assert float(s["se_pos"]) == (posB - posA) / 2.0 == 20.0
    assert float(s["bias_pos"]) == (posB - posA) / 2.0 and int(s["top_shift"]) == 1 and int(s["top_loss"]) == 1


# ------------------------------------------------------------------ 11. end to end
def test_cli_end_to_end(built, tmp):
    snp = GOLD / "g2.snp"
    base = [str(CLI), "-f", str(snp)]
    for tag, extra in (("s", []), ("p", ["--n-permute=5"])):
        r = subprocess.run(base + extra + ["-o", str(tmp / f"o0{tag}.txt")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        r = subprocess.run(base + extra + ["-o", str(tmp / f"o1{tag}.txt"), f"--jackknife-file={tmp / f'j{tag}.txt'}",
                                           "--jackknife-step=5000", "--jackknife-alphas=-12:0:7"],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "Jackknife: " in r.stdout + r.stderr
        assert (tmp / f"o0{tag}.txt").read_bytes() == (tmp / f"o1{tag}.txt").read_bytes(), "--jackknife-file changed the -o output"
    assert (tmp / "js.txt").read_bytes() == (tmp / "jp.txt").read_bytes()
    r = subprocess.run(base + ["--no-scan", f"--jackknife-file={tmp / 'x.txt'}"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--jackknife-file needs the scan" in r.stderr + r.stdout and not (tmp / "x.txt").exists()
    scan, tab = setup(snp)
    fscl_amd.scan_chromosome(scan, tab)
    bks = fscl_amd.scan_point_jackknife(scan, tab, top=3, halfwidth=100000, step=5000, alphas=(-12.0, 0.0, 7), block_bp=50000)
    assert 1 <= len(bks) <= 3
    fscl_amd.jackknife_output(tmp / "b.txt", scan, bks)
    assert (tmp / "js.txt").read_bytes() == (tmp / "b.txt").read_bytes()
    lines = [ln.split("\t") for ln in (tmp / "js.txt").read_text().splitlines()]
    summaries = [f for f in lines if f[2] == "summary"]
    assert len(summaries) == len(bks)
    pts = fscl_amd.points(scan)
    o = 0
    for bk, f in zip(bks, summaries):
        blocks, s = fscl_amd.jackknife_combine(bk.bs, bk.cnt, bk.sweep_pos, bk.la)
        g = int(s["g"])
        rows = lines[o:o + g]
        assert lines[o + g] is f and len(f) == 18 and all(len(r_) == 11 and r_[2] != "summary" for r_ in rows)
        o += g + 1
        assert int(f[1]) == int(pts["sweep_pos"][int(bk.hdr["point"])])
        assert f[3:6] == [str(bk.bs.shape[0]), str(bk.bs.shape[2]), str(g)] and 21 <= bk.bs.shape[0] <= 41
        assert f[6] == str(int(bk.sweep_pos[int(s["ipos"])])) and f[8] == "%1.2f" % (2.0 * float(s["v"]))
        assert f[9] == ("%1.1f" % float(s["se_pos"]) if g >= 2 else "NA") and f[16:] == [str(int(s["n_edge_pos"])), str(int(s["n_edge_la"]))]
        with_terms = [b for b in blocks if int(b["has_terms"])]
        for r_, b in zip(rows, with_terms):
            start = (int(bk.hdr["b0"]) + int(b["block"])) * 50000
            assert r_[2:5] == [str(start), str(start + 49999), str(int(b["n_terms"]))]
            assert r_[5] == str(int(bk.sweep_pos[int(b["ipos"])])) and r_[7] == "%1.2f" % (2.0 * float(b["v"]))
    assert o == len(lines)
