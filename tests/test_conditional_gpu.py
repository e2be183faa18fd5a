"""The conditional sweep scan (fsclg_cond_submit, fscl_amd_scan_conditional, --conditional-file) on the GPU.

Every value and every point is compared by bit pattern (NaN equal to NaN) with the NumPy restatement
tests/cond_ref.py, which tests/test_conditional_host.py pins without a GPU.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import subprocess
import sys

import numpy as np
import pytest

import cond_ref as cr
import fscl_amd
import walk_ref as wr
from fscl_amd import synth
from util import CLI, GOLD, ROOT

sys.path.insert(0, str(ROOT / "oracle"))
import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
RAW = fscl_amd._POINT_RAW
CASE_ER = 5000  # above every window of walk_ref's geometry: each chromosome is one whole-chromosome window
E_ARG, E_STATE = -1, -3
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def sentinel(n, dtype):
    a = np.zeros(max(n, 1), dtype=dtype)
    a.view(np.uint8)[:] = SENTINEL
    return a


def no_sentinel(pts, sm, what):
    w = pts.view(np.uint8).reshape(len(pts), -1).view(np.uint32)
    assert not (w == int.from_bytes(bytes([SENTINEL] * 4), "little")).any(), f"{what}: a point was left unwritten"
    assert not (sm.reshape(-1).view(np.uint64) == int.from_bytes(bytes([SENTINEL] * 8), "little")).any(), \
        f"{what}: a value was left unwritten"


def grid(n, lo=wr.LOG_AD_MIN, hi=wr.LOG_AD_MAX):
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


class CondShim(wr.Shim):
    def __init__(self):
        super().__init__()
        L, vp = self.L, C.c_void_p
        L.fsclg_cond_submit.restype = C.c_int
        L.fsclg_cond_submit.argtypes = [vp, C.c_int, C.c_int, C.POINTER(wr.RunT), C.c_int, vp, C.c_int, vp, C.c_int]
        L.fsclg_cond_wait.restype, L.fsclg_cond_wait.argtypes = C.c_int, [vp, C.c_int, vp, vp]
        L.fsclg_cond_last_ms.restype, L.fsclg_cond_last_ms.argtypes = C.c_double, [vp, C.c_int]
        L.fsclg_surface_submit.restype = C.c_int
        L.fsclg_surface_submit.argtypes = [vp, C.c_int, C.c_int, C.POINTER(wr.RunT), C.c_int, vp, C.c_int, C.c_int]
        L.fsclg_surface_wait.restype, L.fsclg_surface_wait.argtypes = C.c_int, [vp, C.c_int, vp, vp]
        L.fsclg_slot_set_rows.restype, L.fsclg_slot_set_rows.argtypes = C.c_int, [vp, C.c_int, vp, vp]

    def n_terms(self) -> int:
        st = wr.StatsT()
        self._ok(self.L.fsclg_get_stats(self.ctx, C.byref(st)), "fsclg_get_stats")
        return int(st.n_terms)

    def submit(self, runs, las, clip, er, batch=0, slot=0):
        run = (wr.RunT * max(len(runs), 1))(*[wr.RunT(*r) for r in runs])
        la = np.ascontiguousarray(las, dtype=np.float64).reshape(max(len(runs), 1), -1)
        cl = None if clip is None else np.ascontiguousarray(clip, dtype=np.int32).reshape(-1)
        return self.L.fsclg_cond_submit(self.ctx, batch, slot, run, len(runs), la.ctypes.data, la.shape[1],
                                        None if cl is None else cl.ctypes.data, er)

    def run(self, runs, las, clip, er, N, n_chr, batch=0, slot=0, surface=False):
        """(points, values [positions][n_la]) of the runs with one (lo, hi) per position, on the uploaded rows set
        into `slot` with the whole-chromosome null sums N; the outputs are prefilled with a sentinel."""
        nul = (C.c_double * n_chr)(*([N] * n_chr))
        self._ok(self.L.fsclg_slot_set_rows(self.ctx, slot, None, nul), "fsclg_slot_set_rows")
        total, k = sum(r[3] for r in runs), len(las[0])
        pts, sm = sentinel(total, RAW), sentinel(total * k, np.float64)
        if surface:
            run = (wr.RunT * max(len(runs), 1))(*[wr.RunT(*r) for r in runs])
            la = np.ascontiguousarray(las, dtype=np.float64).reshape(max(len(runs), 1), -1)
            self._ok(self.L.fsclg_surface_submit(self.ctx, batch, slot, run, len(runs), la.ctypes.data, k, er), "fsclg_surface_submit")
            self._ok(self.L.fsclg_surface_wait(self.ctx, batch, pts.ctypes.data, sm.ctypes.data), "fsclg_surface_wait")
        else:
            assert len(np.asarray(clip).reshape(-1)) == 2 * total
            self._ok(self.submit(runs, las, clip, er, batch, slot), "fsclg_cond_submit")
            self._ok(self.L.fsclg_cond_wait(self.ctx, batch, pts.ctypes.data, sm.ctypes.data), "fsclg_cond_wait")
        pts, sm = pts[:total], sm[:total * k].reshape(total, k)
        no_sentinel(pts, sm, "conditional")
        return pts, sm


@pytest.fixture(scope="module")
def shim(built):
    s = CondShim()
    yield s
    s.close()


def case_chromosomes():
    """The 15 windows of walk_ref.geometry() as 15 chromosomes (as the surface tests take them)."""
    g, n = wr.geometry()
    start = [q.ws for q in g]
    return start, [b - a for a, b in zip(start, start[1:] + [n])]


def clip_kinds(near, ws, we, lens):
    """The clips of one position: lens = the (left, right) part lengths of the walks of the list's alphas."""
    kinds = {
        "whole": (ws, we), "empty": (near + 1, near), "no-nearest-right": (near + 1, we), "no-nearest-left": (ws, near - 1),
        "nearest-alone": (near, near), "single-right": (min(near + 3, we), min(near + 3, we)),
        "single-left": (max(near - 70, ws), max(near - 70, ws)), "beyond": (ws - 1000, we + 1000), "int-range": (INT_MIN, INT_MAX),
        "inverted-far": (INT_MAX, INT_MIN), "left-of-window": (ws - 50, ws - 1), "right-of-window": (we + 1, we + 50),
    }
    for d in (63, 64, 65):
        kinds[f"lo-{d}"] = (near - d, we)
        kinds[f"hi+{d}"] = (ws, near + d)
        kinds[f"both-{d}"] = (near - d, near + d)
    live = [ln for ln in lens if ln[0] >= 0]
    if len(live) >= 2:  # cuts the longest walk (the smallest alpha's) alone: every site the second longest reaches stays
        kinds["smallest-alpha-only"] = (near - live[1][0], near + live[1][1])
    elif live:
        kinds["smallest-alpha-only"] = (near - max(live[0][0] - 1, 0), near + max(live[0][1] - 1, 0))
    return kinds


def expect_rows(T, pts_geom, N, la, clips, walks):
    """Per position: the row of clipped values, its point (lalpha, sm_logl, clr) and its number of terms."""
    out = []
    for (near, sweep, ws, we), (lo, hi), wk in zip(pts_geom, clips, walks):
        pt = wr.Point(near, sweep, ws, we, N)
        row, cnt = [], 0
        for a, w in zip(la, wk):
            v, n = cr.clipped_value(T, pt, a, lo, hi, walk=w)
            row.append(v)
            cnt += n
        bla, best = cr.row_maximum(row, la)
        with np.errstate(all="ignore"):
            clr = float(np.float64(2.0) * (np.float64(best) - np.float64(N)))
        out.append((row, (bla, best, clr), cnt))
    return out


def compare(pts, sm, want, geom, what, bad):
    for p, (q, (row, point, _), gm) in enumerate(zip(pts, want, geom)):
        got = (int(q["nearest_snp"]), int(q["sweep_pos"]), int(q["window_start"]), int(q["window_end"]))
        if got != tuple(gm):
            bad.append(f"{what} position {p}: geometry {got} != {tuple(gm)}")
        for k, v in enumerate(row):
            if not wr.same(float(sm[p][k]), v):
                bad.append(f"{what} position {p} alpha {k}: {float(sm[p][k]).hex()} != {float(v).hex()}")
        gp = (float(q["lalpha"]), float(q["sm_logl"]), float(q["clr"]))
        if not all(wr.same(x, y) for x, y in zip(gp, point)):
            bad.append(f"{what} position {p}: point {gp} != {point}")


# ------------------------------------------------------------------ 1. the shim: clips on the crafted geometry
TABLES = ["edge-nonneg", "ties-dense-odd", "edge-back"]  # random rows; tie-heavy; binade edges


@pytest.mark.parametrize("n_la", [1, 4, 5, 64])
@pytest.mark.parametrize("name", TABLES)
def test_clips(shim, name, n_la):
    """Every window of walk_ref's geometry (parts of 0 .. 4097 sites) at its own position, once per clip: the whole
    window (the surface's bytes), empty, without the nearest SNP on either side, single sites, the trip boundaries
    63 / 64 / 65 sites from the nearest SNP, beyond the window and the int range, and one that cuts the smallest
    alpha's walk alone."""
    c = wr.cases()[name]
    T, N = c.tables, float(c.points[0].null_logl)
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    la = grid(n_la)
    runs, clips, geom, walks, kind_of = [], [], [], [], []
    for k, q in enumerate(g):
        gm = cr.init_point(T.pos, cs[k], cn[k], q.sweep, CASE_ER)
        pt = wr.Point(gm[0], gm[1], gm[2], gm[3], N)
        wk = [wr.walk_terms(T, pt, a) for a in la]
        for kind, cl in clip_kinds(gm[0], gm[2], gm[3], [w[1] for w in wk]).items():
            runs.append((k, q.sweep, 1, 1)); clips.append(cl); geom.append(gm); walks.append(wk); kind_of.append(kind)
    want = expect_rows(T, geom, N, la, clips, walks)
    assert any(k == "smallest-alpha-only" and w[2] > 0 for k, w in zip(kind_of, want))

    @device_guard
    def go():
        shim.upload(T, cs, cn)
        t0 = shim.n_terms()
        pts, sm = shim.run(runs, [la] * len(runs), clips, CASE_ER, N, len(cs))
        t1 = shim.n_terms()
        whole = [i for i, k in enumerate(kind_of) if k == "whole"]
        sp, ss = shim.run([runs[i] for i in whole], [la] * len(whole), None, CASE_ER, N, len(cs), surface=True)
        return pts, sm, t1 - t0, whole, sp, ss
    pts, sm, terms, whole, sp, ss = go()
    bad = []
    compare(pts, sm, want, geom, f"{name} n_la {n_la}", bad)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])
    assert all(wr.same(float(q["null_logl"]), N) for q in pts)
    assert terms == sum(w[2] for w in want), "the device counter of terms"
    assert pts[whole].tobytes() == sp.tobytes() and sm[whole].tobytes() == ss.tobytes(), "whole-window clips differ from the surface"
    for i, k in enumerate(kind_of):
        if k in ("empty", "inverted-far", "left-of-window", "right-of-window"):
            assert all(wr.same(float(v), N) for v in sm[i]), (k, i)


def test_device_counters(shim):
    """One position per window of walk_ref's geometry with 5 alphas, clipped to 70 sites on either side of the nearest
    SNP: the launch adds the clipped walks' terms, the sites of the points' windows (the null-sum elements, which
    no clip cuts) and 5 walks per position to the device counters."""
    c = wr.cases()["edge-nonneg"]
    T, N = c.tables, wr.N_TIE
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)]
    la = grid(5)
    geom = [cr.init_point(T.pos, cs[k], cn[k], q.sweep, CASE_ER) for k, q in enumerate(g)]
    clips = [(gm[0] - 70, gm[0] + 70) for gm in geom]
    walks = [[wr.walk_terms(T, wr.Point(gm[0], gm[1], gm[2], gm[3], N), a) for a in la] for gm in geom]
    want = expect_rows(T, geom, N, la, clips, walks)
    terms, whole = sum(w[2] for w in want), sum(len(w[0]) for wk in walks for w in wk)
    null = sum(gm[3] - gm[2] + 1 for gm in geom)

    @device_guard
    def go():
        shim.upload(T, cs, cn)
        c0 = shim.counters()
        shim.run(runs, [la] * len(runs), clips, CASE_ER, N, len(cs))
        return c0, shim.counters()
    c0, c1 = go()
    assert 0 < terms < whole, "the clips cut no walk"
    assert tuple(b - a for a, b in zip(c0, c1)) == (terms, null, 5 * len(runs))


def test_nan_rows_stay_in_their_clips(shim):
    """walk_ref's table with a NaN row far from the nearest SNP: a clip that leaves the site out gives finite values."""
    c = wr.cases()["row-nan"]
    T, N = c.tables, float(c.points[0].null_logl)
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    la = grid(5)
    runs, clips, geom, walks = [], [], [], []
    for k, q in enumerate(g):
        gm = cr.init_point(T.pos, cs[k], cn[k], q.sweep, CASE_ER)
        pt = wr.Point(gm[0], gm[1], gm[2], gm[3], N)
        wk = [wr.walk_terms(T, pt, a) for a in la]
        for cl in ((gm[2], gm[3]), (gm[0] - 40, gm[0] + 40)):
            runs.append((k, q.sweep, 1, 1)); clips.append(cl); geom.append(gm); walks.append(wk)
    want = expect_rows(T, geom, N, la, clips, walks)

    @device_guard
    def go():
        shim.upload(T, cs, cn)
        return shim.run(runs, [la] * len(runs), clips, CASE_ER, N, len(cs))
    pts, sm = go()
    bad = []
    compare(pts, sm, want, geom, "row-nan", bad)
    assert not bad, "\n".join(bad[:12])
    assert np.isnan(sm[0::2]).any() and not np.isnan(sm[1::2]).any()


@device_guard
def test_same_bytes_on_every_batch_slot_and_chunking(shim):
    c = wr.cases()["ties-dense-odd"]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    N = wr.N_TIE
    A = [(k, q.sweep - 3, 2, 5) for k, q in enumerate(g)][3:9]
    rng = np.random.default_rng(3)
    clipA = []
    for k, _, _, n in A:
        for _ in range(n):
            lo = int(rng.integers(g[k].ws - 5, g[k].near + 70))
            clipA.append((lo, int(rng.integers(lo - 2, max(g[k].we + 5, lo + 3)))))  # (some empty, some past the window)
    split = [r2 for (k, x, st, n) in A for r2 in ((k, x, st, 2), (k, x + 2 * st, st, 3))]  # the same positions, other runs
    X = [(0, g[0].sweep, 1, 3), (14, g[14].sweep - 40, 7, 19)]
    la = grid(9)
    other = grid(9, -19.0, 3.0)
    shim.upload(c.tables, cs, cn)
    nA, nX = len(clipA), sum(r[3] for r in X)
    p0, s0 = shim.run(A, [la] * len(A), clipA, CASE_ER, N, len(cs), batch=0, slot=0)
    p1, s1 = shim.run(A, [la] * len(A), clipA, CASE_ER, N, len(cs), batch=3, slot=2)
    p2, s2 = shim.run(X + split, [other] * len(X) + [la] * len(split), [(0, 10 ** 6)] * nX + clipA, CASE_ER, N, len(cs), batch=5, slot=1)
    assert p0.tobytes() == p1.tobytes() and s0.tobytes() == s1.tobytes(), "the bytes depend on the batch or slot"
    assert p0.tobytes() == p2[nX:nX + nA].tobytes() and s0.tobytes() == s2[nX:nX + nA].tobytes(), \
        "the bytes depend on how the runs are split or on the other requests of the call"
    # and they are the reference's
    T, geom, walks = c.tables, [], []
    for k, x, st, n in A:
        for t in range(n):
            gm = cr.init_point(T.pos, cs[k], cn[k], x + t * st, CASE_ER)
            geom.append(gm)
            walks.append([wr.walk_terms(T, wr.Point(gm[0], gm[1], gm[2], gm[3], N), a) for a in la])
    bad = []
    compare(p0, s0, expect_rows(T, geom, N, la, clipA, walks), geom, "chunking", bad)
    assert not bad, "\n".join(bad[:12])


def test_submit_argument_errors(shim):
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()

    @device_guard
    def go():
        shim.upload(wr.cases()["zero-exact"].tables, cs, cn)
    go()
    ok, la = [(0, g[0].sweep, 1, 2)], grid(4)
    cl = [(0, 10), (0, 10)]
    assert shim.submit(ok, [la], None, CASE_ER) == E_ARG                       # a NULL clip with positions
    assert shim.submit([(0, g[0].sweep, 1, 0)], [la], None, CASE_ER) == 0      # (none: nothing to clip)
    assert shim.L.fsclg_cond_wait(shim.ctx, 0, None, None) == 0
    assert shim.submit(ok, [[]], cl, CASE_ER) == E_ARG
    assert shim.submit(ok, [[1.0, 1.0]], cl, CASE_ER) == E_ARG
    assert shim.submit(ok, [[0.0, 4.5]], cl, CASE_ER) == E_ARG
    assert shim.submit([(len(cs), 100, 1, 2)], [la], cl, CASE_ER) == E_ARG
    assert shim.submit(ok, [la], cl, CASE_ER, 10, 0) == E_ARG and shim.submit(ok, [la], cl, CASE_ER, 0, 8) == E_ARG
    out_p, out_s = sentinel(2, RAW), sentinel(2 * 4, np.float64)
    assert shim.L.fsclg_cond_wait(shim.ctx, 0, out_p.ctypes.data, out_s.ctypes.data) == E_STATE   # nothing submitted
    assert shim.submit(ok, [la], cl, CASE_ER) == 0
    assert shim.submit(ok, [la], cl, CASE_ER) == E_STATE                       # the batch is pending
    assert shim.L.fsclg_surface_wait(shim.ctx, 0, out_p.ctypes.data, out_s.ctypes.data) == E_STATE  # (not a surface)
    assert shim.L.fsclg_cond_wait(shim.ctx, 0, None, None) == E_ARG            # (the batch stays submitted)
    assert shim.L.fsclg_cond_wait(shim.ctx, 0, out_p.ctypes.data, out_s.ctypes.data) == 0
    no_sentinel(out_p, out_s, "after the argument errors")
    assert shim.L.fsclg_cond_last_ms(shim.ctx, 0) > 0.0


# ------------------------------------------------------------------ 2. the library
ER, STEP = 200, 6000


def setup(snp, **tab_opts):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    scan = fscl_amd.load_snp_input(snp)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp, *tab_opts.get("asc", ()))
    fscl_amd.compute_snp_null_model(scan, fsp)
    return scan, tab


def oracle_tables(snp, **opts):
    real = orc.OracleScan
    orc.OracleScan = lambda f: real(f, **opts)  # (wr.OracleTables sets the oracle up with default options)
    try:
        return wr.OracleTables(snp).tables
    finally:
        orc.OracleScan = real


class Lib:
    def __init__(self, tmp, asc=False):
        # ascertained data with a few sites of lower depth (missing genotypes): their corrected table rows are NaN
        kw = dict(asc_depth=20, asc_min_freq=2) if asc else {}
        chrs = synth.generate(n_chr=2, chr_len=600_000, snps_per_chr=1500, n=16 if not asc else 40, seed=91, sweeps_per_chr=1,
                              missing=0.006 if asc else 0.0, **kw)
        self.snp = tmp / "c.snp"
        synth.write_snp_file(str(self.snp), chrs)
        self.scan, self.tab = setup(self.snp, asc=(20, 2) if asc else ())
        self.T = oracle_tables(self.snp, **kw)
        s = self.scan.contents
        self.cs = [s.chr_limits[c].start_index for c in range(2)]
        self.cn = [s.chr_limits[c].n_snps for c in range(2)]
        self.start = [s.chr_limits[c].start_pos for c in range(2)]
        self.end = [s.chr_limits[c].bp_length for c in range(2)]
        self.pos = self.T.pos.astype(np.int64)

    def free_grid_pos(self, c, k):
        """A grid position start + k' * STEP with no site on it, k' >= k."""
        while self.start[c] + k * STEP in set(self.pos[self.cs[c]:self.cs[c] + self.cn[c]].tolist()):
            k += 1
        return int(self.start[c] + k * STEP)

    def reference(self, c, given, la, halfwidth=0):
        """[(nearest, sweep_pos, window_start, window_end, lo, hi, G)] per position of chromosome c's grid."""
        gv = [(q, a) for ch, q, a in given if ch == c]
        G = cr.given_terms(self.T, self.pos, self.cs[c], self.cn[c], gv, ER)
        out = []
        for x in range(self.start[c], self.end[c] + 1, STEP):
            if halfwidth > 0 and not any(abs(x - q) <= halfwidth for q, _ in gv):
                continue
            near, sp, ws, we = cr.init_point(self.pos, self.cs[c], self.cn[c], x, ER)
            lo, hi = cr.clip(self.pos, self.cs[c], self.cn[c], [q for q, _ in gv], sp)
            out.append((near, sp, ws, we, lo, hi, G))
        return out

    def check_block(self, b, given, la, bad, halfwidth=0):
        c = int(b.hdr["chr"])
        ref = self.reference(c, given, la, halfwidth)
        assert len(ref) == len(b.rows), (len(ref), len(b.rows))
        assert [(int(w["pos"]), float(w["alpha"])) for w in b.given] == [(q, a) for ch, q, a in given if ch == c]
        for i, (r, (near, sp, ws, we, lo, hi, G)) in enumerate(zip(b.rows, ref)):
            N = float(r["null_logl"])
            pt = wr.Point(near, sp, ws, we, N)
            row = [cr.clipped_value(self.T, pt, a, lo, hi)[0] for a in la]
            bla, best = cr.row_maximum(row, la)
            A, n = cr.base(G, self.cs[c], lo, hi, ws, we)
            want = (sp, bla, best, A, n, cr.cond_clr(best, N, A))
            got = (int(r["pos"]), float(r["lalpha"]), float(r["v"]), float(r["base"]), int(r["n_terms"]), float(r["cond_clr"]))
            if not all(x == y if isinstance(x, int) else wr.same(x, y) for x, y in zip(got, want)):
                bad.append(f"chr {c} position {i}: {got} != {want}")
            if not ((int(r["lo"]) > int(r["hi"]) and lo > hi) or (int(r["lo"]), int(r["hi"])) == (lo, hi)):
                bad.append(f"chr {c} position {i}: clip ({r['lo']}, {r['hi']}) != ({lo}, {hi})")


@pytest.fixture(scope="module")
def lib(built, tmp_path_factory):
    return Lib(tmp_path_factory.mktemp("condlib"))


LA = grid(7)


def test_one_given_sweep(lib):
    q = lib.free_grid_pos(0, 25)
    given = [(0, q, 1e-3)]
    blocks = fscl_amd.scan_conditional(lib.scan, lib.tab, given, 0, STEP, LA, eval_range=ER)
    assert len(blocks) == 1 and int(blocks[0].hdr["chr"]) == 0 and int(blocks[0].hdr["round"]) == 1
    assert fscl_amd.conditional_last_ms() > 0.0 and fscl_amd.conditional_last_terms() > 0
    b, bad = blocks[0], []
    lib.check_block(b, given, LA, bad)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])
    at = [i for i, r in enumerate(b.rows) if int(r["pos"]) == q]
    assert len(at) == 1 and int(b.rows[at[0]]["lo"]) > int(b.rows[at[0]]["hi"])
    assert wr.bits(float(b.rows[at[0]]["cond_clr"])) == wr.bits(0.0), "a candidate at the given position scores +0.0"
    # positions whose window lies inside their own sites and holds no term of the given sweep: the surface's CLR
    runs = [(0, lib.start[0], STEP, len(b.rows))]
    pts, _ = fscl_amd.surface_runs(lib.scan, lib.tab, runs, [LA], ER)
    far = [i for i, (r, p) in enumerate(zip(b.rows, pts)) if int(r["lo"]) <= int(p["window_start"]) and
           int(p["window_end"]) <= int(r["hi"]) and wr.bits(float(r["base"])) == wr.bits(0.0)]
    assert len(far) >= 10 and len(far) < len(b.rows)
    for i in far:
        assert wr.same(float(b.rows[i]["cond_clr"]), float(pts[i]["clr"])), i
    assert any(not wr.same(float(r["cond_clr"]), float(p["clr"])) for r, p in zip(b.rows, pts))


def test_two_given_sweeps_and_halfwidth(lib):
    q1, q2 = lib.free_grid_pos(0, 20), lib.free_grid_pos(0, 45)
    given = [(0, q2, 2e-3), (1, lib.free_grid_pos(1, 30), 5e-4), (0, q1, 1e-3)]
    blocks = fscl_amd.scan_conditional(lib.scan, lib.tab, given, 0, STEP, LA, eval_range=ER)
    assert [(int(b.hdr["chr"]), int(b.hdr["round"])) for b in blocks] == [(0, 1), (1, 1)]
    bad = []
    for b in blocks:
        lib.check_block(b, given, LA, bad)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])
    mid = [r for r in blocks[0].rows if q1 < int(r["pos"]) < q2]
    assert mid and all(int(r["lo"]) > lib.cs[0] and int(r["hi"]) < lib.cs[0] + lib.cn[0] - 1 for r in mid), "both cuts"
    hw = 5 * STEP
    near = fscl_amd.scan_conditional(lib.scan, lib.tab, given, hw, STEP, LA, eval_range=ER)
    bad = []
    for b in near:
        lib.check_block(b, given, LA, bad, halfwidth=hw)
    assert not bad, "\n".join(bad[:12])
    assert len(near[0].rows) == 22 and len(near[1].rows) == 11
    full = {int(r["pos"]): r.tobytes() for r in blocks[0].rows}
    assert all(full[int(r["pos"])] == r.tobytes() for r in near[0].rows)


def test_rounds(lib):
    q = lib.free_grid_pos(0, 25)
    given = [(0, q, 1e-3)]
    blocks = fscl_amd.scan_conditional(lib.scan, lib.tab, given, 0, STEP, LA, rounds=3, eval_range=ER)
    assert all(int(b.hdr["chr"]) == 0 for b in blocks) and [int(b.hdr["round"]) for b in blocks] == list(range(1, len(blocks) + 1))
    cur, bad = list(given), []
    for i, b in enumerate(blocks):
        lib.check_block(b, cur, LA, bad)
        clr = b.rows["cond_clr"]
        ok = np.flatnonzero(clr == clr)
        best = int(ok[np.argmax(clr[ok])]) if len(ok) else -1  # (argmax: the first on a tie)
        assert int(b.hdr["max_row"]) == best
        added = best >= 0 and float(clr[best]) > 0.0
        assert int(b.hdr["added"]) == int(added)
        if added:
            cur.append((0, int(b.rows[best]["pos"]), math.exp(float(b.rows[best]["lalpha"]))))
        assert (i == len(blocks) - 1) == (not added or i == 2), "the rounds stop when nothing is added, or after the third"
    assert not bad, "\n".join(bad[:12])
    assert len(blocks) >= 2, "the synthetic sweep's shoulder should add a second round"
    one = fscl_amd.scan_conditional(lib.scan, lib.tab, given, 0, STEP, LA, rounds=3, min_clr=1e9, eval_range=ER)
    assert len(one) == 1 and int(one[0].hdr["added"]) == 0 and one[0].rows.tobytes() == blocks[0].rows.tobytes()


def test_two_devices_give_the_same_blocks(built, tmp):
    """g2.snp, given its two highest scan points that lie well apart on its one chromosome, two rounds: each
    sweep's interval of 5001 positions is two runs (a piece holds 4096), so a round's four or more runs are
    split over the devices.  One device and two give the same blocks, rows, given sweeps, terms and file."""
    halfwidth, step = 25000, 10
    scan, tab = setup(GOLD / "g2.snp")
    fscl_amd.scan_chromosome(scan, tab)
    pts = fscl_amd.points(scan)
    order = [int(i) for i in np.argsort(-pts["clr"], kind="stable")]
    far = [i for i in order if abs(int(pts["sweep_pos"][i]) - int(pts["sweep_pos"][order[0]])) > 4 * halfwidth]
    given = [(int(pts["chr"][i]), int(pts["sweep_pos"][i]), math.exp(float(pts["lalpha"][i]))) for i in (order[0], far[0])]
    assert given[0][0] == given[1][0] == 0 and scan.contents.n_chromosomes == 1

    def evaluate(path):
        blocks = fscl_amd.scan_conditional(scan, tab, given, halfwidth, step, LA, rounds=2)
        fscl_amd.conditional_output(path, scan, blocks)
        return blocks, fscl_amd.conditional_last_terms()
    fscl_amd.set_devices([0, 0])
    try:
        two, terms2 = evaluate(tmp / "two.txt")
        assert fscl_amd.get_lib().fscl_amd_n_devices() == 2
    finally:
        fscl_amd.set_device(0)
    one, terms1 = evaluate(tmp / "one.txt")
    assert len(one) == len(two) and 1 <= len(one) <= 2 and [int(b.hdr["round"]) for b in one] == list(range(1, len(one) + 1))
    assert 2 * 4096 < 2 * (2 * halfwidth // step) <= len(one[0].rows) <= 2 * (2 * halfwidth // step + 1), \
        "two intervals of two runs each"
    for a, b in zip(one, two):
        assert a.hdr.tobytes() == b.hdr.tobytes() and a.rows.tobytes() == b.rows.tobytes() and a.given.tobytes() == b.given.tobytes()
    print(f"conditional terms: one device {terms1}, two devices {terms2}")
    assert terms1 == terms2 > 0
    assert (tmp / "two.txt").read_bytes() == (tmp / "one.txt").read_bytes() and (tmp / "one.txt").stat().st_size > 0


def test_refusals(lib, monkeypatch):
    ok = [(0, lib.free_grid_pos(0, 25), 1e-3)]
    for kw, what in ((dict(given=[(2, 100, 1e-3)]), "unknown chromosome"), (dict(given=[(0, 100, 0.0)]), "alpha"),
                     (dict(given=[(0, 100, math.exp(5.0))]), "alpha"), (dict(given=[(0, 100 + i, 1e-3) for i in range(65)]), "more than 64"),
                     (dict(step=0), "--conditional-step"), (dict(rounds=9), "--conditional-rounds")):
        with pytest.raises(ValueError, match=what):
            fscl_amd.scan_conditional(lib.scan, lib.tab, kw.get("given", ok), 0, kw.get("step", STEP), LA, kw.get("rounds", 1),
                                      eval_range=ER)
    monkeypatch.setenv("FSCL_AMD_COND_CAP", "2000")
    with pytest.raises(ValueError, match="FSCL_AMD_COND_CAP"):
        fscl_amd.scan_conditional(lib.scan, lib.tab, ok, 0, STEP, LA, eval_range=ER)
    monkeypatch.delenv("FSCL_AMD_COND_CAP")
    assert len(fscl_amd.scan_conditional(lib.scan, lib.tab, ok, 0, STEP, LA, eval_range=ER)) == 1


def test_ascertained_nan_rows(built, tmp_path):
    """Ascertained data (-d 20, minimum frequency 2) with a few sites of lower depth: the corrected tables hold NaN rows
    for them.  The given sweep's walk crosses three such sites, so G holds NaN; NaN stays with the positions whose
    owned sites inside the window hold such a site (through A) or whose every walk is NaN (through V), bit for bit."""
    lb = Lib(tmp_path, asc=True)
    T, c = lb.T, 0
    nan_row = np.isnan(T.coef).any(axis=(1, 2)) | np.isnan(T.nullrow)
    nan_site = nan_row[T.row.astype(np.int64)]
    assert 3 <= nan_site[:lb.cn[0]].sum() <= 12, "the case needs a few NaN sites on the first chromosome"
    k = (int(lb.pos[lb.cs[c] + 1000]) - lb.start[c]) // STEP
    q = lb.free_grid_pos(c, k)
    given = [(c, q, 1e-4)]  # (log(alpha d) <= 4 up to 546 kb: its walk spans its window)
    G = cr.given_terms(T, lb.pos, lb.cs[c], lb.cn[c], [(q, 1e-4)], ER)
    assert np.isnan(G).any() and not np.isnan(G).all(), "G must hold NaN terms, and not only NaN"
    blocks = fscl_amd.scan_conditional(lb.scan, lb.tab, given, 0, STEP, LA, eval_range=ER)
    bad = []
    lb.check_block(blocks[0], given, LA, bad)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])
    rows = blocks[0].rows
    n_nan = 0
    for r, (near, sp, ws, we, lo, hi, _) in zip(rows, lb.reference(c, given, LA)):
        a, b = max(lo, ws), min(hi, we)
        owns_nan = a <= b and bool(np.isnan(G[a - lb.cs[c]:b - lb.cs[c] + 1]).any())
        assert math.isnan(float(r["base"])) == owns_nan, int(r["pos"])
        assert math.isnan(float(r["cond_clr"])) == (owns_nan or math.isnan(float(r["v"]))), int(r["pos"])
        n_nan += math.isnan(float(r["cond_clr"]))
    assert 0 < n_nan < len(rows) // 2, "NaN neither absent nor spread over the chromosome"


def test_cli_end_to_end(lib, tmp):
    q = lib.free_grid_pos(0, 25)
    name = lib.scan.contents.chr_limits[0].name.decode()
    base, step = [str(CLI), "-f", str(lib.snp)], f"--conditional-step={STEP}"  # (the CLI's eval_range is the default)
    opt = [f"--conditional-file={tmp / 'c.txt'}", f"--given-sweep={name}:{q}:1e-3", "--conditional-alphas=-20:4:7", "--conditional-rounds=2",
           "--prepend-label=lab", step]
    outs = []
    for tag, extra in (("0", ["--prepend-label=lab"]), ("1", opt)):
        r = subprocess.run(base + ["-o", str(tmp / f"o{tag}.txt"), "--n-permute=3"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout + r.stderr)
    assert "Conditional scan: " in outs[1] and "Conditional scan: " not in outs[0]
    assert (tmp / "o0.txt").read_bytes() == (tmp / "o1.txt").read_bytes(), "--conditional-file changed the -o output or the permutations"
    blocks = fscl_amd.scan_conditional(lib.scan, lib.tab, [(0, q, 1e-3)], 0, STEP, grid(7), rounds=2)
    fscl_amd.conditional_output(tmp / "b.txt", lib.scan, blocks, "lab")
    assert (tmp / "c.txt").read_bytes() == (tmp / "b.txt").read_bytes()
    lines = (tmp / "c.txt").read_text().splitlines()
    assert len(lines) == sum(len(b.rows) + 1 for b in blocks) and all(ln.startswith(f"lab\t{name}\t") for ln in lines)
    assert sum(ln.split("\t")[3] == "summary" for ln in lines) == len(blocks)
    # --no-scan with an explicit sweep writes the same first round; without one it is refused (the CPU tests)
    r = subprocess.run(base + ["--no-scan", "-o", str(tmp / "o3.txt"), f"--conditional-file={tmp / 'n.txt'}", f"--given-sweep={name}:{q}:1e-3",
                               "--conditional-alphas=-20:4:7", "--prepend-label=lab", step], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp / "n.txt").read_text().splitlines() == lines[:len(blocks[0].rows) + 1]
    # the default given sweep: the scan point of greatest CLR
    r = subprocess.run(base + ["-o", str(tmp / "o2.txt"), f"--conditional-file={tmp / 'd.txt'}", "--conditional-halfwidth=30000", step],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and (tmp / "d.txt").stat().st_size > 0, r.stderr[-2000:]
