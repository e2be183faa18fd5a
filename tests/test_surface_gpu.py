"""The position-by-alpha likelihood surfaces (fsclg_surface_submit, --surface-file) on the GPU.

Every sm value is compared by bit pattern (NaN equal to NaN) with the plain sequential reference of
tests/walk_ref.py -- the null sum plus the walk's terms in walk order (walk_terms + seq_sum) -- on the
record's own point; the points' geometry with the compiled oracle's init_scan_result.
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
from util import CLI, GOLD, ROOT, read_dump, same_bits

sys.path.insert(0, str(ROOT / "oracle"))
import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

B = 4  # SURF_B, the kernel's alphas per wave item
SENTINEL = 0xA5
RAW = fscl_amd._POINT_RAW
CASE_ER = 5000  # above every window of walk_ref's geometry: each chromosome is one whole-chromosome window


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
    """n ascending log alphas from lo to hi (fscl_amd_surface_alphas' grid, also at 64 values)."""
    return [-3.0] if n == 1 else [hi if i == n - 1 else lo + i * ((hi - lo) / (n - 1)) for i in range(n)]


def check_cells(pts, sm, T, las, what, bad, stride=1):
    """Every position's row against the sequential reference on the record's own point, and the point's
    (lalpha, sm_logl, clr) against the row's first strict maximum from the (LOG_AD_MAX, -DBL_MAX) state."""
    for p in range(0, len(pts), stride):
        q = pts[p]
        la = las[p] if isinstance(las[0], (list, np.ndarray)) else las
        N = float(q["null_logl"])
        pt = wr.Point(int(q["nearest_snp"]), int(q["sweep_pos"]), int(q["window_start"]), int(q["window_end"]), N)
        best, bla = -wr.DBL_MAX, wr.LOG_AD_MAX
        for k, a in enumerate(la):
            want = wr.seq_sum(N, wr.walk_terms(T, pt, float(a))[0])[0]
            got = float(sm[p][k])
            if not wr.same(got, want):
                bad.append(f"{what} position {p} la[{k}]={a!r}: {got.hex()} != {want.hex()}")
            if got > best:
                best, bla = got, float(a)
        with np.errstate(all="ignore"):
            clr = float(np.float64(2.0) * (np.float64(best) - np.float64(N)))
        if not (wr.same(float(q["lalpha"]), bla) and wr.same(float(q["sm_logl"]), best) and wr.same(float(q["clr"]), clr)):
            bad.append(f"{what} position {p}: point ({q['lalpha']!r}, {q['sm_logl']!r}, {q['clr']!r}) != row maximum "
                       f"({bla!r}, {best!r}, {clr!r})")


def oracle_points(pos_all, cs, cn, k, at, er):
    """orc_init_scan_result at positions `at` of chromosome k of the concatenated sites (global indices,
    the chromosome's start index and count as the scan's chr_limits give them)."""
    L = orc.load()
    L.orc_init_scan_result.argtypes = [C.POINTER(orc.OrcPt), C.c_int, C.c_void_p, C.POINTER(wr.OrcChr), C.c_int, C.c_int,
                                       C.c_void_p]
    L.orc_init_scan_result.restype = None
    snps = (wr.OrcSnp * len(pos_all))()
    for s_, p in zip(snps, pos_all):
        s_.pos = int(p)
    lim = wr.OrcChr(k, b"c", cs[k], cn[k], int(pos_all[cs[k]]), int(pos_all[cs[k] + cn[k] - 1]))
    out = []
    for x in at:
        q = orc.OrcPt()
        L.orc_init_scan_result(C.byref(q), k, snps, C.byref(lim), er, int(x), None)
        out.append((q.nearest_snp, q.sweep_pos, q.window_start, q.window_end))
    return out


def check_geometry(pts, want, what, bad):
    for p, (q, w) in enumerate(zip(pts, want)):
        got = (int(q["nearest_snp"]), int(q["sweep_pos"]), int(q["window_start"]), int(q["window_end"]))
        if got != tuple(w) or int(q["n_snps"]) != w[3] - w[2] + 1:
            bad.append(f"{what} position {p}: geometry {got} != oracle {tuple(w)}")


# ------------------------------------------------------------------ the shim alone
class SurfShim(wr.Shim):
    def __init__(self):
        super().__init__()
        L, vp = self.L, C.c_void_p
        L.fsclg_surface_submit.restype = C.c_int
        L.fsclg_surface_submit.argtypes = [vp, C.c_int, C.c_int, C.POINTER(wr.RunT), C.c_int, vp, C.c_int, C.c_int]
        L.fsclg_surface_wait.restype, L.fsclg_surface_wait.argtypes = C.c_int, [vp, C.c_int, vp, vp]
        L.fsclg_surface_last_ms.restype, L.fsclg_surface_last_ms.argtypes = C.c_double, [vp, C.c_int]
        L.fsclg_slot_set_rows.restype, L.fsclg_slot_set_rows.argtypes = C.c_int, [vp, C.c_int, vp, vp]

    def submit(self, runs, las, er, batch=0, slot=0):
        run = (wr.RunT * max(len(runs), 1))(*[wr.RunT(*r) for r in runs])
        la = np.ascontiguousarray(las, dtype=np.float64).reshape(max(len(runs), 1), -1)
        return self.L.fsclg_surface_submit(self.ctx, batch, slot, run, len(runs), la.ctypes.data, la.shape[1], er)

    def surface(self, runs, las, er, N, n_chr, batch=0, slot=0):
        """(points, values [positions][n_la]) of the runs on the uploaded rows set into `slot` with the
        whole-chromosome null sums N; the outputs are prefilled with a sentinel."""
        nul = (C.c_double * n_chr)(*([N] * n_chr))
        self._ok(self.L.fsclg_slot_set_rows(self.ctx, slot, None, nul), "fsclg_slot_set_rows")
        total, k = sum(r[3] for r in runs), len(las[0])
        pts, sm = sentinel(total, RAW), sentinel(total * k, np.float64)
        self._ok(self.submit(runs, las, er, batch, slot), "fsclg_surface_submit")
        self._ok(self.L.fsclg_surface_wait(self.ctx, batch, pts.ctypes.data, sm.ctypes.data), "fsclg_surface_wait")
        pts, sm = pts[:total], sm[:total * k].reshape(total, k)
        no_sentinel(pts, sm, "surface")
        return pts, sm


@pytest.fixture(scope="module")
def shim(built):
    s = SurfShim()
    yield s
    s.close()


def case_chromosomes():
    """The 15 windows of walk_ref.geometry() as 15 chromosomes (as the curve tests take them)."""
    g, n = wr.geometry()
    start = [q.ws for q in g]
    return start, [b - a for a, b in zip(start, start[1:] + [n])]


def device_guard(fn):
    """A device error ends the session: nothing more runs on the GPU after it."""
    @functools.wraps(fn)
    def run(*a, **kw):
        try:
            return fn(*a, **kw)
        except RuntimeError as e:
            pytest.exit(f"{fn.__name__}: {e}", returncode=3)
    return run


# ------------------------------------------------------------------ 1. trip boundaries
@pytest.mark.parametrize("n_la", [1, B - 1, B, B + 1, 2 * B + 1, 64])
def test_trip_boundaries(shim, n_la):
    """walk_ref's crafted geometry (parts of 0 .. 4097 sites on either side), four positions per window --
    two on a SNP (de-collision), two between SNPs -- and lists of every length around the block size."""
    c = wr.cases()["edge-nonneg"]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep - 2, 1, 4) for k, q in enumerate(g)]
    la, N, bad = grid(n_la), wr.N_TIE, []

    @device_guard
    def go():
        shim.upload(c.tables, cs, cn)
        return shim.surface(runs, [la] * len(runs), CASE_ER, N, len(cs))
    pts, sm = go()
    assert any(int(q["sweep_pos"]) != r[1] + t for r in runs for t, q in zip(range(4), pts[4 * r[0]:4 * r[0] + 4])), \
        "no position was de-collided"
    for k, r in enumerate(runs):
        want = oracle_points(c.tables.pos, cs, cn, k, [r[1] + t for t in range(4)], CASE_ER)
        check_geometry(pts[4 * k:4 * k + 4], want, f"window {k}", bad)
    assert all(wr.same(float(q["null_logl"]), N) for q in pts)
    check_cells(pts, sm, c.tables, la, f"n_la {n_la}", bad)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 2. unequal cuts inside a block
def sparse_tables():
    """300 sites every 1000 bp, cubic rows with random coefficients: a site's term depends on log(alpha d)."""
    rng = np.random.default_rng(321)
    n, nrow = 300, 24
    coef = rng.uniform(-1e-3, 1e-3, (nrow, wr.N_IV, 4))
    return wr.Tables((5000 + 1000 * np.arange(n)).astype(np.int32), rng.integers(0, nrow, n).astype(np.uint32), coef,
                     rng.uniform(-0.5, 0.5, nrow), wr.log_table())


@device_guard
def test_unequal_cuts(shim):
    """One walk of a block spans the window (alpha exactly LOG_AD_MIN), the next is the nearest SNP alone or
    empty (alphas up to exactly LOG_AD_MAX); positions 500 bp from the nearest SNP have empty walks."""
    T = sparse_tables()
    lists = [[wr.LOG_AD_MIN, -2.0, 3.5, wr.LOG_AD_MAX], [wr.LOG_AD_MIN, 2.5, 3.0, 3.5, wr.LOG_AD_MAX]]
    at = [5000 + 1000 * 150 + 1, 5000 + 1000 * 150 + 500, 5000 + 1000 * 7 + 499, 5000 + 1000 * 150, 4000, 305_500]
    N, bad = -321.25, []
    shim.upload(T)
    for lst in lists:
        runs = [(0, x, 1, 1) for x in at]
        pts, sm = shim.surface(runs, [lst] * len(runs), 1000, N, 1)
        check_geometry(pts, [(p.nearest_snp, p.sweep_pos, p.window_start, p.window_end)
                             for p in wr.oracle_init_points(T.pos, at, 1000, N)], "sparse", bad)
        check_cells(pts, sm, T, lst, f"list {lst}", bad)
        # the position half way between two sites: every alpha above -2.2 has an empty walk, sm is the null sum
        for k, a in enumerate(lst):
            if a > -2.0:
                assert wr.same(float(sm[1][k]), N), (a, sm[1][k])
        assert not wr.same(float(sm[1][0]), N)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 3. exact sums
EXACT_LA = grid(2 * B + 1)


@pytest.mark.parametrize("name", list(wr.cases()))
def test_exact_sums(shim, name):
    """walk_ref.cases(): ties at half an ulp, partial sums leaving N's binade, N with no integer grid,
    +-inf and NaN rows, each point as a surface at a fixed list: whatever path a chunk's sum takes, every
    value is the sequential fold."""
    c = wr.cases()[name]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)]
    Ns = list({wr.bits(p.null_logl): p.null_logl for p in c.points}.values())
    bad = []

    @device_guard
    def go():
        shim.upload(c.tables, cs, cn)
        return [shim.surface(runs, [EXACT_LA] * len(runs), CASE_ER, N, len(cs)) for N in Ns]
    for N, (pts, sm) in zip(Ns, go()):
        assert all(wr.same(float(q["null_logl"]), N) for q in pts)
        check_cells(pts, sm, c.tables, EXACT_LA, f"N={N!r}", bad)
    assert not bad, f"{name}: {len(bad)} mismatches:\n" + "\n".join(bad[:12])


def test_exact_sums_n_list(shim):
    """Every null value of walk_ref.N_LIST (binade edges, zero, subnormal, infinities, NaN) on one table."""
    c = wr.cases()["big-quotient"]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)][::2]
    la, bad = grid(B + 1), []

    @device_guard
    def go():
        shim.upload(c.tables, cs, cn)
        return [shim.surface(runs, [la] * len(runs), CASE_ER, N, len(cs)) for N in wr.N_LIST]
    for N, (pts, sm) in zip(wr.N_LIST, go()):
        assert all(wr.same(float(q["null_logl"]), N) for q in pts)
        check_cells(pts, sm, c.tables, la, f"N={N!r}", bad)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 4. the device counters
def test_device_counters(shim):
    """One position per window of walk_ref's geometry with 5 alphas: the launch adds the walks' terms, the sites of
    the points' windows (the null-sum elements) and 5 walks per position to the device counters."""
    c = wr.cases()["edge-nonneg"]
    T, N = c.tables, wr.N_TIE
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)]
    la = grid(5)
    terms = null = 0
    for k, q in enumerate(g):
        near, sweep, ws, we = cr.init_point(T.pos, cs[k], cn[k], q.sweep, CASE_ER)
        null += we - ws + 1
        for a in la:
            nl, nr = wr.walk_terms(T, wr.Point(near, sweep, ws, we, N), a)[1]
            terms += 0 if nl < 0 else 1 + nl + nr

    @device_guard
    def go():
        shim.upload(T, cs, cn)
        c0 = shim.counters()
        shim.surface(runs, [la] * len(runs), CASE_ER, N, len(cs))
        return c0, shim.counters()
    c0, c1 = go()
    assert terms > 0 and tuple(b - a for a, b in zip(c0, c1)) == (terms, null, 5 * len(runs))


# ------------------------------------------------------------------ helpers of the whole-library tests
def setup(snp):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    scan = fscl_amd.load_snp_input(snp)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp)
    fscl_amd.compute_snp_null_model(scan, fsp)
    return scan, tab


class Oracle:
    """orc_init_scan_result per position on an SNP file: the geometry and the window null sum."""

    def __init__(self, snp, eval_range=81920):
        self.o = orc.OracleScan(snp)
        L = self.o.L
        L.orc_init_scan_result.argtypes = [C.POINTER(orc.OrcPt), C.c_int, C.c_void_p, C.POINTER(wr.OrcChr), C.c_int, C.c_int,
                                           C.POINTER(orc.OrcStats)]
        L.orc_init_scan_result.restype = None
        self.er = eval_range

    def points(self, chr_pos):
        L, s, st = self.o.L, self.o.s.contents, self.o.stats
        lim = C.cast(s.chr, C.POINTER(wr.OrcChr))
        out = []
        for ch, pos in chr_pos:
            pt = orc.OrcPt()
            L.orc_init_scan_result(C.byref(pt), int(ch), s.snps, C.byref(lim[int(ch)]), self.er, int(pos), C.byref(st))
            out.append((pt.nearest_snp, pt.sweep_pos, pt.window_start, pt.window_end, pt.null_logl))
        return out


def check_points_oracle(pts, want, what, bad):
    check_geometry(pts, [w[:4] for w in want], what, bad)
    for p, (q, w) in enumerate(zip(pts, want)):
        if not same_bits(float(q["null_logl"]), w[4]):
            bad.append(f"{what} position {p}: null_logl {float(q['null_logl']).hex()} != oracle {w[4].hex()}")


# ------------------------------------------------------------------ 4. window null sums
def test_window_null_sums(built, tmp):
    """Chromosomes of 1, 3 and 500 SNPs (whole-chromosome windows at eval_range 300) and one of 2 000
    (window null sums); runs that reach past both ends of their chromosome."""
    er = 300
    chrs = []
    for i, (k, length) in enumerate(((1, 50_000), (3, 150_000), (500, 500_000), (2000, 2_000_000))):
        chrs += synth.generate(n_chr=1, chr_len=length, snps_per_chr=k, n=16, seed=270 + i, chr_names=[f"t{i}"],
                               sweeps_per_chr=1 if k >= 500 else 0)
    snp = tmp / "win.snp"
    synth.write_snp_file(str(snp), chrs)
    scan, tab = setup(snp)
    s = scan.contents
    assert [s.chr_limits[c].n_snps for c in range(3)] == [1, 3, 500] and s.chr_limits[3].n_snps > 2 * er + 1
    p1 = s.snps[s.chr_limits[0].start_index].pos
    runs = [(0, max(p1 - 2000, 0), 1000, 5), (0, p1, 1, 1), (1, 0, 50_000, 4), (2, -20_000, 60_000, 10),
            (3, -30_000, 230_000, 10), (3, 1_000_000, 777, 3)]
    la = [grid(B + 1)] * len(runs)
    total = sum(r[3] for r in runs)
    pts, sm = fscl_amd.surface_runs(scan, tab, runs, la, er, pts=sentinel(total, RAW), sm=sentinel(total * (B + 1), np.float64))
    no_sentinel(pts, sm, "windows")
    chr_pos = [(c, a + t * st) for c, a, st, n in runs for t in range(n)]
    bad = []
    check_points_oracle(pts, Oracle(snp, er).points(chr_pos), "windows", bad)
    assert (pts["chr"] == [c for c, _ in chr_pos]).all()
    check_cells(pts, sm, wr.OracleTables(snp).tables, la[0], "windows", bad)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 5. golden data
# the fixtures of a scan with default options (g2 has no *_scan.dump: its default-option dump is the
# 30-permutation one, whose points are the scan's)
GOLDEN_DUMP = {"g1": "g1_scan.dump", "g2": "g2_p30.dump"}


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_golden(built, name):
    """A surface centred on every scan point of the golden dump, the point's own lalpha inserted into a
    5-alpha grid, half-width two steps: the centre cell at that alpha is the dump's sm_logl, the centre
    point the dump's point, every other cell the sequential reference."""
    step = 500
    dump = read_dump(GOLD / GOLDEN_DUMP[name])
    scan, tab = setup(GOLD / f"{name}.snp")
    req = [(r[0], r[1], 2 * step, step, fscl_amd.surface_alphas(wr.LOG_AD_MIN, wr.LOG_AD_MAX, 5, r[3])) for r in dump]
    sfs = fscl_amd.scan_surface(scan, tab, req)
    assert len(sfs) == len(dump)
    T = wr.OracleTables(GOLD / f"{name}.snp").tables
    bad = []
    for i, (sf, r) in enumerate(zip(sfs, dump)):
        h = sf.hdr
        assert int(h["n_pos"]) == len(sf.pts) and sf.sm.shape == (len(sf.pts), len(sf.la))
        ks = [k for k, a in enumerate(sf.la) if same_bits(float(a), r[3])]
        assert len(ks) == 1 and len(sf.la) in (5, 6), f"point {i}: lalpha {r[3]!r} not once in {sf.la}"
        assert (r[1] - int(h["start_pos"])) % step == 0
        pc = (r[1] - int(h["start_pos"])) // step
        if not same_bits(float(sf.sm[pc][ks[0]]), r[4]):
            bad.append(f"point {i}: centre cell {float(sf.sm[pc][ks[0]]).hex()} != dump sm_logl {r[4].hex()}")
        q = sf.pts[pc]
        got = (int(q["chr"]), int(q["sweep_pos"]), float(q["clr"]), float(q["lalpha"]), float(q["sm_logl"]),
               float(q["null_logl"]), int(q["nearest_snp"]), int(q["window_start"]), int(q["window_end"]))
        for f, x, y in zip(("chr", "sweep_pos", "clr", "lalpha", "sm_logl", "null_logl", "nearest_snp", "window_start",
                            "window_end"), got, r[:9]):
            if not (same_bits(x, y) if isinstance(x, float) else x == y):
                bad.append(f"point {i}: centre point {f}: {x!r} != dump {y!r}")
        check_cells(sf.pts, sf.sm, T, [float(a) for a in sf.la], f"point {i}", bad)
    assert not bad, f"{name}: {len(bad)} mismatches:\n" + "\n".join(bad[:12])


def test_two_devices_give_the_same_surfaces(built, tmp):
    """The requests of test_golden on five scan points of g2, once on one device and once split over two:
    the same headers, points, values, terms and file.  Every g2 point's lalpha lies off the 5-alpha grid
    (its list has 6 values), so one request takes the grid alone, the list of a point whose lalpha is a
    grid value: of the 5-lists one device's share is empty, the 6-lists go to both devices and come back
    into request order around it."""
    step = 500
    scan, tab = setup(GOLD / "g2.snp")
    fscl_amd.scan_chromosome(scan, tab)
    pts = fscl_amd.points(scan)
    assert len(pts) >= 5
    las = [fscl_amd.surface_alphas(wr.LOG_AD_MIN, wr.LOG_AD_MAX, 5, float(pts["lalpha"][i])) for i in range(5)]
    las[2] = fscl_amd.surface_alphas(wr.LOG_AD_MIN, wr.LOG_AD_MAX, 5)
    assert [len(la) for la in las] == [6, 6, 5, 6, 6], "one 5-list between two pairs of 6-lists"
    req = [(int(pts["chr"][i]), int(pts["sweep_pos"][i]), 2 * step, step, las[i], i) for i in range(5)]

    def evaluate(path):
        sfs = fscl_amd.scan_surface(scan, tab, req)
        fscl_amd.surface_output(path, scan, sfs, 2.0)
        return sfs, fscl_amd.surface_last_terms()
    fscl_amd.set_devices([0, 0])
    try:
        two, terms2 = evaluate(tmp / "two.txt")
        assert fscl_amd.get_lib().fscl_amd_n_devices() == 2
    finally:
        fscl_amd.set_device(0)
    one, terms1 = evaluate(tmp / "one.txt")
    assert len(one) == len(two) == 5
    for a, b in zip(one, two):
        assert a.hdr.tobytes() == b.hdr.tobytes() and a.pts.tobytes() == b.pts.tobytes() and a.sm.tobytes() == b.sm.tobytes()
    print(f"surface terms: one device {terms1}, two devices {terms2}")
    assert terms1 == terms2 > 0
    assert (tmp / "two.txt").read_bytes() == (tmp / "one.txt").read_bytes() and (tmp / "one.txt").stat().st_size > 0


# ------------------------------------------------------------------ 6. determinism
@device_guard
def test_same_bytes_on_every_batch_and_slot(shim):
    c = wr.cases()["ties-dense-odd"]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    N = wr.N_TIE
    A = [(k, q.sweep - 3, 2, 5) for k, q in enumerate(g)][3:9]
    X = [(0, g[0].sweep, 1, 3), (14, g[14].sweep - 40, 7, 19)]
    Y = [(9, g[9].sweep, 1, 1), (2, g[2].sweep, 5, 0), (1, g[1].sweep - 9, 3, 17)]
    la = grid(2 * B + 1)
    shim.upload(c.tables, cs, cn)
    nA, nX = sum(r[3] for r in A), sum(r[3] for r in X)
    p0, s0 = shim.surface(A, [la] * len(A), CASE_ER, N, len(cs), batch=0, slot=0)
    p1, s1 = shim.surface(A, [la] * len(A), CASE_ER, N, len(cs), batch=3, slot=2)
    other = grid(2 * B + 1, -19.0, 3.0)
    p2, s2 = shim.surface(X + A + Y, [other] * len(X) + [la] * len(A) + [other] * len(Y), CASE_ER, N, len(cs), batch=5, slot=1)
    assert p0.tobytes() == p1.tobytes() and s0.tobytes() == s1.tobytes(), "the bytes depend on the batch or slot"
    assert p0.tobytes() == p2[nX:nX + nA].tobytes() and s0.tobytes() == s2[nX:nX + nA].tobytes(), \
        "the bytes depend on the other requests of the call"
    bad = []
    check_cells(p2, s2, c.tables, [other] * nX + [la] * nA + [other] * (len(p2) - nX - nA), "mixed", bad, stride=3)
    assert not bad, "\n".join(bad[:12])


# ------------------------------------------------------------------ 7. end to end
def parse_surface_file(path):
    """[(chr name, centre, [(pos, alpha text, stat text, mark)], summary fields)] per surface."""
    out = []
    for line in path.read_text().splitlines():
        f = line.split("\t")
        if f[2] == "summary":
            out[-1][3].extend(f[3:])
            continue
        if not out or out[-1][3]:
            out.append((f[0], int(f[1]), [], []))
        out[-1][2].append((int(f[2]), f[3], f[4], f[5]))
    return out


def test_cli_end_to_end(built, tmp):
    snp = GOLD / "g2.snp"
    base = [str(CLI), "-f", str(snp), "--n-permute=5"]
    r = subprocess.run(base + ["-o", str(tmp / "o0.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(base + ["-o", str(tmp / "o1.txt"), f"--surface-file={tmp / 's.txt'}", f"--alpha-file={tmp / 'a.txt'}"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Surfaces: " in r.stdout + r.stderr
    assert (tmp / "o0.txt").read_bytes() == (tmp / "o1.txt").read_bytes(), "--surface-file changed the -o output"
    assert (tmp / "a.txt").stat().st_size > 0
    scan, tab = setup(snp)
    fscl_amd.scan_chromosome(scan, tab)
    sfs = fscl_amd.scan_point_surfaces(scan, tab, top=3)
    assert 1 <= len(sfs) <= 3 and fscl_amd.surface_last_ms() > 0.0 and fscl_amd.surface_last_terms() > 0
    fscl_amd.surface_output(tmp / "b.txt", scan, sfs, 2.0)
    assert (tmp / "s.txt").read_bytes() == (tmp / "b.txt").read_bytes()
    rows = parse_surface_file(tmp / "s.txt")
    assert len(rows) == len(sfs)
    pts = fscl_amd.points(scan)
    for (name, centre, cells, summ), sf in zip(rows, sfs):
        reg, mark = fscl_amd.surface_region(sf, 2.0)
        n_pos, n_la = sf.sm.shape
        assert centre == int(pts["sweep_pos"][int(sf.hdr["point"])]) and len(cells) == n_pos * n_la and len(summ) == 14
        assert any(same_bits(float(a), float(pts["lalpha"][int(sf.hdr["point"])])) for a in sf.la)
        assert [m for *_, m in cells] == [{2: "*", 1: "+", 0: "-"}[int(v)] for v in mark.reshape(-1)]
        pos = [int(v) for v in sf.pts["sweep_pos"]]
        want = [str(n_pos), str(n_la), str(pos[reg["max_ipos"]]), "%1.3e" % math.exp(sf.la[reg["max_ila"]]),
                "%1.2f" % (2.0 * float(reg["max_v"])), str(pos[reg["ipos_lo"]]), str(pos[reg["ipos_hi"]]),
                str(int(reg["open_pos_lo"])), str(int(reg["open_pos_hi"])), "%1.3e" % math.exp(sf.la[reg["ila_lo"]]),
                "%1.3e" % math.exp(sf.la[reg["ila_hi"]]), str(int(reg["open_la_lo"])), str(int(reg["open_la_hi"])),
                str(int(reg["n_region"]))]
        assert summ == want


def test_cli_six_files_at_once_equal_each_alone(built, tmp):
    """One invocation writing the alpha, sites, surface, jackknife, conditional and expect files together, the
    surface's step, half-width and alpha grid given and the others' left to follow them, against six invocations
    that each write one file with the inherited values spelled out: the same bytes, file by file."""
    g, step, hw, grid_s = 2000, 5000, 20000, "-12:0:5"
    base = [str(CLI), "-f", str(GOLD / "g1.snp"), "-g", str(g), "-G", "100000"]
    alone = {"alpha": [], "sites": [],
             "surface": [f"--surface-step={step}", f"--surface-halfwidth={hw}", f"--surface-alphas={grid_s}"],
             "jackknife": [f"--jackknife-step={step}", f"--jackknife-halfwidth={hw}", f"--jackknife-alphas={grid_s}"],
             "conditional": [f"--conditional-step={g}", f"--conditional-alphas={grid_s}"],
             "expect": [f"--expect-alphas={grid_s}"]}
    runs = [("all", [f"--{k}-file={tmp / f'all_{k}.txt'}" for k in alone] + alone["surface"])]
    runs += [(k, [f"--{k}-file={tmp / f'one_{k}.txt'}"] + extra) for k, extra in alone.items()]
    for tag, extra in runs:
        r = subprocess.run(base + ["-o", str(tmp / f"o_{tag}.txt")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
    for k in alone:
        got, want = (tmp / f"all_{k}.txt").read_bytes(), (tmp / f"one_{k}.txt").read_bytes()
        assert len(want) > 0 and got == want, f"--{k}-file: written with the other five it differs from the file written alone"
        assert (tmp / f"o_{k}.txt").read_bytes() == (tmp / "o_all.txt").read_bytes()


# ------------------------------------------------------------------ 8. argument errors
def test_submit_argument_errors(shim):
    E_ARG, E_STATE = -1, -3
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()

    @device_guard
    def go():
        shim.upload(wr.cases()["zero-exact"].tables, cs, cn)
    go()
    ok = [(0, g[0].sweep, 1, 2)]
    la = grid(B)
    assert shim.submit(ok, [[]], CASE_ER) == E_ARG                                  # n_la 0
    assert shim.submit(ok, [list(np.linspace(-20, 4, 65))], CASE_ER) == E_ARG       # n_la 65
    for lst in ([-20.5, 0.0], [0.0, 4.5], [0.0, math.nan], [math.nan, 1.0], [1.0, 1.0], [2.0, 1.0], [-math.inf, 0.0]):
        assert shim.submit(ok, [lst], CASE_ER) == E_ARG, lst
    assert shim.submit(ok + ok, [la, la[:-1] + [la[-2]]], CASE_ER) == E_ARG         # the second run's list
    for run in ((0, 100, 0, 2), (0, 100, 1, -1), (-1, 100, 1, 1), (len(cs), 100, 1, 1), (0, 2**31 - 10, 1, 1),
                (0, 2**30, 2**20, 2000)):
        assert shim.submit([run], [la], CASE_ER) == E_ARG, run
    for batch, slot in ((-1, 0), (10, 0), (0, -1), (0, 8)):
        assert shim.submit(ok, [la], CASE_ER, batch, slot) == E_ARG, (batch, slot)
    assert shim.submit(ok, [la], -1) == E_ARG
    out_p, out_s = sentinel(2, RAW), sentinel(2 * B, np.float64)
    assert shim.L.fsclg_surface_wait(shim.ctx, 0, out_p.ctypes.data, out_s.ctypes.data) == E_STATE   # nothing submitted
    assert shim.submit(ok, [la], CASE_ER) == 0
    assert shim.submit(ok, [la], CASE_ER) == E_STATE                                # the batch is pending
    assert shim.L.fsclg_surface_wait(shim.ctx, 0, None, None) == E_ARG              # (the batch stays submitted)
    assert shim.L.fsclg_surface_wait(shim.ctx, 0, out_p.ctypes.data, out_s.ctypes.data) == 0
    no_sentinel(out_p, out_s, "after the argument errors")
    fresh = SurfShim()
    try:
        assert fresh.submit(ok, [la], CASE_ER) == E_STATE                           # no tables, no sites
    finally:
        fresh.close()
