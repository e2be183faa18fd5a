"""search_maxalpha over raw arrays, restated in NumPy, with the vectors that pin the kernels' exact-sum
fallbacks and a ctypes view of the device shim (include/fsclg.h).

The restatement (sm-search.c:269-300 over the shim's inputs): a walk takes the nearest SNP, then the
sites to its left until log(alpha d) > 4 or the window start, then the sites to its right until
log(alpha d) > 4 or the window end; a site's term is the cubic of its row's interval minus the row's
null value; the sum is strictly sequential from the point's null_logl; the coarse alphas, then the
refine alphas around the coarse winner, each compared with a strict '>' from (-DBL_MAX, 4.0).

The diagnostics say which regime of the integer-ulp scheme a point is in (ties, partial sums leaving
N's binade, quotients past 2^51, equal candidates): the tests use them as preconditions, so that a
vector named for a regime is in it.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import struct
from dataclasses import dataclass, field

import numpy as np

import fscl_amd
from fscl_amd import PointT, RunT

DBL_MAX = 1.7976931348623157e308
LOG_AD_MIN, LOG_AD_MAX = -20.0, 4.0
N_IV = 200
STEP = 24.0 / 201.0
MAXTIES, XTIES = 512, 64  # the kernels' tie table per phase and tie slots per split member


# ------------------------------------------------------------------ the reference
@dataclass
class Tables:
    pos: np.ndarray       # int32 [n_snps], sorted
    row: np.ndarray       # uint32 [n_snps]
    coef: np.ndarray      # float64 [n_rows][n_iv][4]
    nullrow: np.ndarray   # float64 [n_rows]
    log_table: np.ndarray  # float64 [65536]
    step: float = STEP


@dataclass
class Point:
    nearest_snp: int
    sweep_pos: int
    window_start: int
    window_end: int
    null_logl: float


@dataclass
class Diag:
    """Per phase (0 coarse, 1 refine): one entry per walk, in candidate order."""
    ties: list = field(default_factory=lambda: [[], []])      # ties of each walk
    leaves: list = field(default_factory=lambda: [[], []])    # a partial sum leaves N's binade or is >= 0
    max_r: list = field(default_factory=lambda: [[], []])     # max |rint(t / u)| of each walk (inf: no grid)
    sums: list = field(default_factory=lambda: [[], []])      # the walks' sums
    lens: list = field(default_factory=lambda: [[], []])      # (left part, right part) lengths, -1 -1 if empty

    def phase_ties(self, ph):
        return int(sum(self.ties[ph]))

    def equal_sums(self, ph):
        b = [bits(s) for s in self.sums[ph] if s == s]
        return len(set(b)) < len(b)


def bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def same(a: float, b: float) -> bool:
    """Equal by bit pattern; two NaNs equal whatever their sign or payload."""
    return bits(a) == bits(b) or (a != a and b != b)


@functools.lru_cache(maxsize=None)
def _lib() -> C.CDLL:
    """A handle of this module's own on the native library: the argument types set here do not
    touch the functions of fscl_amd.get_lib(), which other tests declare differently."""
    fscl_amd.get_lib()
    return C.CDLL(str(fscl_amd.LIB_PATH))


def log_table() -> np.ndarray:
    L = _lib()
    L.fh_log_table.restype = C.POINTER(C.c_double)
    L.fh_log_table.argtypes = []
    return np.ctypeslib.as_array(L.fh_log_table(), shape=(0x10000,)).copy()


@functools.lru_cache(maxsize=None)
def alpha_grid():
    """(coarse[nc], refine rows [nc + 1] of lists) from fh_alpha_grid."""
    L = _lib()
    coarse = (C.c_double * 16)()
    refine = (C.c_double * (17 * 16))()
    nref = (C.c_int32 * 17)()
    L.fh_alpha_grid.restype = C.c_int
    nc = L.fh_alpha_grid(coarse, 16, refine, nref)
    return ([coarse[i] for i in range(nc)], [[refine[c * 16 + k] for k in range(nref[c])] for c in range(nc + 1)])


def logt(d: np.ndarray, lt: np.ndarray) -> np.ndarray:
    """sm-search.c:40-46."""
    d = np.abs(d.astype(np.int64))
    return np.where(d > 0xFFFFFF, 11.783502069519070 + lt[np.minimum(d >> 16, 0xFFFF)],
                    np.where(d > 0xFFFF, 5.545177444479562 + lt[np.minimum(d >> 8, 0xFFFF)], lt[np.minimum(d, 0xFFFF)]))


def walk_terms(T: Tables, pt: Point, la: float):
    """The terms of one walk in walk order, and its (left, right) part lengths."""
    ws, we, near = pt.window_start, pt.window_end, pt.nearest_snp
    x = logt(T.pos[ws:we + 1].astype(np.int64) - pt.sweep_pos, T.log_table) + la
    out = x > LOG_AD_MAX
    k = near - ws
    if out[k]:
        return np.zeros(0), (-1, -1)
    lo = out[:k][::-1]  # leftwards from the nearest SNP
    nl = int(np.argmax(lo)) if lo.any() else k
    ro = out[k + 1:]
    nr = int(np.argmax(ro)) if ro.any() else len(ro)
    idx = np.concatenate([[k], np.arange(k - 1, k - 1 - nl, -1), np.arange(k + 1, k + 1 + nr)]).astype(np.int64)
    xs = x[idx]
    r = T.row[ws:we + 1][idx].astype(np.int64)
    with np.errstate(all="ignore"):
        iv = np.clip(((xs + 20.0) / T.step).astype(np.int64), 0, T.coef.shape[1] - 1)
        c = T.coef[r, iv]
        t = (xs * (c[:, 0] * xs * xs + c[:, 1] * xs + c[:, 2]) + c[:, 3]) - T.nullrow[r]
    return t, (nl, nr)


def ulp_of(N: float) -> float:
    """The ulp of a negative normal N (the kernels' integer grid); 0.0 when N has no such grid."""
    if not (N < 0.0) or math.isinf(N):
        return 0.0
    m, e = math.frexp(-N)  # -N = m 2^e, m in [0.5, 1)
    if e - 1 < -1022:
        return 0.0
    return math.ldexp(1.0, e - 1 - 52)


def seq_sum(N: float, t: np.ndarray):
    """N + t0 + t1 + ... strictly in order; returns (sum, partial sums)."""
    with np.errstate(all="ignore"):
        p = np.add.accumulate(np.concatenate([[N], t]))
    return float(p[-1]), p


def walk_diag(N: float, t: np.ndarray, p: np.ndarray):
    u = ulp_of(N)
    if u == 0.0:
        return 0, True, math.inf
    with np.errstate(all="ignore"):
        q = t / u
        fin = np.isfinite(q)
        ties = int(np.count_nonzero(np.abs(q[fin] - np.floor(q[fin])) == 0.5))
        mr = float(np.max(np.abs(np.rint(q)))) if len(q) else 0.0
        if mr != mr or not fin.all():
            mr = math.inf
        lo = u * 2.0 ** 52  # |N| in [lo, 2 lo)
        leaves = bool(np.any(~((-p >= lo) & (-p < 2.0 * lo))))
    return ties, leaves, mr


def search(T: Tables, pt: Point, lalpha0: float = LOG_AD_MAX):
    """(lalpha, sm_logl, clr, Diag) of search_maxalpha on the point."""
    coarse, refine = alpha_grid()
    N = float(pt.null_logl)
    D = Diag()
    best, best_la, ci = -DBL_MAX, lalpha0, len(coarse)

    def phase(ph, alphas):
        nonlocal best, best_la
        win = -1
        for j, la in enumerate(alphas):
            t, lens = walk_terms(T, pt, la)
            s, p = seq_sum(N, t)
            ties, leaves, mr = walk_diag(N, t, p)
            D.ties[ph].append(ties); D.leaves[ph].append(leaves); D.max_r[ph].append(mr)
            D.sums[ph].append(s); D.lens[ph].append(lens)
            if s > best:
                best, best_la, win = s, la, j
        return win

    w = phase(0, coarse)
    if w >= 0:
        ci = w
    phase(1, refine[ci])
    with np.errstate(all="ignore"):
        clr = float(np.float64(2.0) * (np.float64(best) - np.float64(N)))
    return best_la, best, clr, D


# ------------------------------------------------------------------ the device shim
class StatsT(C.Structure):  # fsclg_stats_t
    _fields_ = [(k, C.c_ulonglong) for k in ("n_terms", "n_null", "n_walks", "n_maxalpha", "n_unsafe", "n_slow",
                                              "n_ties", "n_cells")] + \
               [("kernel_ms", C.c_double), ("n_launches", C.c_ulonglong), ("cache_iv0", C.c_int),
                ("cache_n_iv", C.c_int), ("cache_n_rows", C.c_int), ("cache_cover", C.c_double),
                ("window_ms", C.c_double), ("n_dup_cells", C.c_ulonglong), ("n_ep_saved", C.c_ulonglong),
                ("busy_ms", C.c_double), ("n_split_retry", C.c_ulonglong)]


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Shim:
    """A device context of its own (fsclg_open(0)) with the alpha grid set."""

    def __init__(self):
        L = self.L = _lib()
        L.fsclg_last_error.restype = C.c_char_p
        P = C.POINTER
        vp, i32 = C.c_void_p, C.POINTER(C.c_int32)
        for name, args in {
            "fsclg_open": [C.c_int, P(vp)], "fsclg_close": [vp],
            "fsclg_upload_tables": [vp, P(C.c_double), P(C.c_double), C.c_int, C.c_int, P(C.c_double), C.c_double],
            "fsclg_upload_snps": [vp, i32, P(C.c_uint32), C.c_int, i32, i32, C.c_int],
            "fsclg_set_alpha_grid": [vp, P(C.c_double), C.c_int, P(C.c_double), i32],
            "fsclg_set_chr_null": [vp, P(C.c_double)],
            "fsclg_search_points": [vp, P(PointT), C.c_int],
            "fsclg_profile": [vp, P(RunT), C.c_int, C.c_int, P(PointT)],
            "fsclg_get_stats": [vp, P(StatsT)], "fsclg_reset_stats": [vp],
        }.items():
            f = getattr(L, name)
            f.restype, f.argtypes = C.c_int, args
        L.fh_alpha_grid.restype = C.c_int
        self.ctx = vp()
        self._ok(L.fsclg_open(0, C.byref(self.ctx)), "fsclg_open")
        coarse = (C.c_double * 16)()
        refine = (C.c_double * (17 * 16))()
        nref = (C.c_int32 * 17)()
        nc = L.fh_alpha_grid(coarse, 16, refine, nref)
        self._ok(L.fsclg_set_alpha_grid(self.ctx, coarse, nc, refine, nref), "fsclg_set_alpha_grid")

    def _ok(self, r, what):
        if r != 0:
            raise RuntimeError(f"{what}: code {r}: {self.L.fsclg_last_error().decode()}")

    def upload(self, T: Tables, chr_start=None, chr_n=None):
        """The tables and sites; chr_start / chr_n: the chromosomes' first sites and lengths (default:
        one chromosome)."""
        coef = np.ascontiguousarray(T.coef, dtype=np.float64)
        nul = np.ascontiguousarray(T.nullrow, dtype=np.float64)
        lt = np.ascontiguousarray(T.log_table, dtype=np.float64)
        self._ok(self.L.fsclg_upload_tables(self.ctx, _pd(lt), _pd(coef), coef.shape[0], coef.shape[1], _pd(nul),
                                            T.step), "fsclg_upload_tables")
        pos = np.ascontiguousarray(T.pos, dtype=np.int32)
        row = np.ascontiguousarray(T.row, dtype=np.uint32)
        if chr_start is None:
            chr_start, chr_n = [0], [len(pos)]
        nc = len(chr_start)
        cs, cn = (C.c_int32 * nc)(*chr_start), (C.c_int32 * nc)(*chr_n)
        self._ok(self.L.fsclg_upload_snps(self.ctx, pos.ctypes.data_as(C.POINTER(C.c_int32)),
                                          row.ctypes.data_as(C.POINTER(C.c_uint32)), len(pos), cs, cn, nc),
                 "fsclg_upload_snps")

    def search(self, pts: list[Point], lalpha0: float = LOG_AD_MAX):
        """fsclg_search_points on the points in one call: [(lalpha, sm_logl, clr)]."""
        n = len(pts)
        a = (PointT * n)()
        for q, p in zip(a, pts):
            q.chr = 0; q.nearest_snp = p.nearest_snp; q.sweep_pos = p.sweep_pos
            q.window_start = p.window_start; q.window_end = p.window_end
            q.n_snps = p.window_end - p.window_start + 1
            q.lalpha = lalpha0; q.null_logl = p.null_logl; q.sm_logl = -DBL_MAX; q.clr = 0.0
        self._ok(self.L.fsclg_search_points(self.ctx, a, n), "fsclg_search_points")
        return [(q.lalpha, q.sm_logl, q.clr) for q in a]

    def set_chr_null(self, N, n_chr: int = 1):
        v = (C.c_double * n_chr)(*([N] * n_chr))
        self._ok(self.L.fsclg_set_chr_null(self.ctx, v), "fsclg_set_chr_null")

    def profile(self, start_pos, step: int = 0, count: int = 0, eval_range: int = 0):
        """One run (start_pos, step, count) on chromosome 0, or start_pos = a list of runs
        (chr, start_pos, step, count) in one call; the points of all runs in order."""
        runs = [(0, start_pos, step, count)] if isinstance(start_pos, int) else list(start_pos)
        run = (RunT * len(runs))(*[RunT(*r) for r in runs])
        count = sum(r[3] for r in runs)
        out = (PointT * count)()
        self._ok(self.L.fsclg_profile(self.ctx, run, len(runs), eval_range, out), "fsclg_profile")
        return [(Point(q.nearest_snp, q.sweep_pos, q.window_start, q.window_end, q.null_logl),
                 (q.lalpha, q.sm_logl, q.clr)) for q in out]

    def stats(self) -> dict:
        st = StatsT()
        self._ok(self.L.fsclg_get_stats(self.ctx, C.byref(st)), "fsclg_get_stats")
        return {k: int(getattr(st, k)) for k in ("n_unsafe", "n_slow", "n_ties", "n_walks", "n_maxalpha")}

    def counters(self) -> tuple:
        """The cumulative device counters every launch adds to: (terms, null-sum elements, walks)."""
        st = StatsT()
        self._ok(self.L.fsclg_get_stats(self.ctx, C.byref(st)), "fsclg_get_stats")
        return int(st.n_terms), int(st.n_null), int(st.n_walks)

    def reset_stats(self):
        self._ok(self.L.fsclg_reset_stats(self.ctx), "fsclg_reset_stats")

    def close(self):
        if self.ctx:
            self.L.fsclg_close(self.ctx)
            self.ctx = C.c_void_p()


# ------------------------------------------------------------------ the crafted vectors
# The N list of the binade-edge, no-integer-path and large-quotient cases (k = 10)
N_EDGE_UP = [-1024.0 * (1.0 + j * 2.0 ** -52) for j in (0, 1, 3)]      # positive terms fall through -2^10
N_EDGE_DOWN = [-2048.0 * (1.0 - j * 2.0 ** -53) for j in (0, 1, 3)]    # negative terms fall through -2^11
N_NOGRID = [0.0, -0.0, 12.5, 5e-324, -5e-324, math.inf, -math.inf, math.nan]
N_LIST = N_EDGE_UP + N_EDGE_DOWN + [-2.0 ** -10, -1e18] + N_NOGRID + [-2.0 ** -40, -3.5]

N_TIE = -700.5                 # |N| in [512, 1024): u = 2^-43, and room for the sums on either side
U_TIE = 2.0 ** -43

# Walk geometry: (left part, right part) lengths of the whole-window walks.  Every length of
# {0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4097} is a left part and a
# right part of some point; the windows are disjoint, so a case places rows per point.
PARTS = [(128, 1023), (0, 4097), (1, 2049), (63, 2048), (64, 2047), (65, 1025), (127, 1024), (129, 0),
         (4097, 129), (2049, 1), (2048, 63), (2047, 64), (1025, 65), (1024, 127), (1023, 128)]
# the nearest SNP's index mod 128 where the geometry fixes it (left_anchor, the partial first trip)
NEAR_MOD = {1: 127, 3: 0, 8: 1, 11: 127, 13: 64}
POS0, SPACING = 5000, 2  # sites every 2 bp: d < 2^16, and the sweep may sit between two sites


@dataclass
class Geom:
    near: int
    ws: int
    we: int
    sweep: int


@functools.lru_cache(maxsize=None)
def geometry():
    """The 15 windows, packed left to right: the first starts at site 0 with its nearest SNP at
    index 128, the last ends at n_snps - 1."""
    g, cur = [], 0
    for k, (nl, nr) in enumerate(PARTS):
        near = cur + nl
        if k in NEAR_MOD:
            near += (NEAR_MOD[k] - near) % 128
        ws = near - nl
        sweep = POS0 + SPACING * near + (k & 1)  # odd points: 1 bp right of the nearest SNP
        g.append(Geom(near, ws, near + nr, sweep))
        cur = near + nr + 1
    return g, cur


def positions(n):
    return (POS0 + SPACING * np.arange(n)).astype(np.int32)


def const_tables(c3: np.ndarray, row: np.ndarray) -> Tables:
    """coef[row][iv] = (0, 0, 0, c3[row]) and nullrow = 0: a site's term is exactly c3[row]."""
    coef = np.zeros((len(c3), N_IV, 4))
    coef[:, :, 3] = np.asarray(c3, dtype=np.float64)[:, None]
    return Tables(positions(len(row)), row.astype(np.uint32), coef, np.zeros(len(c3)), log_table())


@dataclass
class Case:
    name: str
    tables: Tables
    points: list          # [Point]
    want: dict            # counter name -> True: > 0 after each shape of the case; False: 0
    regime: str           # the precondition test_walk_ref checks on the diagnostics


def _points(Ns):
    g, _ = geometry()
    return [Point(q.near, q.sweep, q.ws, q.we, N) for N in Ns for q in g]


def _fill(fn):
    """Rows per site: fn(k, off, q) -> row indices for the window of point k, off = site - nearest."""
    g, n = geometry()
    row = np.zeros(n, dtype=np.int64)
    for k, q in enumerate(g):
        off = np.arange(q.ws, q.we + 1) - q.near
        row[q.ws:q.we + 1] = fn(k, off, q)
    return row


def _ordinary(rng, nrow, lo, hi, scale=1.0, grain=2.0 ** -60):
    """Random multiples of grain * scale of magnitude in [lo, hi) * scale, both signs."""
    m = rng.uniform(lo, hi, nrow) * rng.choice([-1.0, 1.0], nrow)
    return np.round(m / grain) * grain * scale


TIE_M = [0, 1, 2, 3, 12345, 12346]


def _tie_rows():
    """(2m + 1) u / 2 of both signs: t / u = m + 1/2, rint gives an even and an odd-then-bumped R."""
    v = [(2 * m + 1) * U_TIE / 2 for m in TIE_M]
    return np.array(v + [-x for x in v])


def _seg_sites(q: Geom):
    """The last site before and the first after the 1024- and 2048-site segment boundaries of both
    parts (left grid ending at the nearest SNP's block + 128, right grid from the next site's block)."""
    A = (q.near & ~127) + 128
    b1 = (q.near + 1) & ~127
    s = []
    for seg in (1024, 2048):
        s += [A - seg - 1, A - seg, b1 + seg - 1, b1 + seg]
    return [i for i in s if q.ws <= i <= q.we]


def _tie_case(kind: str, odd: bool) -> Case:
    rng = np.random.default_rng(1234)
    # magnitudes up to 0.05: the kernels take a walk as safe only if N minus the sum of its negative
    # terms, and N plus the sum of its positive ones, stay in N's binade, and the whole-window walks
    # (up to 4227 sites) must be safe for their ties to be replayed
    ordinary = _ordinary(rng, 40, 0.001, 0.05)
    ordinary -= np.round(ordinary.mean() / 2.0 ** -60) * 2.0 ** -60  # no drift
    ties = _tie_rows()
    c3 = np.concatenate([[0.0], ordinary, ties])
    t0 = 1 + len(ordinary)

    def fn(k, off, q):
        r = 1 + rng.integers(0, len(ordinary), len(off))
        idx = np.arange(q.ws, q.we + 1)
        if kind == "ends":      # the nearest SNP, the first and last site of each part
            at = [q.near, q.near - 1, q.ws, q.near + 1, q.we]
        elif kind == "lanes":   # lanes 0 and 63 of a trip's two 64-site halves, on both sides
            at = [i for i in range(max(q.ws, q.near - 200), min(q.we, q.near + 200) + 1) if i % 64 in (0, 63)][:14]
        elif kind == "segs":
            at = _seg_sites(q)
        elif kind == "medium":  # 70 ties in one stretch beyond every alpha cut but the whole-window walks'
            far = idx[np.abs(off) * SPACING > 1400]
            at = list(far[:140:2]) if len(far) >= 140 else []
        else:                   # dense: every 7th site
            at = list(idx[::7])
        at = sorted(set(i for i in at if q.ws <= i <= q.we))
        for j, i in enumerate(at):
            r[i - q.ws] = t0 + (j * 5 + k) % len(ties)
        return r

    N = N_TIE - U_TIE if odd else N_TIE
    want = {"n_ties": True}
    if kind in ("ends", "segs"):  # every walk safe: the values come from resolve_walk's tie replay
        want.update(n_unsafe=False, n_slow=False)
    if kind == "dense":
        want["n_slow"] = True
    return Case(f"ties-{kind}-{'odd' if odd else 'even'}", const_tables(c3, _fill(fn)), _points([N]), want,
                {"ends": "sparse", "lanes": "sparse", "segs": "sparse"}.get(kind, kind))


def _edge_case(kind: str) -> Case:
    """Partial sums that leave N's binade, with u = ulp(N) = 2^-42 (N in [-2048, -1024])."""
    rng = np.random.default_rng(77)
    u = 2.0 ** -42
    frac = _ordinary(rng, 24, 0.05, 6.0, scale=u, grain=2.0 ** -10)   # a few ulp, 10 fractional bits
    pos_rows, neg_rows = np.abs(frac), -np.abs(frac)
    big = np.array([8192.0 * u + 0.3125 * u, -(8192.0 * u + 0.3125 * u), 200000.0 * u + 0.6875 * u,
                    -(200000.0 * u + 0.6875 * u)])
    c3 = np.concatenate([[0.0], pos_rows, neg_rows, big])
    P0, M0, B0 = 1, 1 + len(frac), 1 + 2 * len(frac)
    sign = -1 if kind.startswith("down") else 1
    base_in, base_out = (P0, M0) if sign > 0 else (M0, P0)   # rows moving towards / away from the edge
    bigin, bigout = (B0, B0 + 1) if sign > 0 else (B0 + 1, B0)

    if kind == "up-tiny":  # terms below u / 2 from the edge itself, and exactly u to step onto it
        pos_rows = np.abs(_ordinary(rng, 24, 0.05, 0.45, scale=u, grain=2.0 ** -10))
        c3[P0:P0 + 24] = pos_rows
        c3[B0] = u

    def fn(k, off, q):
        n = len(off)
        d = np.abs(off)
        dm = int(d.max())  # >= 128: the zones scale with the window
        toward = base_in + rng.integers(0, len(frac), n)
        away = base_out + rng.integers(0, len(frac), n)
        zero = np.zeros(n, dtype=np.int64)
        if kind == "up-tiny":
            r = np.where(d > 100, zero, toward)
            r[d == 1] = B0
        elif kind in ("up-first", "down-first"):    # the first terms cross the edge
            r = np.where(d > 5, zero, toward)       # an all-zero row beyond: the longer walks' sums are equal
        elif kind in ("up-later", "down-later"):    # away first, back through the edge further out
            r = np.where(d < 40, away, np.where((d > dm // 2) & (d < 3 * dm // 4), toward, zero))
            r[d == 7 * dm // 8] = bigin             # well past the edge
        elif kind in ("up-last", "down-last"):      # only the walk's last term crosses
            r = np.where(d < 40, away, zero)
            r[-1 if q.we > q.near else 0] = bigin + 2
        else:                                       # "back": through the edge and back again
            r = np.where(d < 40, away, zero)
            r[d == dm // 3] = bigin
            r[d == 2 * dm // 3] = bigout
            r[d == 2 * dm // 3 + 1] = bigout
        return r

    Ns = N_EDGE_DOWN if sign < 0 else N_EDGE_UP
    if kind == "up-tiny":  # (from j = 3 every term is absorbed: that sum never reaches the edge)
        Ns = N_EDGE_UP[:2]
    return Case(f"edge-{kind}", const_tables(c3, _fill(fn)), _points(Ns), {"n_unsafe": True, "n_slow": True},
                "leaves")


def _random_rows_case(name, Ns, lo, hi, mean, want, regime, extra=None, seed=5) -> Case:
    """Ordinary random rows of magnitude [lo, hi) shifted by mean; extra(k, off, q, r) edits the rows
    (row indices 41.. are the values of extra's list)."""
    rng = np.random.default_rng(seed)
    ordinary = _ordinary(rng, 40, lo, hi) + mean
    xv = extra[0] if extra else []
    c3 = np.concatenate([[0.0], ordinary, xv])

    def fn(k, off, q):
        r = 1 + rng.integers(0, len(ordinary), len(off))
        r[np.abs(off) > 3000] = 0  # an all-zero row at the far end: neighbouring long walks' sums are equal
        if extra:
            extra[1](k, off, q, r)
        return r

    return Case(name, const_tables(c3, _fill(fn)), _points(Ns), want, regime)


def _far(off, j):
    """Index of the j-th site beyond every alpha cut but the longest walks'."""
    i = np.flatnonzero(np.abs(off) * SPACING > 1400)
    if len(i) <= j + 2:  # a short window: beyond the cut of the alphas above -0.8 (d <= 121)
        i = np.flatnonzero(np.abs(off) * SPACING > 130)
    return int(i[j]) if len(i) > j + 2 else -1


def _put(values_at):
    def f(k, off, q, r):
        for j, rowi in values_at:
            i = _far(off, j)
            if i >= 0:
                r[i] = 41 + rowi
    return f


def _every9(k, off, q, r):
    """u = 128 at N = -1e18: 64.0 and 192.0 are ties (t / u = 1/2, 3/2), every other term rounds to 0."""
    i = np.arange(4, len(off), 9)
    r[i] = 41 + (i // 9) % 3


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = []
    # (a) ties
    for kind in ("ends", "lanes", "segs", "medium", "dense"):
        for odd in (False, True):
            out.append(_tie_case(kind, odd))
    # (b) binade edges
    for kind in ("up-tiny", "up-first", "up-later", "up-last", "down-first", "down-later", "down-last", "back"):
        out.append(_edge_case(kind))
    out.append(_random_rows_case("edge-nonneg", [-2.0 ** -10], 0.05, 0.15, 0.01, {"n_unsafe": True, "n_slow": True},
                                 "nonneg"))
    out.append(_random_rows_case("edge-1e18", [-1e18], 0.01, 1.0, 0.0,
                                 {"n_ties": True, "n_unsafe": True, "n_slow": True}, "ties1e18",
                                 extra=([64.0, -64.0, 192.0], _every9)))
    # (c) no integer path
    out.append(_random_rows_case("nogrid", N_NOGRID, 0.01, 1.0, 0.002, {"n_slow": True}, "nogrid"))
    # (d) large quotients
    out.append(_random_rows_case("big-quotient", [-2.0 ** -40], 0.5, 1.5, 0.0, {"n_unsafe": True}, "big"))
    out.append(_random_rows_case("huge-plus", [-3.5], 0.01, 1.0, 0.0, {"n_unsafe": True}, "big",
                                 extra=([1e300, -1e300], _put([(3, 0)]))))
    out.append(_random_rows_case("huge-minus", [-3.5], 0.01, 1.0, 0.0, {"n_unsafe": True}, "big",
                                 extra=([1e300, -1e300], _put([(3, 1)]))))
    # +1e300 then -1e300 as consecutive terms of the walk: they cancel in walk order only
    out.append(_random_rows_case("huge-pair", [-3.5], 0.01, 1.0, 0.002, {"n_unsafe": True}, "big",
                                 extra=([1e300, -1e300], _put([(3, 0), (4, 1)]))))
    # (e) non-finite rows, reached by the long walks only
    nf = [math.nan, math.inf, -math.inf]
    out.append(_random_rows_case("row-nan", [N_TIE], 0.01, 1.0, -0.002, {"n_unsafe": True}, "nonfinite",
                                 extra=(nf, _put([(3, 0)]))))
    out.append(_random_rows_case("row-inf-both", [N_TIE], 0.01, 1.0, -0.002, {"n_unsafe": True}, "nonfinite",
                                 extra=(nf, _put([(3, 1), (9, 2)]))))
    out.append(_random_rows_case("row-inf-plus", [N_TIE], 0.01, 1.0, -0.002, {"n_unsafe": True}, "nonfinite",
                                 extra=(nf, _put([(3, 1)]))))
    # (f) equal maxima: an all-zero table
    g, n = geometry()
    zero = const_tables(np.zeros(2), np.zeros(n, dtype=np.int64))
    out.append(Case("zero-exact", zero, _points([N_TIE]), {}, "allequal"))
    out.append(Case("zero-inexact", zero, _points(N_EDGE_UP[:1] + N_EDGE_DOWN[:1] + [0.0]), {"n_slow": True},
                    "allequal"))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """[(lalpha, sm_logl, clr, Diag)] of the case's points, computed once."""
    c = cases()[name]
    return [search(c.tables, p) for p in c.points]


def shapes(n: int):
    """Index lists of the three kernel shapes: every point alone (8 members), 40 points (6 members),
    130 points (the unsplit kernel); the multi-point calls repeat and interleave the points."""
    one = [[i] for i in range(n)]
    s40 = [(7 * j) % n for j in range(40)] if math.gcd(7, n) == 1 else [(j * 7 + j // n) % n for j in range(40)]
    s130 = [(11 * j + j // n) % n for j in range(130)]
    return one, s40, s130


# ------------------------------------------------------------------ real tables through the oracle
class OrcSnp(C.Structure):  # orc_snp_t
    _fields_ = [("chr", C.c_int), ("pos", C.c_int), ("null_logl", C.c_double), ("obs_freq", C.c_int),
                ("depth_p", C.c_int), ("folded", C.c_int)]


class OrcSpline(C.Structure):  # orc_spline_t
    _fields_ = [("n", C.c_int), ("knots", C.POINTER(C.c_double)), ("coef", C.POINTER(C.c_double))]


class OrcTable(C.Structure):  # orc_table_t
    _fields_ = [("spline", C.POINTER(OrcSpline)), ("fspline", C.POINTER(OrcSpline)), ("sample_size", C.c_int)]


class OracleTables:
    """An SNP file in the oracle, its tables flattened to the shim's coef / nullrow / row layout (one
    row per distinct (depth, folded, frequency, null value) of the sites), and orc_search_maxalpha on
    caller-initialised points."""

    def __init__(self, snp):
        import sys
        from util import ROOT
        sys.path.insert(0, str(ROOT / "oracle"))
        import oracle as orc
        self.orc = orc
        self.o = orc.OracleScan(snp)
        L, s = self.o.L, self.o.s.contents
        L.orc_search_maxalpha.argtypes = [C.POINTER(orc.OrcPt), C.c_void_p, C.c_void_p, C.POINTER(orc.OrcStats)]
        L.orc_search_maxalpha.restype = None
        L.orc_log_ad_step.restype = C.c_double
        snps = C.cast(s.snps, C.POINTER(OrcSnp))
        tab = C.cast(self.o.tab, C.POINTER(OrcTable))
        keys, rows, coef, nul = {}, [], [], []
        pos = np.zeros(s.n_snps, dtype=np.int32)
        for i in range(s.n_snps):
            p = snps[i]
            key = (p.depth_p, p.folded, p.obs_freq, bits(p.null_logl))
            if key not in keys:
                keys[key] = len(keys)
                sp = (tab[p.depth_p].fspline if p.folded else tab[p.depth_p].spline)[p.obs_freq]
                assert sp.n == N_IV
                coef.append(np.ctypeslib.as_array(sp.coef, shape=(sp.n, 4)).copy())
                nul.append(p.null_logl)
            rows.append(keys[key])
            pos[i] = p.pos
        self.tables = Tables(pos, np.array(rows, dtype=np.uint32), np.array(coef), np.array(nul), log_table(),
                             float(L.orc_log_ad_step()))

    def search(self, pt: Point, lalpha0: float = LOG_AD_MAX):
        q = self.orc.OrcPt()
        q.chr = 0; q.nearest_snp = pt.nearest_snp; q.sweep_pos = pt.sweep_pos
        q.window_start = pt.window_start; q.window_end = pt.window_end
        q.n_snps = pt.window_end - pt.window_start + 1
        q.lalpha = lalpha0; q.null_logl = pt.null_logl; q.sm_logl = -DBL_MAX; q.clr = 0.0
        self.o.L.orc_search_maxalpha(C.byref(q), self.o.s.contents.snps, self.o.tab, C.byref(self.o.stats))
        return q.lalpha, q.sm_logl, q.clr


def golden_points(dump_rows) -> list:
    """Points of a golden dump (tests/util.read_dump rows), with their own null_logl."""
    return [Point(r[6], r[1], r[7], r[8], r[5]) for r in dump_rows]


# ------------------------------------------------------------------ two points per search (fsclg_profile)
PROFILE_N, PROFILE_ER = 6000, 20000          # one whole-chromosome window: n_snps <= 2 eval_range + 1
PROFILE_RUN = (POS0 + 2 * 400 + 1, 1600, 7)  # odd positions (no SNP there) beside sites 400, 1200, ..., 5200
PROFILE_SAFE, PROFILE_SLOW = 2, 3            # the "edge" pair: positions 2 and 3 share a search


@dataclass
class ProfileCase:
    name: str
    tables: Tables
    N: float
    want: dict


@functools.lru_cache(maxsize=None)
def profile_cases() -> dict:
    n = PROFILE_N
    rng = np.random.default_rng(99)
    out = []
    # (a)-dense: small ordinary rows, every 7th site a tie
    ordinary = _ordinary(rng, 40, 0.001, 0.05)
    ordinary -= np.round(ordinary.mean() / 2.0 ** -60) * 2.0 ** -60
    ties = _tie_rows()
    row = 1 + rng.integers(0, 40, n)
    at = np.arange(3, n, 7)
    row[at] = 41 + (at // 7) % len(ties)
    out.append(ProfileCase("dense", const_tables(np.concatenate([[0.0], ordinary, ties]), row), N_TIE,
                           {"n_ties": True, "n_slow": True}))
    # (b): N three units below -2^10.  Zero rows but for five positive rows around site 2800 (the walks
    # of the position there cross the edge at once, and those cut before the negative rows have equal
    # sums: the slow path) and eleven large negative rows at 2400.. and 3200.. (a walk that reaches the
    # positive rows from elsewhere has met these: inexact, but far below the exact short walks)
    u = 2.0 ** -42
    c3 = np.array([0.0, 1.3125 * u, 2.6875 * u, 0.8125 * u, -(9.0 + 0.4375 * u)])
    row = np.zeros(n, dtype=np.int64)
    row[2798:2803] = [1, 2, 3, 1, 2]
    row[2400:2411] = 4
    row[3200:3211] = 4
    out.append(ProfileCase("edge", const_tables(c3, row), N_EDGE_UP[2], {"n_unsafe": True, "n_slow": True}))
    # +1e300 then -1e300 on neighbouring sites: every position's longest walks meet both
    row = 1 + rng.integers(0, 40, n)
    row[3000], row[3001] = 41, 42
    out.append(ProfileCase("huge-pair", const_tables(np.concatenate([[0.0], _ordinary(rng, 40, 0.01, 1.0) + 0.002,
                                                                     [1e300, -1e300]]), row), -3.5,
                           {"n_unsafe": True, "n_slow": True}))
    return {c.name: c for c in out}


class OrcChr(C.Structure):  # orc_chr_t
    _fields_ = [("chr", C.c_int), ("name", C.c_char_p), ("start_index", C.c_int), ("n_snps", C.c_int),
                ("start_pos", C.c_int), ("bp_length", C.c_int)]


def oracle_init_points(pos: np.ndarray, at: list, eval_range: int, N: float) -> list:
    """orc_init_scan_result at each position of one chromosome with SNPs at pos; the points with
    their null_logl replaced by N."""
    import sys
    from util import ROOT
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as orc
    L = orc.load()
    L.orc_init_scan_result.argtypes = [C.POINTER(orc.OrcPt), C.c_int, C.c_void_p, C.POINTER(OrcChr), C.c_int, C.c_int,
                                       C.c_void_p]
    L.orc_init_scan_result.restype = None
    snps = (OrcSnp * len(pos))()
    for s_, p in zip(snps, pos):
        s_.pos = int(p)
    lim = OrcChr(0, b"c", 0, len(pos), int(pos[0]), int(pos[-1]))
    out = []
    for x in at:
        q = orc.OrcPt()
        L.orc_init_scan_result(C.byref(q), 0, snps, C.byref(lim), eval_range, int(x), None)
        out.append(Point(q.nearest_snp, q.sweep_pos, q.window_start, q.window_end, N))
    return out
