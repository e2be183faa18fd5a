"""The per-site likelihood terms (fsclg_sites_submit, --sites-file) on the GPU.

Every term of a walk is compared by bit pattern (NaN equal to NaN) with the plain reference of
tests/walk_ref.py, the header's bounds with its walk lengths, and the header's sm_logl with the
strictly sequential sum of the null sum and the terms.
"""
from __future__ import annotations

import ctypes as C
import math
import subprocess
import sys

import numpy as np
import pytest

import fscl_amd
import walk_ref as wr
from fscl_amd import synth
from util import CLI, GOLD, ROOT, read_dump, same_bits

sys.path.insert(0, str(ROOT / "oracle"))
import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SENT64 = int.from_bytes(bytes([SENTINEL] * 8), "little")
WG = 768            # the kernel's workgroup: its threads stride over a walk's terms
FORCED_CAP = 64     # the forced launch capacity of the cut test
E_ARG, E_STATE = -1, -3


def same_arr(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def fold(N, t) -> float:
    """N + t_0 + t_1 + ... one by one, in NumPy doubles."""
    acc = np.float64(N)
    with np.errstate(all="ignore"):
        for x in np.asarray(t, dtype=np.float64):
            acc = acc + x
    return float(acc)


def point_of(h) -> wr.Point:
    q = h["pt"]
    return wr.Point(int(q["nearest_snp"]), int(q["sweep_pos"]), int(q["window_start"]), int(q["window_end"]),
                    float(q["null_logl"]))


def check_walk(h, terms, T, la, what, bad, cache=None):
    """One header and its terms against walk_ref on the header's own geometry."""
    pt = point_of(h)
    key = (pt.nearest_snp, pt.sweep_pos, pt.window_start, pt.window_end, wr.bits(la))
    if cache is not None and key in cache:
        t, (nl, nr) = cache[key]
    else:
        t, (nl, nr) = wr.walk_terms(T, pt, la)
        if cache is not None:
            cache[key] = (t, (nl, nr))
    want = (max(nl, 0), max(nr, 0), len(t))
    got = (int(h["nl"]), int(h["nr"]), int(h["len"]))
    if got != want or int(h["pad"]) != 0:
        bad.append(f"{what}: (nl, nr, len) {got} != {want}")
        return
    mine = terms[int(h["off"]):int(h["off"]) + len(t)]
    if not same_arr(mine, t):
        k = int(np.flatnonzero(~((mine.view(np.int64) == t.view(np.int64)) | (np.isnan(mine) & np.isnan(t))))[0])
        bad.append(f"{what}: term {k} of {len(t)}: {float(mine[k]).hex()} != {float(t[k]).hex()}")
    s = wr.seq_sum(pt.null_logl, t)[0]
    if not wr.same(float(h["pt"]["sm_logl"]), s):
        bad.append(f"{what}: sm_logl {float(h['pt']['sm_logl']).hex()} != {s.hex()}")
    with np.errstate(all="ignore"):
        clr = float(np.float64(2.0) * (np.float64(s) - np.float64(pt.null_logl)))
    if not (wr.same(float(h["pt"]["clr"]), clr) and wr.same(float(h["pt"]["lalpha"]), la)):
        bad.append(f"{what}: clr / lalpha {h['pt']['clr']!r} {h['pt']['lalpha']!r} != {clr!r} {la!r}")


# ------------------------------------------------------------------ the shim alone
class SitesShim(wr.Shim):
    def __init__(self):
        super().__init__()
        L, vp = self.L, C.c_void_p
        L.fsclg_sites_submit.restype, L.fsclg_sites_submit.argtypes = C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]
        L.fsclg_sites_wait.restype = C.c_int
        L.fsclg_sites_wait.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.fsclg_sites_last_ms.restype, L.fsclg_sites_last_ms.argtypes = C.c_double, [vp, C.c_int]
        L.fsclg_slot_set_rows.restype, L.fsclg_slot_set_rows.argtypes = C.c_int, [vp, C.c_int, vp, vp]

    @staticmethod
    def requests(reqs):
        a = np.zeros(max(len(reqs), 1), dtype=fscl_amd.SITE_REQ_DTYPE)
        for q, r in zip(a, reqs):
            q["chr"], q["pos"], q["lalpha"] = r
        return a

    def submit(self, reqs, eval_range, batch=0, slot=0) -> int:
        a = self.requests(reqs)
        return self.L.fsclg_sites_submit(self.ctx, batch, slot, a.ctypes.data, len(reqs), eval_range)

    def wait(self, n, batch=0, slack=16):
        """(headers, terms, the sentinel-filled tail): sized by a first wait with no room."""
        hdr = np.zeros(max(n, 1), dtype=fscl_amd.SITES_DTYPE)
        hdr.view(np.uint8)[:] = SENTINEL
        nt = C.c_size_t(12345)
        r = self.L.fsclg_sites_wait(self.ctx, batch, hdr.ctypes.data, None, 0, C.byref(nt))
        if r == 0:  # no term at all: that wait was the whole of it
            assert nt.value == 0
            return hdr[:n], np.zeros(0), np.zeros(0, dtype=np.uint64)
        assert r == E_ARG, f"sizing wait: code {r}"
        assert (hdr.view(np.uint8) == SENTINEL).all(), "a wait that only sizes wrote headers"
        buf = np.full(nt.value + slack, SENT64, dtype=np.uint64)
        nt2 = C.c_size_t(0)
        self._ok(self.L.fsclg_sites_wait(self.ctx, batch, hdr.ctypes.data, buf.ctypes.data, nt.value, C.byref(nt2)),
                 "fsclg_sites_wait")
        assert nt2.value == nt.value
        return hdr[:n], buf[:nt.value].view(np.float64), buf[nt.value:]

    def sites(self, reqs, eval_range, batch=0, slot=0):
        if slot == 0:
            self._ok(self.L.fsclg_slot_set_rows(self.ctx, 0, None, None), "fsclg_slot_set_rows")  # the uploaded rows
        self._ok(self.submit(reqs, eval_range, batch, slot), "fsclg_sites_submit")
        hdr, terms, tail = self.wait(len(reqs), batch)
        words = hdr.view(np.uint8).view(np.uint32)
        assert not (words == int.from_bytes(bytes([SENTINEL] * 4), "little")).any(), "a header was left unwritten"
        assert not (terms.view(np.uint64) == SENT64).any(), "a term was left unwritten"
        assert (tail == SENT64).all(), "a store past the terms"
        assert hdr["off"].tolist() == (np.cumsum(hdr["len"]) - hdr["len"]).tolist()
        return hdr, terms


@pytest.fixture(scope="module")
def shim(built):
    s = SitesShim()
    yield s
    s.close()


CASE_ER = 5000  # above every window of the geometry: each chromosome is one whole-chromosome window


def case_chromosomes():
    """The 15 windows of walk_ref.geometry() as 15 chromosomes (as tests/test_curve_gpu.py)."""
    g, n = wr.geometry()
    start = [q.ws for q in g]
    return start, [b - a for a, b in zip(start, start[1:] + [n])]


def grid_alphas():
    coarse, refine = wr.alpha_grid()
    seen, out = set(), []
    for la in list(coarse) + [x for row in refine for x in row]:
        if wr.bits(la) not in seen:
            seen.add(wr.bits(la))
            out.append(la)
    return out


def edge_alphas(T, pt):
    """The greatest alpha whose walk still takes the nearest SNP, and the next double above it."""
    d = abs(pt.sweep_pos - int(T.pos[pt.nearest_snp]))
    lt = float(wr.logt(np.array([d]), T.log_table)[0])
    la = wr.LOG_AD_MAX - lt
    while lt + la > wr.LOG_AD_MAX:
        la = math.nextafter(la, -math.inf)
    while lt + math.nextafter(la, math.inf) <= wr.LOG_AD_MAX:
        la = math.nextafter(la, math.inf)
    return la, math.nextafter(la, math.inf)


CRAFT_LEN = [0, 1, 63, 64, 65, WG, WG + 1, 2000]  # (65 and more: longer than one launch at FORCED_CAP)
CRAFT_D0 = 101


def crafted_lengths():
    """Requests left of the first site of chromosome 1 (4 098 sites every 2 bp, no left part): the nearest
    SNP is CRAFT_D0 bp away and the walk takes the sites up to a distance cut between two of them."""
    g, _ = wr.geometry()
    pos = wr.POS0 + wr.SPACING * g[1].ws - CRAFT_D0
    return [(1, pos, wr.LOG_AD_MAX - math.log(CRAFT_D0 + 2 * (L - 1) + 1)) for L in CRAFT_LEN]


@pytest.mark.parametrize("name", list(wr.cases()))
def test_crafted_terms(shim, name):
    c = wr.cases()[name]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)]
    Ns = list({wr.bits(p.null_logl): p.null_logl for p in c.points}.values())
    grid = grid_alphas()
    mid = 0.5 * (grid[3] + grid[4])
    assert wr.bits(mid) not in {wr.bits(x) for x in grid}
    bad, cache, lens = [], {}, set()
    try:
        shim.upload(c.tables, cs, cn)
        for N in Ns:
            shim.set_chr_null(N, len(cs))
            prof = shim.profile(runs, eval_range=CASE_ER)
            reqs = []
            for k, q in enumerate(g):
                pp = prof[k][0]
                reqs += [(k, q.sweep, la) for la in grid + [mid] + list(edge_alphas(c.tables, pp))]
            reqs += crafted_lengths()
            hdr, terms = shim.sites(reqs, CASE_ER)
            for i, (h, (k, pos, la)) in enumerate(zip(hdr, reqs)):
                what = f"N={N!r} request {i} (chr {k}, pos {pos}, la {la!r})"
                if i < len(reqs) - len(CRAFT_LEN):  # the geometry is the profile's at the same position
                    pp = prof[k][0]
                    me = point_of(h)
                    if (me.nearest_snp, me.sweep_pos, me.window_start, me.window_end) != \
                            (pp.nearest_snp, pp.sweep_pos, pp.window_start, pp.window_end):
                        bad.append(f"{what}: point {me} != profile {pp}")
                if int(h["pt"]["chr"]) != k or not wr.same(float(h["pt"]["null_logl"]), N):
                    bad.append(f"{what}: chr / null_logl {h['pt']['chr']} {h['pt']['null_logl']!r}")
                check_walk(h, terms, c.tables, la, what, bad, cache)
                lens.add(int(h["len"]))
            # the nudged pair straddles the nearest SNP: just inside, just outside
            per = len(grid) + 3
            for k in range(len(g)):
                a, b = hdr[k * per + per - 2], hdr[k * per + per - 1]
                if not (int(a["len"]) >= 1 and int(b["len"]) == 0 and wr.same(float(b["pt"]["sm_logl"]), N)):
                    bad.append(f"N={N!r} point {k}: edge alphas give len {a['len']} / {b['len']}")
            if hdr["len"][-len(CRAFT_LEN):].tolist() != CRAFT_LEN:
                bad.append(f"crafted lengths {hdr['len'][-len(CRAFT_LEN):].tolist()} != {CRAFT_LEN}")
    except RuntimeError as e:  # a device error: nothing more runs on the GPU in this session
        pytest.exit(f"{name}: {e}", returncode=3)
    # (checked on the reference's side too: check_walk compares every len with walk_ref's)
    assert set(CRAFT_LEN) <= lens and any(x > FORCED_CAP for x in lens), f"{name}: walk lengths {sorted(lens)[:20]}"
    assert not bad, f"{name}: {len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ launch cuts, buffers, errors
def small_requests():
    g, _ = wr.geometry()
    reqs = crafted_lengths()[:5] + [(0, g[0].sweep, -1.0), (2, g[2].sweep, 0.5), (14, g[14].sweep, 9.0)]
    return reqs


def test_launch_cuts_and_buffers(shim, monkeypatch):
    c = wr.cases()["ties-ends-even"]
    cs, cn = case_chromosomes()
    reqs = small_requests()
    got = {}
    try:
        shim.upload(c.tables, cs, cn)
        shim.set_chr_null(wr.N_TIE, len(cs))
        for cap in (None, 1, FORCED_CAP):
            if cap is None:
                monkeypatch.delenv("FSCLG_SITES_CAP", raising=False)
            else:
                monkeypatch.setenv("FSCLG_SITES_CAP", str(cap))
            assert fscl_amd.sites_cap() == (cap or 1 << 22)
            hdr, terms = shim.sites(reqs, CASE_ER)
            got[cap] = (hdr.tobytes(), terms.tobytes())
            if cap is None:
                bad = []
                for i, (h, r) in enumerate(zip(hdr, reqs)):
                    check_walk(h, terms, c.tables, r[2], f"request {i}", bad)
                assert not bad, "\n".join(bad[:12])
                assert hdr["len"].max() > FORCED_CAP and int(hdr["len"].sum()) == len(terms)
        monkeypatch.delenv("FSCLG_SITES_CAP", raising=False)
        assert got[1] == got[None] and got[FORCED_CAP] == got[None], "the result depends on the launch cut"
        # a buffer one term short: the count, nothing written, and the batch still answers a second wait
        n, total = len(reqs), len(got[None][1]) // 8
        shim._ok(shim.submit(reqs, CASE_ER), "fsclg_sites_submit")
        hdr = np.zeros(n, dtype=fscl_amd.SITES_DTYPE)
        buf = np.full(total, SENT64, dtype=np.uint64)
        nt = C.c_size_t(0)
        L = shim.L
        assert L.fsclg_sites_wait(shim.ctx, 0, hdr.ctypes.data, buf.ctypes.data, total - 1, C.byref(nt)) == E_ARG
        assert nt.value == total and (buf == SENT64).all() and not hdr.view(np.uint8).any()
        assert L.fsclg_sites_wait(shim.ctx, 0, None, buf.ctypes.data, total, C.byref(nt)) == E_ARG  # no headers
        assert shim.submit(reqs, CASE_ER) == E_STATE                     # the batch is still pending
        assert L.fsclg_sites_wait(shim.ctx, 0, hdr.ctypes.data, buf.ctypes.data, total, None) == 0
        assert (hdr.tobytes(), buf.tobytes()) == got[None]
        assert L.fsclg_sites_last_ms(shim.ctx, 0) > 0.0
        # the documented codes
        assert L.fsclg_sites_wait(shim.ctx, 0, hdr.ctypes.data, buf.ctypes.data, total, None) == E_STATE  # nothing submitted
        assert shim.submit([(len(cs), 5000, -1.0)], CASE_ER) == E_ARG    # chromosome
        assert shim.submit([(-1, 5000, -1.0)], CASE_ER) == E_ARG
        assert shim.submit([(0, 5000, math.nan)], CASE_ER) == E_ARG      # lalpha
        assert shim.submit([(0, 5000, -20.5)], CASE_ER) == E_ARG
        assert shim.submit([(0, 2 ** 31 - 10, -1.0)], CASE_ER) == E_ARG  # position
        assert shim.submit(reqs, CASE_ER, batch=10) == E_ARG and shim.submit(reqs, CASE_ER, batch=-1) == E_ARG
        assert shim.submit(reqs, CASE_ER, slot=8) == E_ARG and shim.submit(reqs, CASE_ER, slot=-1) == E_ARG
        assert L.fsclg_sites_wait(shim.ctx, 10, hdr.ctypes.data, buf.ctypes.data, total, None) == E_ARG
        # an empty call, and a call whose walks are all empty
        hdr0, t0 = shim.sites([], CASE_ER)
        assert len(hdr0) == 0 and len(t0) == 0
        hdr1, t1 = shim.sites([(3, 5000, 30.0), (4, 5000, math.inf)], CASE_ER)
        assert hdr1["len"].tolist() == [0, 0] and len(t1) == 0
        assert all(wr.same(float(x), wr.N_TIE) for x in hdr1["pt"]["sm_logl"]) and (hdr1["pt"]["clr"] == 0.0).all()
    except RuntimeError as e:
        pytest.exit(f"launch cuts: {e}", returncode=3)


def test_another_slots_rows(shim):
    """Rows rearranged within their chromosomes in slot 3, evaluated on batch 2: the terms are the
    reference's on the rearranged rows; slot 0 answers as before."""
    c = wr.cases()["nogrid"]
    T = c.tables
    cs, cn = case_chromosomes()
    rng = np.random.default_rng(11)
    perm = np.concatenate([a + rng.permutation(n) for a, n in zip(cs, cn)])
    Tp = wr.Tables(T.pos, T.row[perm], T.coef, T.nullrow, T.log_table, T.step)
    g, _ = wr.geometry()
    reqs = [(k, q.sweep, la) for k, q in enumerate(g) for la in (-3.2, 0.4)] + crafted_lengths()
    N = -812.25
    try:
        shim.upload(T, cs, cn)
        shim.set_chr_null(N, len(cs))
        before = shim.sites(reqs, CASE_ER)
        rows = np.ascontiguousarray(Tp.row, dtype=np.uint32)
        nul = (C.c_double * len(cs))(*([N] * len(cs)))
        shim._ok(shim.L.fsclg_slot_set_rows(shim.ctx, 3, rows.ctypes.data, C.cast(nul, C.c_void_p)), "fsclg_slot_set_rows")
        hdr, terms = shim.sites(reqs, CASE_ER, batch=2, slot=3)
        after = shim.sites(reqs, CASE_ER)
    except RuntimeError as e:
        pytest.exit(f"another slot: {e}", returncode=3)
    bad = []
    for i, (h, r) in enumerate(zip(hdr, reqs)):
        check_walk(h, terms, Tp, r[2], f"slot 3, request {i}", bad)
    for i, (h, r) in enumerate(zip(before[0], reqs)):
        check_walk(h, before[1], T, r[2], f"slot 0, request {i}", bad)
    assert not bad, "\n".join(bad[:12])
    assert terms.tobytes() != before[1].tobytes()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()


# ------------------------------------------------------------------ the whole library
def setup(snp):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    scan = fscl_amd.load_snp_input(snp)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp)
    fscl_amd.compute_snp_null_model(scan, fsp)
    return scan, tab


def test_golden_points(built):
    pts = read_dump(GOLD / "g2_p30.dump")
    scan, tab = setup(GOLD / "g2.snp")
    hdr, terms = fscl_amd.scan_sites(scan, tab, [(r[0], r[1], r[3]) for r in pts])
    assert len(hdr) == len(pts) and int(hdr["len"].sum()) == len(terms)
    for h, r in zip(hdr, pts):
        q = h["pt"]
        assert (int(q["chr"]), int(q["sweep_pos"]), int(q["nearest_snp"]), int(q["window_start"]), int(q["window_end"])) == \
            (r[0], r[1], r[6], r[7], r[8])
        assert same_bits(float(q["null_logl"]), r[5]) and same_bits(float(q["lalpha"]), r[3])
        t = terms[int(h["off"]):int(h["off"]) + int(h["len"])]
        assert same_bits(fold(r[5], t), r[4]), "the fold of the terms is not the golden sm_logl"
        assert same_bits(float(q["sm_logl"]), r[4]) and same_bits(float(q["clr"]), r[2])
    # every alpha of the points' curves: the walk's sum is the curve's entry
    cv = fscl_amd.scan_curves(scan, tab, [(r[0], r[1]) for r in pts])
    reqs, want = [], []
    for rec, r in zip(cv, pts):
        for k in range(int(rec["n_coarse"]) + int(rec["n_refine"])):
            reqs.append((r[0], r[1], float(rec["la"][k])))
            want.append(float(rec["sm"][k]))
    hdr2, terms2 = fscl_amd.scan_sites(scan, tab, reqs)
    assert len(reqs) >= 25 * len(pts)
    for h, w, r in zip(hdr2, want, reqs):
        assert same_bits(float(h["pt"]["sm_logl"]), w), f"{r}: {h['pt']['sm_logl']!r} != curve {w!r}"


class OrcChr(C.Structure):  # orc_chr_t
    _fields_ = [("chr", C.c_int), ("name", C.c_char_p), ("start_index", C.c_int), ("n_snps", C.c_int),
                ("start_pos", C.c_int), ("bp_length", C.c_int)]


def oracle_init(snp, chr_pos, er):
    """orc_init_scan_result at each (chr, pos): (nearest, sweep_pos, window_start, window_end, null_logl)."""
    o = orc.OracleScan(snp)
    L, s = o.L, o.s.contents
    L.orc_init_scan_result.argtypes = [C.POINTER(orc.OrcPt), C.c_int, C.c_void_p, C.POINTER(OrcChr), C.c_int, C.c_int,
                                       C.POINTER(orc.OrcStats)]
    L.orc_init_scan_result.restype = None
    lim = C.cast(s.chr, C.POINTER(OrcChr))
    out = []
    for ch, pos in chr_pos:
        pt = orc.OrcPt()
        L.orc_init_scan_result(C.byref(pt), int(ch), s.snps, C.byref(lim[int(ch)]), er, int(pos), C.byref(o.stats))
        out.append(wr.Point(pt.nearest_snp, pt.sweep_pos, pt.window_start, pt.window_end, pt.null_logl))
    return out


def test_windows_and_edges(built, tmp):
    """A chromosome above 2 * eval_range + 1 SNPs (window null sums), one below, one of a single SNP."""
    er = 300
    chrs = synth.generate(n_chr=1, chr_len=2_000_000, snps_per_chr=2000, n=16, seed=182, sweeps_per_chr=1, chr_names=["a"])
    chrs += synth.generate(n_chr=1, chr_len=500_000, snps_per_chr=500, n=16, seed=63, chr_names=["b"])
    chrs += synth.generate(n_chr=1, chr_len=50_000, snps_per_chr=1, n=16, seed=170, chr_names=["t"])
    snp = tmp / "win.snp"
    synth.write_snp_file(str(snp), chrs)
    scan, tab = setup(snp)
    s = scan.contents
    lim = [s.chr_limits[c] for c in range(3)]
    assert lim[0].n_snps > 2 * er + 1 >= lim[1].n_snps and lim[2].n_snps == 1
    P = lambda i: s.snps[i].pos  # noqa: E731
    a0, an = lim[0].start_index, lim[0].n_snps
    wide, narrow = -14.0, -4.0
    reqs = [(0, P(a0 + 1000) + 7, wide),             # clipped by the window on both sides
            (0, P(a0 + 1000) + 7, narrow),
            (0, P(a0 + 120) + 3, wide),              # reaches the chromosome's first site; clipped on the right
            (0, P(a0 + an - 90) + 3, wide),          # reaches the last site; clipped on the left
            (0, P(a0 + 700), narrow),                # on a SNP: de-collision
            (0, 0, wide), (0, P(a0 + an - 1) + 5000, wide),
            (1, P(lim[1].start_index + 250) + 1, wide), (1, P(lim[1].start_index + 250), 1.5),
            (2, P(lim[2].start_index) - 40, wide), (2, P(lim[2].start_index), wide), (2, P(lim[2].start_index) + 9, 3.0)]
    hdr, terms = fscl_amd.scan_sites(scan, tab, reqs, er)
    want = oracle_init(snp, [(c, p) for c, p, _ in reqs], er)
    T = wr.OracleTables(snp).tables
    bad = []
    for i, (h, w, r) in enumerate(zip(hdr, want, reqs)):
        pt = point_of(h)
        if (pt.nearest_snp, pt.sweep_pos, pt.window_start, pt.window_end) != \
                (w.nearest_snp, w.sweep_pos, w.window_start, w.window_end) or not wr.same(pt.null_logl, w.null_logl):
            bad.append(f"request {i} {r}: point {pt} != oracle {w}")
        check_walk(h, terms, T, r[2], f"request {i} {r}", bad)
    assert not bad, "\n".join(bad[:12])
    q = hdr["pt"]
    left = q["nearest_snp"] - hdr["nl"] == q["window_start"]
    right = q["nearest_snp"] + hdr["nr"] == q["window_end"]
    first, last = a0, a0 + an - 1
    assert (left & (q["window_start"] > first) & (q["chr"] == 0)).any(), "no walk clipped by window_start"
    assert (right & (q["window_end"] < last) & (q["chr"] == 0)).any(), "no walk clipped by window_end"
    assert (left & (q["window_start"] == first) & (q["chr"] == 0)).any(), "no walk reaches the first site"
    assert (right & (q["window_end"] == last) & (q["chr"] == 0)).any(), "no walk reaches the last site"
    assert int(q["sweep_pos"][4]) == reqs[4][1] + 1, "no de-collision"
    assert hdr["len"][9:].max() <= 1 and (q["n_snps"][9:] == 1).all()
    assert (q["n_snps"][:7] == 2 * er + 1).all() and (q["n_snps"][7:9] == lim[1].n_snps).all()


# ------------------------------------------------------------------ the whole path
G_JOB, g_JOB = 50000, 5000


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """One 600 kb chromosome, 1 500 SNPs, one planted sweep (the curve tests' job)."""
    d = tmp_path_factory.mktemp("sitesjob")
    snp = d / "job.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=1, chr_len=600_000, snps_per_chr=1500, n=20, seed=7,
                                                   sweeps_per_chr=1))
    return dict(dir=d, snp=snp)


def parse_sites_file(path):
    """[(sweep_pos, [site row fields], summary fields)] per walk."""
    out = [(None, [], None)]
    for line in path.read_text().splitlines():
        f = line.split("\t")
        if f[2] == "summary":
            out[-1] = (int(f[1]), out[-1][1], f[3:])
            out.append((None, [], None))
        else:
            out[-1][1].append(f)
    assert out.pop() == (None, [], None)
    return out


def starred_clr(path):
    """sweep_pos -> the statistic text of the starred row of an --alpha-file."""
    return {int(f[1]): f[3] for f in (ln.split("\t") for ln in path.read_text().splitlines()) if f[-1] == "*"}


@pytest.mark.parametrize("mode", ["bisection", "grid"])
def test_whole_path(built, job, mode):
    d = job["dir"]
    kw = dict(large_grid_sp=G_JOB, small_grid_sp=g_JOB, scan_mode=mode, n_permute=5)
    s0 = fscl_amd.run(job["snp"], d / f"o0_{mode}.txt", **kw)
    p0 = fscl_amd.points(s0).tobytes()
    s1 = fscl_amd.run(job["snp"], d / f"o1_{mode}.txt", sites_file=d / f"s_{mode}.txt", sites_top=0,
                      alpha_file=d / f"a_{mode}.txt", profile_file=d / f"p_{mode}.txt", **kw)
    assert fscl_amd.points(s1).tobytes() == p0, "the permutation test's stream was disturbed"
    assert (d / f"o0_{mode}.txt").read_bytes() == (d / f"o1_{mode}.txt").read_bytes()
    scan, tab = setup(job["snp"])
    if mode == "grid":
        fscl_amd.scan_chromosome_grid(scan, tab, small_grid_sp=g_JOB, large_grid_sp=G_JOB)
    else:
        fscl_amd.scan_chromosome(scan, tab, large_grid_sp=G_JOB)
    pts = fscl_amd.points(scan)
    hdr, terms = fscl_amd.scan_point_sites(scan, tab, top=0)
    assert len(hdr) == len(pts) == 12 and fscl_amd.sites_last_ms() > 0.0
    for h, p in zip(hdr, pts):
        for f in ("chr", "nearest_snp", "sweep_pos", "n_snps", "window_start", "window_end", "null_logl", "lalpha",
                  "sm_logl", "clr"):
            assert h["pt"][f].tobytes() == p[f].tobytes(), f
    fscl_amd.sites_output(d / f"t_{mode}.txt", scan, hdr, terms)
    assert (d / f"s_{mode}.txt").read_bytes() == (d / f"t_{mode}.txt").read_bytes()
    walks = parse_sites_file(d / f"s_{mode}.txt")
    summ = fscl_amd.sites_summary(scan, hdr, terms)
    star = starred_clr(d / f"a_{mode}.txt")
    assert len(walks) == 12
    s = scan.contents
    for (pos, rows, sm), h, u in zip(walks, hdr, summ):
        assert pos == int(h["pt"]["sweep_pos"]) and len(rows) == int(h["len"]) == int(sm[0]) == int(u["n_sites"])
        near, nl = int(h["pt"]["nearest_snp"]), int(h["nl"])
        t = terms[int(h["off"]):int(h["off"]) + int(h["len"])]
        for j, f in enumerate(rows):  # ascending position: site near - nl + j holds term k
            i = near - nl + j
            k = 0 if i == near else (near - i if i < near else nl + i - near)
            assert int(f[2]) == s.snps[i].pos and int(f[3]) == s.snps[i].pos - pos and f[8] == "%1.4f" % t[k]
        assert int(h["len"]) > 0  # (every point of this job has a footprint: no NA column)
        assert [int(x) for x in sm[1:6]] == [int(u[f]) for f in ("first_pos", "last_pos", "n_pos", "n_neg", "top_pos")]
        assert sm[6] == "%1.4f" % u["top_term"] and int(sm[8]) == int(u["n_half"])
        assert sm[7] == ("NA" if math.isnan(u["top_share"]) else "%1.4f" % u["top_share"])
        assert star[pos] == "%1.2f" % (2.0 * (fold(float(h["pt"]["null_logl"]), t) - float(h["pt"]["null_logl"])))
    # the default takes the ten points of greatest CLR, listed in scan order
    top, _ = fscl_amd.scan_point_sites(scan, tab)
    order = sorted(sorted(range(12), key=lambda i: (-float(pts["clr"][i]), i))[:10])
    assert top["pt"]["sweep_pos"].tolist() == [int(pts["sweep_pos"][i]) for i in order]
    job[mode] = (d / f"s_{mode}.txt").read_bytes()


def test_two_devices_give_the_same_file(built, job):
    d = job["dir"]
    fscl_amd.set_devices([0, 0])
    try:
        fscl_amd.run(job["snp"], None, large_grid_sp=G_JOB, sites_file=d / "two.txt", sites_top=0)
        assert fscl_amd.get_lib().fscl_amd_n_devices() == 2
    finally:
        fscl_amd.set_device(0)
    fscl_amd.run(job["snp"], None, large_grid_sp=G_JOB, sites_file=d / "one.txt", sites_top=0)
    assert (d / "two.txt").read_bytes() == (d / "one.txt").read_bytes()
    if "bisection" in job:
        assert job["bisection"] == (d / "one.txt").read_bytes()


def test_cli(built, job, tmp):
    base = [str(CLI), "-f", str(job["snp"]), "-G", str(G_JOB), "-g", str(g_JOB)]
    r = subprocess.run(base + ["-o", str(tmp / "o.txt"), f"--sites-file={tmp / 's.txt'}", "--sites-top=3",
                               f"--alpha-file={tmp / 'a.txt'}", "--n-permute=5", "--prepend-label=L"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Site terms: 3 walks" in r.stderr + r.stdout
    fscl_amd.run(job["snp"], tmp / "ref.txt", large_grid_sp=G_JOB, n_permute=5, sites_file=tmp / "ref_s.txt", sites_top=3,
                 alpha_file=tmp / "ref_a.txt", label="L")
    assert (tmp / "o.txt").read_bytes() == (tmp / "ref.txt").read_bytes()
    assert (tmp / "s.txt").read_bytes() == (tmp / "ref_s.txt").read_bytes()
    assert (tmp / "a.txt").read_bytes() == (tmp / "ref_a.txt").read_bytes()
    assert all(ln.startswith("L\t") for ln in (tmp / "s.txt").read_text().splitlines())
