"""The submit / wait protocol of the device shim's batches (include/fsclg.h), for the nine kinds of call
beside the search: profile, cell maxima, curves, site terms, sample, tail fit, surface, conditional scan and
block sums.

What a batch holds between a submit and its wait, which error a misplaced call gets and whether it leaves the
batch submitted, each kind's kernel time, the slot's user count and the reuse of a batch's buffers: every check
is an error code or an equality of bytes between two runs of one request.  What the kernels compute is checked
by the kinds' own test files.

The data is the golden set g1 with its tables; a request is one run of 3 positions (2 alphas, 2 blocks), 2 site
requests, or 2 tail points of 8 samples.  The sampler draws every site of g1 with one sweep (it has no smaller
request, and no empty one).
"""
from __future__ import annotations

import ctypes as C
import types

import numpy as np
import pytest

import fscl_amd
import walk_ref as wr
from util import GOLD

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE = 0, -1, -3
ER = 81920
N_BATCH = 10            # FSCLG_N_BATCHES
NULL_SUM = -123.25      # every chromosome's whole-chromosome null sum
SENTINEL = 0xA5
RAW = fscl_amd._POINT_RAW
LAS = [-6.0, -3.0]
vp = C.c_void_p


class BlkT(C.Structure):  # fsclg_blocks_t
    _fields_ = [("block_bp", C.c_int32), ("b0", C.c_int32), ("nb", C.c_int32), ("pad", C.c_int32)]


def sentinel(n, dtype):
    a = np.zeros(max(n, 1), dtype=dtype)
    a.view(np.uint8)[:] = SENTINEL
    return a


def untouched(*arrays):
    return all((a.view(np.uint8) == SENTINEL).all() for a in arrays)


# ------------------------------------------------------------------ the data and a context
class Data:
    def __init__(self):
        ot = wr.OracleTables(GOLD / "g1.snp")
        s = ot.o.s.contents
        lim = C.cast(s.chr, C.POINTER(wr.OrcChr))
        self.tables = ot.tables
        self.chr_start = [lim[c].start_index for c in range(s.n_chr)]
        self.chr_n = [lim[c].n_snps for c in range(s.n_chr)]
        self.n_snps = len(ot.tables.pos)
        self.pos = ot.tables.pos
        # the sampler's own tables: one depth of sample size 4, every coefficient 0 (a site under the sweep draws
        # each count with probability exp(0)), on the knot grid of the scan's tables
        self.n_iv = ot.tables.coef.shape[1]
        self.smp_coef = np.zeros(self.n_iv * 3 * 4)
        self.smp_neutral = np.array([0.5, 0.3, 0.2])
        self.smp_depth_n = np.array([4], dtype=np.int32)


@pytest.fixture(scope="module")
def data(built):
    return Data()


class Ctx(wr.Shim):
    """A context with g1 uploaded, the sampler's tables set and every slot's null sums given."""

    def __init__(self, d: Data):
        super().__init__()
        L = self.L
        run, i32 = C.POINTER(wr.RunT), C.c_int
        for name, res, args in (
                ("fsclg_profile_submit", i32, [vp, run, i32, i32]), ("fsclg_profile_wait", i32, [vp, vp]),
                ("fsclg_cellmax_submit", i32, [vp, i32, i32, run, i32, i32]), ("fsclg_cellmax_wait", i32, [vp, i32, vp]),
                ("fsclg_curve_submit", i32, [vp, i32, i32, run, i32, i32]), ("fsclg_curve_wait", i32, [vp, i32, vp]),
                ("fsclg_sites_submit", i32, [vp, i32, i32, vp, i32, i32]),
                ("fsclg_sites_wait", i32, [vp, i32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
                ("fsclg_sample_tables", i32, [vp, vp, vp, vp, i32, i32, C.c_double]),
                ("fsclg_sample_submit", i32, [vp, i32, vp, vp, i32, C.c_ulonglong, i32]),
                ("fsclg_sample_wait", i32, [vp, i32, vp, C.POINTER(C.c_ulonglong)]),
                ("fsclg_tail_submit", i32, [vp, i32, vp, C.c_size_t, vp, vp, vp, i32, i32, i32]),
                ("fsclg_tail_wait", i32, [vp, i32, vp]),
                ("fsclg_surface_submit", i32, [vp, i32, i32, run, i32, vp, i32, i32]),
                ("fsclg_surface_wait", i32, [vp, i32, vp, vp]),
                ("fsclg_cond_submit", i32, [vp, i32, i32, run, i32, vp, i32, vp, i32]),
                ("fsclg_cond_wait", i32, [vp, i32, vp, vp]),
                ("fsclg_blocks_submit", i32, [vp, i32, i32, run, i32, vp, i32, C.POINTER(BlkT), i32]),
                ("fsclg_blocks_wait", i32, [vp, i32, vp, vp, vp]),
                ("fsclg_slot_set_rows", i32, [vp, i32, vp, vp]),
                ("fsclg_profile_last_ms", C.c_double, [vp])):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
        for k in ("cellmax", "curve", "sites", "sample", "tail", "surface", "cond", "blocks"):
            f = getattr(L, f"fsclg_{k}_last_ms")
            f.restype, f.argtypes = C.c_double, [vp, C.c_int]
        self.d = d
        self.upload(d.tables, d.chr_start, d.chr_n)
        self._ok(L.fsclg_sample_tables(self.ctx, d.smp_coef.ctypes.data, d.smp_neutral.ctypes.data,
                                       d.smp_depth_n.ctypes.data, 1, d.n_iv, d.tables.step), "fsclg_sample_tables")
        self.set_chr_null(NULL_SUM, len(d.chr_n))
        for slot in (0, 1):
            self._ok(self.set_rows(slot), "fsclg_slot_set_rows")

    def set_rows(self, slot):
        """The uploaded rows and the null sums into the slot: FSCLG_E_STATE while a batch uses the slot."""
        nul = (C.c_double * len(self.d.chr_n))(*([NULL_SUM] * len(self.d.chr_n)))
        return self.L.fsclg_slot_set_rows(self.ctx, slot, None, nul)


@pytest.fixture(scope="module")
def ctx(data):
    s = Ctx(data)
    yield s
    s.close()


# ------------------------------------------------------------------ the nine kinds
def runs_of(d: Data, size):
    """(chr, start_pos, step, count) runs on chromosome 0: one run of 3 positions; or 1100 runs of 2, more
    runs, chunks and positions than the 1024 elements a buffer starts with; or none."""
    p0, p1 = int(d.pos[d.chr_start[0]]), int(d.pos[d.chr_start[0] + d.chr_n[0] - 1])
    if size == "small":
        return [(0, (p0 + p1) // 2, 1000, 3)]
    if size == "big":
        return [(0, p0 + (k * (p1 - p0 - 10)) // 1100, 7, 2) for k in range(1100)]
    return []


def run_array(runs):
    return (wr.RunT * max(len(runs), 1))(*[wr.RunT(*r) for r in runs])


class Kind:
    """One kind of call: submit(ctx, batch, slot, size) -> code; wait(ctx, batch, size, null=False) -> (code,
    the outputs as bytes, the output arrays); bad(ctx, batch, slot) -> the code of a submit whose argument fails a
    check after the batch's state has been looked at."""
    name = ""
    has_empty = True

    def last_ms(self, s: Ctx, batch):
        return getattr(s.L, f"fsclg_{self.name}_last_ms")(s.ctx, batch)

    def total(self, s, size):
        return sum(r[3] for r in runs_of(s.d, size))

    def outputs(self, s, size):
        raise NotImplementedError

    def call_wait(self, s, batch, ptrs):
        raise NotImplementedError

    def wait(self, s, batch, size, null=False):
        out = self.outputs(s, size)
        r = self.call_wait(s, batch, [None] * len(out) if null else [a.ctypes.data for a in out])
        return r, b"".join(a.tobytes() for a in out), out


class RunKind(Kind):
    def submit(self, s, batch, slot, size, runs=None):
        runs = runs_of(s.d, size) if runs is None else runs
        return getattr(s.L, f"fsclg_{self.name}_submit")(s.ctx, batch, slot, run_array(runs), len(runs), ER)

    def bad(self, s, batch, slot):
        return self.submit(s, batch, slot, None, [(0, 5000, 0, 3)])  # step 0

    def call_wait(self, s, batch, ptrs):
        return getattr(s.L, f"fsclg_{self.name}_wait")(s.ctx, batch, *ptrs)


class Profile(RunKind):
    name = "profile"  # batch 0 and slot 0 always

    def submit(self, s, batch, slot, size, runs=None):
        runs = runs_of(s.d, size) if runs is None else runs
        return s.L.fsclg_profile_submit(s.ctx, run_array(runs), len(runs), ER)

    def call_wait(self, s, batch, ptrs):
        return s.L.fsclg_profile_wait(s.ctx, *ptrs)

    def last_ms(self, s, batch):
        return s.L.fsclg_profile_last_ms(s.ctx)

    def outputs(self, s, size):
        return [sentinel(self.total(s, size), RAW)]


class Cellmax(RunKind):
    name = "cellmax"

    def outputs(self, s, size):
        return [sentinel(len(runs_of(s.d, size)), RAW)]


class Curve(RunKind):
    name = "curve"

    def outputs(self, s, size):
        return [sentinel(self.total(s, size), fscl_amd.CURVE_DTYPE)]


class Surface(RunKind):
    name = "surface"

    def la(self, runs):
        return np.ascontiguousarray([LAS] * max(len(runs), 1), dtype=np.float64)

    def submit(self, s, batch, slot, size, runs=None):
        runs = runs_of(s.d, size) if runs is None else runs
        la = self.la(runs)
        return s.L.fsclg_surface_submit(s.ctx, batch, slot, run_array(runs), len(runs), la.ctypes.data, 2, ER)

    def outputs(self, s, size):
        n = self.total(s, size)
        return [sentinel(n, RAW), sentinel(2 * n, np.float64)]


class Cond(Surface):
    name = "cond"

    def submit(self, s, batch, slot, size, runs=None):
        runs = runs_of(s.d, size) if runs is None else runs
        n = sum(r[3] for r in runs)
        clip = np.ascontiguousarray([(k % 7, s.d.n_snps - 1 - k % 5) for k in range(max(n, 1))], dtype=np.int32)
        la = self.la(runs)
        return s.L.fsclg_cond_submit(s.ctx, batch, slot, run_array(runs), len(runs), la.ctypes.data, 2,
                                     clip.ctypes.data, ER)


class Blocks(Surface):
    name = "blocks"

    def submit(self, s, batch, slot, size, runs=None):
        runs = runs_of(s.d, size) if runs is None else runs
        mid = (int(s.d.pos[0]) + int(s.d.pos[s.d.chr_n[0] - 1])) // 2
        blk = (BlkT * max(len(runs), 1))(*[BlkT(mid, 0, 2, 0) for _ in runs])  # two blocks, cut at the middle
        la = self.la(runs)
        return s.L.fsclg_blocks_submit(s.ctx, batch, slot, run_array(runs), len(runs), la.ctypes.data, 2, blk, ER)

    def outputs(self, s, size):
        n = self.total(s, size)
        return [sentinel(n, RAW), sentinel(n * 2 * 2, np.float64), sentinel(n * 2 * 2, np.uint32)]


class Sites(Kind):
    name = "sites"

    def requests(self, s, size):
        runs = runs_of(s.d, size)
        return [(c, p + j * st, LAS[(i + j) % 2]) for i, (c, p, st, n) in enumerate(runs) for j in range(n)][:2 if size == "small" else None]

    def submit(self, s, batch, slot, size, reqs=None):
        reqs = self.requests(s, size) if reqs is None else reqs
        a = np.zeros(max(len(reqs), 1), dtype=fscl_amd.SITE_REQ_DTYPE)
        for q, r in zip(a, reqs):
            q["chr"], q["pos"], q["lalpha"] = r
        return s.L.fsclg_sites_submit(s.ctx, batch, slot, a.ctypes.data, len(reqs), ER)

    def bad(self, s, batch, slot):
        return self.submit(s, batch, slot, None, [(0, 5000, float("nan"))])

    def wait(self, s, batch, size, null=False):
        n = len(self.requests(s, size))
        hdr, nt = sentinel(n, fscl_amd.SITES_DTYPE), C.c_size_t(0)
        if null:
            return s.L.fsclg_sites_wait(s.ctx, batch, None, None, 0, None), b"", [hdr]
        # a wait that only sizes the buffer leaves the batch submitted (include/fsclg.h)
        r = s.L.fsclg_sites_wait(s.ctx, batch, hdr.ctypes.data, None, 0, C.byref(nt))
        if n == 0 or r == E_STATE or (r == OK and nt.value == 0):
            return r, hdr.tobytes(), [hdr]
        assert r == E_ARG and nt.value > 0 and untouched(hdr)
        terms = sentinel(nt.value, np.float64)
        r = s.L.fsclg_sites_wait(s.ctx, batch, hdr.ctypes.data, terms.ctypes.data, nt.value, None)
        return r, hdr.tobytes() + terms.tobytes(), [hdr, terms]


class Sample(Kind):
    name = "sample"
    has_empty = False

    def submit(self, s, batch, slot, size, sweeps=None):
        if sweeps is None:  # one sweep; or 1100, above the 1024 a buffer starts with
            p0 = int(s.d.pos[0])
            sweeps = [(0, p0 + 50000, -9.0)] if size == "small" else [(0, p0 + 97 * k, -9.0 - (k % 3)) for k in range(1100)]
        a = np.zeros(max(len(sweeps), 1), dtype=fscl_amd.SITE_REQ_DTYPE)  # fsclg_sweep_t has the same layout
        for q, r in zip(a, sweeps):
            q["chr"], q["pos"], q["lalpha"] = r
        depth = np.zeros(s.d.n_snps, dtype=np.int32)
        return s.L.fsclg_sample_submit(s.ctx, batch, depth.ctypes.data, a.ctypes.data, len(sweeps), 12345, 3)

    def bad(self, s, batch, slot):
        return self.submit(s, batch, slot, None, [(99, 5000, -9.0)])  # no such chromosome

    def wait(self, s, batch, size, null=False):
        f, deg = sentinel(s.d.n_snps, np.int32), C.c_ulonglong(0)
        r = s.L.fsclg_sample_wait(s.ctx, batch, None if null else f.ctypes.data, C.byref(deg))
        return r, f.tobytes(), [f]


class Tail(Kind):
    name = "tail"

    def points(self, size):
        return {"small": 2, "big": 1100}.get(size, 0)

    def submit(self, s, batch, slot, size, counts=None):
        n = self.points(size)
        rng = np.random.default_rng(11)
        x = (rng.chisquare(2, 8 * max(n, 1)) + 3.0).astype(np.float32)
        off = np.arange(max(n, 1), dtype=np.uint64) * 8
        cnt = np.full(max(n, 1), 8, dtype=np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
        x0 = np.full(max(n, 1), 20.0)
        n = n if counts is None else len(counts)
        return s.L.fsclg_tail_submit(s.ctx, batch, x.ctypes.data, 8 * n, off.ctypes.data, cnt.ctypes.data,
                                     x0.ctypes.data, n, 2, 4)

    def bad(self, s, batch, slot):
        return self.submit(s, batch, slot, "small", counts=[8, -1])

    def outputs(self, s, size):
        return [sentinel(self.points(size), fscl_amd.TAIL_DTYPE)]

    def call_wait(self, s, batch, ptrs):
        return s.L.fsclg_tail_wait(s.ctx, batch, *ptrs)


KINDS = [Profile(), Cellmax(), Curve(), Sites(), Sample(), Tail(), Surface(), Cond(), Blocks()]
NAMES = [k.name for k in KINDS]
BY_NAME = {k.name: k for k in KINDS}


def other_kind(k: Kind) -> Kind:
    return KINDS[(KINDS.index(k) + 1) % len(KINDS)]


def call(s: Ctx, k: Kind, batch, slot, size):
    """One submit and its wait, both OK: the outputs' bytes."""
    s._ok(k.submit(s, batch, slot, size), f"fsclg_{k.name}_submit")
    r, got, out = k.wait(s, batch, size)
    s._ok(r, f"fsclg_{k.name}_wait")
    assert size == "empty" or not untouched(*out), f"{k.name}: the wait wrote nothing"
    return got


def all_ms(s: Ctx, batch):
    return [k.last_ms(s, batch) for k in KINDS]


@pytest.fixture(scope="module")
def want(ctx):
    """Every kind's small request on the module's context (batch 0, slot 0), computed once."""
    return {k.name: call(ctx, k, 0, 0, "small") for k in KINDS}


def batch_is_free(s: Ctx, k: Kind, batch, slot, want):
    """A call on the batch runs and gives the known bytes, and the slot has no user left."""
    assert call(s, k, batch, slot, "small") == want[k.name]
    assert s.set_rows(slot) == OK, s.L.fsclg_last_error().decode()


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", NAMES)
def test_nothing_submitted(ctx, want, name):
    k = BY_NAME[name]
    r, _, out = k.wait(ctx, 0, "small")
    assert r == E_STATE and untouched(*out)
    r, _, _ = k.wait(ctx, 0, "small", null=True)
    assert r == E_STATE


@pytest.mark.parametrize("name", NAMES)
def test_wrong_kind(ctx, want, name):
    """Kind A submitted; the next kind's wait on the batch is rejected, writes nothing and leaves A pending."""
    a = BY_NAME[name]
    b = other_kind(a)
    ctx._ok(a.submit(ctx, 0, 0, "small"), "submit")
    r, _, out = b.wait(ctx, 0, "small")
    assert r == E_STATE and untouched(*out), f"{b.name}'s wait on a batch that holds {a.name}"
    r, got, _ = a.wait(ctx, 0, "small")
    assert r == OK and got == want[name]
    batch_is_free(ctx, b, 0, 0, want)


@pytest.mark.parametrize("name", NAMES)
def test_double_submit(ctx, want, name):
    a = BY_NAME[name]
    ctx._ok(a.submit(ctx, 0, 0, "small"), "submit")
    for k in (a, other_kind(a), BY_NAME["tail"], BY_NAME["sample"]):
        assert k.submit(ctx, 0, 1, "big" if k is a else "small") == E_STATE, f"{k.name} submitted on a pending batch"
    r, got, _ = a.wait(ctx, 0, "small")
    assert r == OK and got == want[name]
    assert ctx.set_rows(0) == OK and ctx.set_rows(1) == OK, "a rejected submit left a user on a slot"


@pytest.mark.parametrize("name", NAMES)
def test_null_outputs(ctx, want, name):
    """A wait without outputs is FSCLG_E_ARG and the batch stays submitted; the proper wait then gives the bytes
    of a fresh call of the same request on another batch."""
    k = BY_NAME[name]
    batch = 0 if name == "profile" else 4
    ctx._ok(k.submit(ctx, batch, 0, "small"), "submit")
    for _ in range(2):
        r, _, _ = k.wait(ctx, batch, "small", null=True)
        assert r == E_ARG
    assert ctx.set_rows(0) == E_STATE or name in ("sample", "tail"), "the slot lost its user"
    r, got, _ = k.wait(ctx, batch, "small")
    assert r == OK
    assert got == call(ctx, k, 0 if name == "profile" else 7, 1, "small") == want[name]
    assert ctx.set_rows(0) == OK


@pytest.mark.parametrize("name", [k.name for k in KINDS if k.has_empty])
def test_empty_call(ctx, want, name):
    k = BY_NAME[name]
    call(ctx, k, 0, 0, "small")
    assert k.last_ms(ctx, 0) > 0.0
    ctx._ok(k.submit(ctx, 0, 0, "empty"), "submit of nothing")
    assert ctx.set_rows(0) == E_STATE or name == "tail", "an empty call holds its slot like any other"
    r, _, out = k.wait(ctx, 0, "empty", null=True)
    assert r == OK, ctx.L.fsclg_last_error().decode()
    ms = k.last_ms(ctx, 0)
    print(f"{name}: last_ms of an empty call {ms!r}")
    if name == "tail":
        # the tail call brackets its launch with the events whether or not it has a point, and its wait reads
        # them: its time is that of an empty bracket, two event records one after the other on an idle stream
        # (0.005 ms measured; the events' resolution is 0.001 ms or finer), not 0.0
        assert 0.0 <= ms < 0.05
    else:
        assert ms == 0.0
    r, _, _ = k.wait(ctx, 0, "empty")
    assert r == E_STATE, "an empty call's wait ends it"
    batch_is_free(ctx, k, 0, 0, want)


@pytest.mark.parametrize("name", NAMES)
def test_times(ctx, want, name):
    """A submit zeroes its own kind's time on its batch, the wait sets it; no other kind's and no other batch's
    time moves."""
    k = BY_NAME[name]
    b, o = 0, 5
    for q in KINDS:  # every kind has a time on both batches (the profile's is the context's)
        for batch in (b, o):
            call(ctx, q, batch, 0, "small")
    before, before_o = all_ms(ctx, b), all_ms(ctx, o)
    assert all(m > 0.0 for m in before + before_o)
    i = KINDS.index(k)
    ctx._ok(k.submit(ctx, b, 0, "small"), "submit")
    now = all_ms(ctx, b)
    assert now[i] == 0.0 and now[:i] + now[i + 1:] == before[:i] + before[i + 1:]
    r, got, _ = k.wait(ctx, b, "small")
    assert r == OK and got == want[name]
    after, after_o = all_ms(ctx, b), all_ms(ctx, o)
    print(f"{name}: last_ms {before[i]!r} -> {after[i]!r}")
    assert after[i] > 0.0
    assert after[:i] + after[i + 1:] == before[:i] + before[i + 1:]
    if name == "profile":  # one time per context
        before_o[i] = after[i]
    assert after_o == before_o
    null = types.SimpleNamespace(L=ctx.L, ctx=None)
    for q in KINDS:  # (the profile's time takes no batch)
        assert q.last_ms(ctx, -1) == 0.0 or q.name == "profile"
        assert q.last_ms(ctx, N_BATCH) == 0.0 or q.name == "profile"
        assert q.last_ms(null, 0) == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_slot_users(ctx, want, name):
    """A submit that fails, on an argument or on a pending batch, adds no user to its slot."""
    k = BY_NAME[name]
    assert k.bad(ctx, 2, 1) == E_ARG
    ctx._ok(k.submit(ctx, 0, 0, "small"), "submit")
    assert k.submit(ctx, 0, 1, "small") == E_STATE
    assert k.bad(ctx, 0, 1) == E_STATE  # (the pending batch is seen before the argument)
    assert ctx.set_rows(1) == OK, "a failed submit left a user on its slot"
    r, got, _ = k.wait(ctx, 0, "small")
    assert r == OK and got == want[name]
    assert call(ctx, k, 0 if name == "profile" else 2, 0 if name == "profile" else 1, "small") == want[name]
    assert ctx.set_rows(0) == OK and ctx.set_rows(1) == OK


@pytest.mark.parametrize("name", NAMES)
def test_buffer_reuse(data, want, name):
    """A small request, one that grows every buffer of the kind past its first 1024 elements, the small one again:
    the bytes of contexts that meet the requests first."""
    k = BY_NAME[name]
    batch, slot = (0, 0) if name == "profile" else (3, 1)
    s, fresh = Ctx(data), Ctx(data)
    try:
        small1 = call(s, k, batch, slot, "small")
        big = call(s, k, batch, slot, "big")
        small2 = call(s, k, batch, slot, "small")
        big_fresh = call(fresh, k, batch, slot, "big")
        small_after = call(fresh, k, batch, slot, "small")
    finally:
        s.close()
        fresh.close()
    assert small1 == want[name] and small2 == want[name] and small_after == want[name]
    assert big == big_fresh and big != small1


def test_open_close(data, want):
    for _ in range(3):
        s = Ctx(data)
        try:
            for k in KINDS:
                batch, slot = (0, 0) if k.name == "profile" else (1 + KINDS.index(k), KINDS.index(k) % 2)
                assert call(s, k, batch, slot, "small") == want[k.name]
        finally:
            s.close()
