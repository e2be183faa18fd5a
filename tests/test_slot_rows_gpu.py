"""The rows a slot holds after each of its four entry points (fsclg_slot_set_rows, _host, _packed, _plan),
read back through sites_kernel and compared by bit pattern with tests/rows_ref.py -- never with another
device result: scatter_rows_kernel at 1-, 2- and 4-byte rows over whole blocks, vector tails and scalar
tails; the whole-chromosome null sums it carries; plan_swap_kernel and the rotation kernels on crafted and
random plans against the sequential element swaps; every refusal, with the slot's rows untouched; and the
window null sums and chunk table of a slot, which must go when its rows change and travel with
fsclg_slot_swap.  The read-back keeps the checks of tests/test_sites_gpu.py's SitesShim: sentinel-filled
buffers, no store past the end, nothing left unwritten.  tests/test_rows_ref.py checks, without a GPU,
that every case is in the regime it is named for.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np
import pytest

import fscl_amd
import rows_ref as rr
import walk_ref as wr

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SENT64 = int.from_bytes(bytes([SENTINEL] * 8), "little")
E_ARG, E_STATE = -1, -3
SWAP_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("len", "<i4"), ("kind", "<i4")])  # fsclg_swap_t
ENT_CAP, GRP_CAP, ROW_CAP = 4096, 4096, rr.BIG_N  # elements of the host buffers


class HostBuf:
    """fsclg_host_alloc memory as a NumPy array, used from offset 0."""

    def __init__(self, L, dtype, count):
        self.L = L
        self.ptr = L.fsclg_host_alloc(np.dtype(dtype).itemsize * count)
        assert self.ptr, "fsclg_host_alloc"
        self.a = np.frombuffer((C.c_char * (np.dtype(dtype).itemsize * count)).from_address(self.ptr), dtype=dtype)

    def free(self):
        self.a = None
        self.L.fsclg_host_free(C.c_void_p(self.ptr))


class RowsShim(wr.Shim):
    """walk_ref.Shim with the row entry points and the sites read-back."""

    def __init__(self):
        super().__init__()
        L, vp, ci = self.L, C.c_void_p, C.c_int
        for name, res, args in (
                ("fsclg_sites_submit", ci, [vp, ci, ci, vp, ci, ci]),
                ("fsclg_sites_wait", ci, [vp, ci, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
                ("fsclg_slot_set_rows", ci, [vp, ci, vp, vp]),
                ("fsclg_slot_set_rows_host", ci, [vp, ci, vp, vp]),
                ("fsclg_slot_set_rows_packed", ci, [vp, ci, vp, ci, vp]),
                ("fsclg_slot_set_rows_plan", ci, [vp, ci, vp, vp, ci, vp]),
                ("fsclg_slot_row_buffer", vp, [vp, ci]),
                ("fsclg_slot_wait", ci, [vp, ci]),
                ("fsclg_slot_swap", ci, [vp, ci, ci]),
                ("fsclg_host_alloc", vp, [C.c_size_t]),
                ("fsclg_host_free", None, [vp])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        L.fsclg_set_chr_null.argtypes = [vp, vp]
        self.h_ent = [HostBuf(L, SWAP_DTYPE, ENT_CAP) for _ in range(2)]
        self.h_grp = [HostBuf(L, np.int32, GRP_CAP) for _ in range(2)]
        self.h_rows = HostBuf(L, np.uint8, 4 * ROW_CAP)
        self.n_rows = self.n = 0
        self.cs = self.cn = None
        self.rows_user = None          # the slot whose last upload reads h_rows
        self.plan_user = [None, None]  # ... h_ent / h_grp [buf]

    def close(self):
        if self.ctx:
            self.L.fsclg_close(self.ctx)  # (idle before the host buffers go)
            self.ctx = C.c_void_p()
            for b in self.h_ent + self.h_grp + [self.h_rows]:
                b.free()

    # ---- uploads
    def upload_tables(self, n_rows):
        if n_rows == self.n_rows:
            return
        coef, nul, lt = rr._identity(n_rows)
        self._ok(self.L.fsclg_upload_tables(self.ctx, wr._pd(lt), wr._pd(coef), n_rows, coef.shape[1], wr._pd(nul),
                                            wr.STEP), "fsclg_upload_tables")
        self.n_rows = n_rows

    def upload_rows(self, n_rows, rows, chr_start=None, chr_n=None):
        """The identity tables of n_rows rows and the sites with these rows."""
        self.upload_tables(n_rows)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        assert int(rows.max()) < n_rows
        n = len(rows)
        if chr_start is None:
            chr_start, chr_n = [0], [n]
        pos = rr.positions(n)
        nc = len(chr_start)
        cs, cn = (C.c_int32 * nc)(*chr_start), (C.c_int32 * nc)(*chr_n)
        self._ok(self.L.fsclg_upload_snps(self.ctx, pos.ctypes.data_as(C.POINTER(C.c_int32)),
                                          rows.ctypes.data_as(C.POINTER(C.c_uint32)), n, cs, cn, nc), "fsclg_upload_snps")
        self.n, self.cs, self.cn = n, list(chr_start), list(chr_n)

    # ---- the entry points (rows below n_rows always: the device does not check _host and _packed)
    def _nul(self, chr_null):
        if chr_null is None:
            return None, None
        a = np.ascontiguousarray(chr_null, dtype=np.float64)
        assert len(a) == len(self.cs)
        return a, a.ctypes.data

    def _checked(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        assert len(rows) == self.n and int(rows.max()) < self.n_rows
        return rows

    def set_copy(self, slot, rows, chr_null=None) -> int:
        keep, p = self._nul(chr_null)
        r = None if rows is None else self._checked(rows)
        return self.L.fsclg_slot_set_rows(self.ctx, slot, None if r is None else r.ctypes.data, p)

    def set_in_place(self, slot, rows, chr_null=None) -> int:
        keep, p = self._nul(chr_null)
        buf = self.L.fsclg_slot_row_buffer(self.ctx, slot)
        assert buf, "fsclg_slot_row_buffer"
        np.frombuffer((C.c_uint32 * self.n).from_address(buf), dtype=np.uint32)[:] = self._checked(rows)
        return self.L.fsclg_slot_set_rows(self.ctx, slot, buf, p)

    def set_packed(self, slot, rows, width, chr_null=None, call="packed") -> int:
        keep, p = self._nul(chr_null)
        r = self._checked(rows)
        dt = rr.WIDTH_DTYPE[width]
        assert int(r.max()) <= np.iinfo(dt).max
        if self.rows_user is not None:  # the buffer stays unchanged until the upload that reads it is done
            self.wait_slot(self.rows_user)
        self.h_rows.a.view(dt)[:self.n] = r.astype(dt)
        self.rows_user = slot
        if call == "host":
            assert width == 4
            return self.L.fsclg_slot_set_rows_host(self.ctx, slot, self.h_rows.ptr, p)
        return self.L.fsclg_slot_set_rows_packed(self.ctx, slot, self.h_rows.ptr, width, p)

    def set_host(self, slot, rows, chr_null=None) -> int:
        return self.set_packed(slot, rows, 4, chr_null, call="host")

    def set_plan(self, slot, ent, grp, chr_null=None, buf=0, n_grp=None, checked=True) -> int:
        """ent / grp None: a NULL pointer.  checked: only plans the restated validator accepts."""
        keep, p = self._nul(chr_null)
        if n_grp is None:
            n_grp = len(grp) - 1
        if checked:
            assert rr.plan_ok(ent, grp, self.n, n_grp), rr.plan_refusal(ent, grp, self.n, n_grp)
        self.fill_plan(buf, ent, grp)
        self.plan_user[buf] = slot
        return self.L.fsclg_slot_set_rows_plan(self.ctx, slot, None if ent is None else self.h_ent[buf].ptr,
                                               None if grp is None else self.h_grp[buf].ptr, n_grp, p)

    def fill_plan(self, buf, ent, grp):
        if self.plan_user[buf] is not None:  # unchanged until the plan that reads them is done
            self.wait_slot(self.plan_user[buf])
            self.plan_user[buf] = None
        if ent:
            assert len(ent) <= ENT_CAP
            self.h_ent[buf].a[:len(ent)] = np.array([tuple(e) for e in ent], dtype=SWAP_DTYPE)
        if grp:
            assert len(grp) <= GRP_CAP
            self.h_grp[buf].a[:len(grp)] = grp

    def wait_slot(self, slot):
        self._ok(self.L.fsclg_slot_wait(self.ctx, slot), "fsclg_slot_wait")

    def set_chr_null_values(self, values):
        a = np.ascontiguousarray(values, dtype=np.float64)
        assert len(a) == len(self.cs)
        self._ok(self.L.fsclg_set_chr_null(self.ctx, a.ctypes.data), "fsclg_set_chr_null")

    # ---- the read-back
    def submit(self, reqs, eval_range, batch, slot) -> int:
        a = np.zeros(max(len(reqs), 1), dtype=fscl_amd.SITE_REQ_DTYPE)
        for q, r in zip(a, reqs):
            q["chr"], q["pos"], q["lalpha"] = r
        return self.L.fsclg_sites_submit(self.ctx, batch, slot, a.ctypes.data, len(reqs), eval_range)

    def wait(self, n, batch):
        hdr = np.zeros(n, dtype=fscl_amd.SITES_DTYPE)
        hdr.view(np.uint8)[:] = SENTINEL
        nt = C.c_size_t(12345)
        r = self.L.fsclg_sites_wait(self.ctx, batch, hdr.ctypes.data, None, 0, C.byref(nt))
        if r != E_ARG:
            self._ok(r, "fsclg_sites_wait")
            raise AssertionError("the sizing wait found no term")
        assert (hdr.view(np.uint8) == SENTINEL).all(), "a wait that only sizes wrote headers"
        buf = np.full(nt.value + 16, SENT64, dtype=np.uint64)
        nt2 = C.c_size_t(0)
        self._ok(self.L.fsclg_sites_wait(self.ctx, batch, hdr.ctypes.data, buf.ctypes.data, nt.value, C.byref(nt2)),
                 "fsclg_sites_wait")
        assert nt2.value == nt.value
        terms, tail = buf[:nt.value], buf[nt.value:]
        words = hdr.view(np.uint8).view(np.uint32)
        assert not (words == int.from_bytes(bytes([SENTINEL] * 4), "little")).any(), "a header was left unwritten"
        assert not (terms == SENT64).any(), "a term was left unwritten"
        assert (tail == SENT64).all(), "a store past the terms"
        assert hdr["off"].tolist() == (np.cumsum(hdr["len"]) - hdr["len"]).tolist()
        return hdr, terms.view(np.float64)

    def sites(self, reqs, eval_range, slot, batch=None):
        batch = (2 + slot) % 10 if batch is None else batch
        self._ok(self.submit(reqs, eval_range, batch, slot), "fsclg_sites_submit")
        return self.wait(len(reqs), batch)

    def read(self, slot):
        """(the slot's rows in site order, the requests' null_logl per chromosome)."""
        hdr, terms = self.sites(rr.requests(self.cs), rr.READ_ER, slot)
        out = []
        for h, a, m in zip(hdr, self.cs, self.cn):
            q = h["pt"]
            assert (int(q["nearest_snp"]), int(q["window_start"]), int(q["window_end"]), int(q["n_snps"])) == \
                (a, a, a + m - 1, m), f"chromosome at {a}: point {q}"
            assert int(h["pad"]) == 0 and wr.same(float(q["lalpha"]), rr.LALPHA)
            t = terms[int(h["off"]):int(h["off"]) + int(h["len"])]
            out.append(rr.rows_of_terms(a, int(h["nl"]), int(h["nr"]), a, a + m - 1, t))
        return np.concatenate(out), hdr["pt"]["null_logl"].copy()


@pytest.fixture(scope="module")
def shim(built):
    s = RowsShim()
    saved = os.environ.get("FSCLG_WINDOW_CHUNK")
    yield s
    s.close()
    os.environ.pop("FSCLG_WINDOW_CHUNK", None) if saved is None else os.environ.__setitem__("FSCLG_WINDOW_CHUNK", saved)


def device(what, fn):
    """fn(); a device error ends the session: nothing more runs on the GPU."""
    t0 = time.perf_counter()
    try:
        out = fn()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)
    print(f"TIME {what}: {time.perf_counter() - t0:.2f} s")
    return out


def diff(got, want, what) -> list:
    """[] or one line on the first site where the rows differ."""
    if got.tobytes() == want.tobytes():
        return []
    if len(got) != len(want):
        return [f"{what}: {len(got)} rows != {len(want)}"]
    k = np.flatnonzero(got != want)
    return [f"{what}: {len(k)} sites differ, the first {int(k[0])}: {int(got[k[0]])} != {int(want[k[0]])}, "
            f"the last {int(k[-1])}"]


# ------------------------------------------------------------------ scatter
@pytest.mark.parametrize("width", [1, 2, 4])
def test_scatter(shim, width):
    n_rows = rr.WIDTH_ROWS[width]

    def run():
        bad = []
        for n in rr.SCATTER_N:
            A = rr.base_rows(n, n_rows, seed=n)
            B = rr.scatter_rows(width, n)
            shim.upload_rows(n_rows, A, *rr.even_chromosomes(n, 1500))
            slot = 1 + n % 7
            shim._ok(shim.set_packed(slot, B, width), "fsclg_slot_set_rows_packed")
            bad += diff(shim.read(slot)[0], B, f"width {width}, n {n}, packed into slot {slot}")
            if width == 4:
                for k, (name, call) in enumerate((("copy", shim.set_copy), ("host", shim.set_host),
                                                  ("in place", shim.set_in_place))):
                    Bk = rr.scatter_rows(4, n, seed=k + 1)
                    s2 = 1 + (slot + k) % 7
                    shim._ok(call(s2, Bk), name)
                    bad += diff(shim.read(s2)[0], Bk, f"n {n}, {name} into slot {s2}")
            bad += diff(shim.read(0)[0], A, f"width {width}, n {n}, slot 0")
        return bad
    bad = device(f"scatter width {width}", run)
    assert not bad, "\n".join(bad[:12])


def test_uploaded_rows_come_back(shim):
    """row == NULL and an empty plan put the uploaded rows over a slot that held other rows."""
    n, n_rows = 3589, 70000
    A, B = rr.base_rows(n, n_rows), rr.scatter_rows(4, n)

    def run():
        bad = []
        shim.upload_rows(n_rows, A, *rr.even_chromosomes(n, 1500))
        for slot, restore in ((2, lambda s: shim.set_copy(s, None)),
                              (5, lambda s: shim.set_plan(s, [], [0])),
                              (6, lambda s: shim.set_plan(s, None, None, n_grp=0))):
            shim._ok(shim.set_host(slot, B), "fsclg_slot_set_rows_host")
            bad += diff(shim.read(slot)[0], B, f"slot {slot} before")
            shim._ok(restore(slot), "restore")
            bad += diff(shim.read(slot)[0], A, f"slot {slot} restored")
        return bad
    bad = device("uploaded rows", run)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ null sums through the scatter
def test_chr_null_through_every_entry_point(shim):
    nc, per = 130, 3  # more chromosomes than one wave's lanes
    n, n_rows = nc * per, 256
    A = rr.base_rows(n, n_rows)
    cs, cn = rr.even_chromosomes(n, per)
    val = lambda k: -(1000.0 * k + np.arange(nc) + 0.375)  # noqa: E731
    plan = rr.one_group_each([(1, 200, 50, 0)])
    calls = {1: ("copy", lambda s, v: shim.set_copy(s, rr.scatter_rows(1, n, 1), v)),
             2: ("host", lambda s, v: shim.set_host(s, rr.scatter_rows(1, n, 2), v)),
             3: ("packed", lambda s, v: shim.set_packed(s, rr.scatter_rows(1, n, 3), 1, v)),
             4: ("plan", lambda s, v: shim.set_plan(s, *plan, chr_null=v)),
             5: ("uploaded", lambda s, v: shim.set_copy(s, None, v))}

    def run():
        bad = []

        def check(slot, want, what):
            got = shim.read(slot)[1]
            if got.tobytes() != want.tobytes():
                k = int(np.flatnonzero(got.view(np.int64) != want.view(np.int64))[0])
                bad.append(f"{what}: chromosome {k}: null_logl {got[k]!r} != {want[k]!r}")
        assert len(cs) == nc
        shim.upload_rows(n_rows, A, cs, cn)
        shim.set_chr_null_values(val(9))
        for slot, (name, call) in calls.items():
            shim._ok(call(slot, val(slot)), name)
        for slot, (name, call) in calls.items():
            check(slot, val(slot), f"{name}, slot {slot}")
        check(0, val(9), "slot 0")
        for slot, (name, call) in calls.items():  # NULL: the slot's earlier values stay
            shim._ok(call(slot, None), name)
            check(slot, val(slot), f"{name} with NULL sums, slot {slot}")
        shim.set_chr_null_values(val(7))           # slot 0 alone
        check(0, val(7), "slot 0 after fsclg_set_chr_null")
        for slot, (name, _) in calls.items():
            check(slot, val(slot), f"slot {slot} after fsclg_set_chr_null")
        bad += diff(shim.read(4)[0], rr.apply_plan(A, *plan), "plan rows")
        return bad
    bad = device("null sums", run)
    assert not bad, "\n".join(bad[:12])


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_rows(shim):
    n = rr.PLAN_N
    A = rr.base_rows(n, 256, seed=3)
    B = rr.base_rows(n, 256, seed=4)
    L = shim.L

    def run():
        shim.upload_rows(257, A)
        slot = 3
        shim._ok(shim.set_host(slot, B), "fsclg_slot_set_rows_host")
        shim.wait_slot(slot)
        hp = shim.h_rows.ptr
        got = {}
        got["width 1 with 257 table rows"] = L.fsclg_slot_set_rows_packed(shim.ctx, slot, hp, 1, None)
        shim.upload_tables(65537)
        got["width 2 with 65537 table rows"] = L.fsclg_slot_set_rows_packed(shim.ctx, slot, hp, 2, None)
        for w in (3, 0, 8, -1):
            got[f"width {w}"] = L.fsclg_slot_set_rows_packed(shim.ctx, slot, hp, w, None)
        got["NULL rows to the packed call"] = L.fsclg_slot_set_rows_packed(shim.ctx, slot, None, 4, None)
        got["NULL rows to the host call"] = L.fsclg_slot_set_rows_host(shim.ctx, slot, None, None)
        over = B.copy()
        over[n - 1] = 65537
        got["a row equal to n_rows"] = L.fsclg_slot_set_rows(shim.ctx, slot, over.ctypes.data, None)
        for s in (-1, 8):
            got[f"slot {s}"] = L.fsclg_slot_set_rows_packed(shim.ctx, s, hp, 4, None)
        for r in rr.plan_refusals(n):
            assert not rr.plan_ok(r.ent, r.grp, n, r.n_grp)
            got[f"plan: {r.name}"] = shim.set_plan(slot, r.ent, r.grp, n_grp=r.n_grp, checked=False)
        rows = shim.read(slot)[0]
        # a batch submitted and not waited for: every set call is refused
        shim.fill_plan(0, *rr.swap_plans()["adjacent"])
        shim._ok(shim.submit(rr.requests(shim.cs), rr.READ_ER, 4, slot), "fsclg_sites_submit")
        busy = {"copy": shim.L.fsclg_slot_set_rows(shim.ctx, slot, A.ctypes.data, None),
                "uploaded": shim.L.fsclg_slot_set_rows(shim.ctx, slot, None, None),
                "host": L.fsclg_slot_set_rows_host(shim.ctx, slot, hp, None),
                "packed": L.fsclg_slot_set_rows_packed(shim.ctx, slot, hp, 4, None),
                "plan": L.fsclg_slot_set_rows_plan(shim.ctx, slot, shim.h_ent[0].ptr, shim.h_grp[0].ptr, 1, None),
                "row buffer": E_STATE if not L.fsclg_slot_row_buffer(shim.ctx, slot) else 0,
                "swap": L.fsclg_slot_swap(shim.ctx, slot, 5)}
        shim.wait(1, 4)
        return got, busy, rows, shim.read(slot)[0]
    got, busy, rows, rows2 = device("refusals", run)
    assert {k: v for k, v in got.items() if v != E_ARG} == {}
    assert {k: v for k, v in busy.items() if v != E_STATE} == {}
    assert not diff(rows, B, "after the refusals") and not diff(rows2, B, "after the busy slot's refusals")


# ------------------------------------------------------------------ plans
def run_plans(shim, plans, what):
    """Each plan into a slot of its own turn, read back and compared with the sequential statement."""
    A = rr.base_rows(rr.PLAN_N, 70000)

    def run():
        bad = []
        shim.upload_rows(70000, A)
        for k, (name, (ent, grp)) in enumerate(plans.items()):
            slot = 1 + k % 7
            shim._ok(shim.set_plan(slot, ent, grp), f"plan {name}")
            shim.wait_slot(slot)
            bad += diff(shim.read(slot)[0], rr.apply_plan(A, ent, grp), f"{what} {name} (slot {slot})")
        bad += diff(shim.read(0)[0], A, "slot 0")
        return bad
    bad = device(what, run)
    assert not bad, "\n".join(bad[:12])


def test_plan_swaps(shim):
    run_plans(shim, rr.swap_plans(), "swap plan")


def test_plan_random(shim):
    run_plans(shim, {str(k): p for k, p in enumerate(rr.random_plans())}, "random plan")


def test_plan_rotations(shim):
    run_plans(shim, rr.rot_plans(), "rotation plan")


def test_plan_rotation_buffer_grows_between_two_slots(built):
    """A context of its own, so that its rotation buffer starts empty: a small rotation in one slot and at
    once, with no wait, a larger one in another, for which the buffer is reallocated."""
    A = rr.base_rows(rr.PLAN_N, 70000)
    small = rr.one_group_each([(127, 128, 3, 1), (700, 900, 300, 1)])
    large = rr.rot_plans()["len-5000-d-4999-down"]
    s = RowsShim()

    def run():
        try:
            s.upload_rows(70000, A)
            s._ok(s.set_plan(2, *small, buf=0), "the small plan")
            s._ok(s.set_plan(6, *large, buf=1), "the large plan")
            return (diff(s.read(2)[0], rr.apply_plan(A, *small), "the small rotation's slot")
                    + diff(s.read(6)[0], rr.apply_plan(A, *large), "the large rotation's slot"))
        finally:
            s.close()
    bad = device("rotation buffer", run)
    assert not bad, "\n".join(bad)


def test_plan_rotation_grid_stride(shim):
    n = rr.BIG_N
    A = rr.base_rows(n, 70000)
    ent, grp = rr.big_plan()

    def run():
        shim.upload_rows(70000, A, *rr.even_chromosomes(n, rr.BIG_PER))
        shim._ok(shim.set_plan(4, ent, grp), "the large rotation")
        return shim.read(4)[0]
    got = device("rotation of 270 000 sites", run)
    bad = diff(got, rr.apply_plan(A, ent, grp), "R = 270 000")
    assert not bad, bad[0]


# ------------------------------------------------------------------ stale window sums
ST_N, ST_ER = 3000, 500


def window_requests(sites):
    return [(0, rr.POS0 + rr.SPACING * i + 1, rr.LALPHA) for i in sites]


def check_windows(hdr, terms, rows, what) -> list:
    """Every header's null_logl and every term are those of `rows` on the header's own proper window."""
    bad = []
    for k, h in enumerate(hdr):
        q = h["pt"]
        ws, we, near = int(q["window_start"]), int(q["window_end"]), int(q["nearest_snp"])
        if not (0 <= ws <= near <= we < len(rows) and we - ws == 2 * ST_ER and int(q["n_snps"]) == 2 * ST_ER + 1):
            bad.append(f"{what}, request {k}: no proper window [{ws}, {we}] around {near}")
            continue
        want = rr.window_null(rows, ws, we)
        if not wr.same(float(q["null_logl"]), want):
            bad.append(f"{what}, request {k}: null_logl {float(q['null_logl'])!r} != {want!r} on [{ws}, {we}]")
        t = terms[int(h["off"]):int(h["off"]) + int(h["len"])]
        try:
            bad += diff(rr.rows_of_terms(near, int(h["nl"]), int(h["nr"]), ws, we, t), rows[ws:we + 1],
                        f"{what}, request {k}, window from {ws}")
        except ValueError as e:
            bad.append(f"{what}, request {k}: {e}")
    return bad


@pytest.mark.parametrize("mode", ["2", "0"])
def test_changed_rows_drop_the_window_sums(shim, mode):
    """FSCLG_WINDOW_CHUNK 2: chunk table and window_chunk_kernel; 0: window_null_kernel (read per call)."""
    n, n_rows = ST_N, 256
    A = rr.base_rows(n, n_rows, seed=20)
    plan = (rr.one_group_each([(5, 1505, 1400, 0), (100, 900, 1500, 1)]))
    os.environ["FSCLG_WINDOW_CHUNK"] = mode

    def run():
        bad = []
        shim.upload_rows(n_rows, A)
        slot, other = 3, 6
        for label, reqs in (("dense", window_requests(list(range(0, n, 50)) + [n - 1])),  # most windows: every one is summed
                            ("sparse", window_requests([700, n - 1]))):                   # few: only theirs
            seed = 30 if label == "dense" else 40
            steps = (("copy", lambda: shim.set_copy(slot, rr.base_rows(n, n_rows, seed + 1)), rr.base_rows(n, n_rows, seed + 1)),
                     ("host", lambda: shim.set_host(slot, rr.base_rows(n, n_rows, seed + 2)), rr.base_rows(n, n_rows, seed + 2)),
                     ("packed", lambda: shim.set_packed(slot, rr.base_rows(n, n_rows, seed + 3), 1),
                      rr.base_rows(n, n_rows, seed + 3)),
                     ("plan", lambda: shim.set_plan(slot, *plan), rr.apply_plan(A, *plan)),
                     ("uploaded", lambda: shim.set_copy(slot, None), A))
            bad += check_windows(*shim.sites(reqs, ST_ER, 0), A, f"{label}: slot 0 first")
            for name, call, want in steps:  # the slot's sums exist for the rows before each call
                shim._ok(call(), name)
                bad += check_windows(*shim.sites(reqs, ST_ER, slot), want, f"{label}: after {name}")
            # the other slot's rows and sums, then the exchange
            X, Y = rr.base_rows(n, n_rows, seed + 5), rr.base_rows(n, n_rows, seed + 6)
            shim._ok(shim.set_host(slot, X), "host")
            bad += check_windows(*shim.sites(reqs, ST_ER, slot), X, f"{label}: X in slot {slot}")
            shim._ok(shim.set_copy(other, Y), "copy")
            bad += check_windows(*shim.sites(reqs, ST_ER, other), Y, f"{label}: Y in slot {other}")
            shim._ok(shim.L.fsclg_slot_swap(shim.ctx, slot, other), "fsclg_slot_swap")
            bad += check_windows(*shim.sites(reqs, ST_ER, slot), Y, f"{label}: slot {slot} after the swap")
            bad += check_windows(*shim.sites(reqs, ST_ER, other), X, f"{label}: slot {other} after the swap")
            bad += check_windows(*shim.sites(reqs, ST_ER, 0), A, f"{label}: slot 0 last")
        return bad
    try:
        bad = device(f"stale sums, mode {mode}", run)
    finally:
        os.environ.pop("FSCLG_WINDOW_CHUNK", None)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:12])
