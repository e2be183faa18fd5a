"""The slot row cases of tests/rows_ref.py, without a GPU: every case is in the regime it is named for
(lengths, tails modulo 4 / 16 / 256 / 512 / 1024, the highest row value of each width, R above the
rotation kernels' grid), the read-back tables give a site's row as its term, the host applier
fh_plan_apply_u32 of the built library gives the rows of the sequential restatement on every crafted and
random plan, and the restated validator refuses every refusal case and accepts every plan the GPU test
sends -- so that tests/test_slot_rows_gpu.py never sends a plan whose group races by contract."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rows_ref as rr
import walk_ref as wr


def all_plans() -> dict:
    """name -> (n, ent, grp): every plan the GPU test sends."""
    out = {f"swap {k}": (rr.PLAN_N, *p) for k, p in rr.swap_plans().items()}
    out.update({f"random {k}": (rr.PLAN_N, *p) for k, p in enumerate(rr.random_plans())})
    out.update({f"rot {k}": (rr.PLAN_N, *p) for k, p in rr.rot_plans().items()})
    out["big"] = (rr.BIG_N, *rr.big_plan())
    return out


def host_apply(rows, n, ent, grp):
    L = wr._lib()
    L.fh_plan_apply_u32.restype = None
    L.fh_plan_apply_u32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    r = np.array(rows, dtype=np.uint32, copy=True)
    e = np.ascontiguousarray(np.array(ent, dtype=np.int32).reshape(-1, 4))
    g = np.ascontiguousarray(np.array(grp, dtype=np.int32))
    L.fh_plan_apply_u32(r.ctypes.data, n, e.ctypes.data, g.ctypes.data, len(grp) - 1)
    return r


def test_scatter_cases_are_in_their_regimes():
    assert rr.SCATTER_N == [1, 63, 64, 1024, 1025, 3589, 3597]
    # 3589 = 3 * 1024 + 517 = 7 * 512 + 5 = 14 * 256 + 5: a last block of whole 16-byte reads plus a scalar rest
    # in the 1- and 4-byte widths; 5 two-byte rows are less than one read (8), so 3597 = 7 * 512 + 13 is there too
    for n, tails in ((3589, (517, 5, 5)), (3597, (525, 13, 13))):
        for width, per, tail in zip((1, 2, 4), (1024, 512, 256), tails):
            E = 16 // width
            assert per == 64 * E and n % per == tail and tail % E != 0  # a partial read in the last block ...
            assert tail >= E or (n, width) == (3589, 2)                 # ... after at least one whole read
    assert 1025 % 1024 == 1 and 1025 % 512 == 1 and 1025 % 256 == 1   # a second block of one site
    assert 1024 % 1024 == 0 and 63 < 64                                # exactly whole blocks; less than one wave
    for width, n_rows in rr.WIDTH_ROWS.items():
        assert n_rows <= 1 << (8 * width) and (width == 4 or n_rows == 1 << (8 * width))
        for n in rr.SCATTER_N:
            r = rr.scatter_rows(width, n)
            assert len(r) == n and int(r.max()) == n_rows - 1 and int(r[-1]) == n_rows - 1
            assert r.astype(rr.WIDTH_DTYPE[width]).astype(np.uint32).tolist() == r.tolist()  # fits the staging
            if width == 4 and n > 2:
                assert int(np.sort(r)[1]) > 0xFFFF  # all but the planted 0
            if n > 1:
                assert int(r.min()) == 0
            assert r.tobytes() == rr.scatter_rows(width, n).tobytes()  # seeded
            assert r.tobytes() != rr.base_rows(n, n_rows).tobytes() or n == 1


def test_read_back_tables_give_the_rows():
    """walk_terms on the identity tables: the request of rows_ref.requests walks its whole chromosome from
    the first site rightwards and every term is the site's row + 1, also where the interval clamps at
    N_IV_WIDE - 1."""
    for n_rows in (256, 70000):
        n = 3589
        rows = rr.scatter_rows(4 if n_rows > 256 else 1, n)
        T = rr.tables(n_rows, rows)
        assert T.coef.shape[1] == (wr.N_IV if n_rows <= 256 else rr.N_IV_WIDE)
        cs, cn = rr.even_chromosomes(n, 1500)
        assert cn == [1500, 1500, 589]
        got = []
        for (c, pos, la), a, m in zip(rr.requests(cs), cs, cn):
            assert pos == int(T.pos[a]) and la == wr.LOG_AD_MIN
            pt = wr.Point(a, pos + 1, a, a + m - 1, -1.0)  # de-collided; the first site is the nearest
            assert abs(int(T.pos[a]) - pt.sweep_pos) < abs(int(T.pos[a + 1]) - pt.sweep_pos)
            t, (nl, nr) = wr.walk_terms(T, pt, la)
            assert (nl, nr) == (0, m - 1)
            got.append(rr.rows_of_terms(a, nl, nr, a, a + m - 1, t))
            assert wr.same(rr.window_null(rows, a, a + m - 1), float(T.nullrow[rows[a:a + m]].sum()))
        assert np.concatenate(got).tobytes() == rows.tobytes()
    # a walk from the middle of a window: walk order is undone
    rows = rr.base_rows(100, 256)
    T = rr.tables(256, rows)
    t, (nl, nr) = wr.walk_terms(T, wr.Point(40, int(T.pos[40]) + 1, 10, 90, -1.0), rr.LALPHA)
    assert (nl, nr) == (30, 50) and rr.rows_of_terms(40, nl, nr, 10, 90, t).tolist() == rows[10:91].tolist()
    with pytest.raises(ValueError):
        rr.rows_of_terms(40, nl, nr - 1, 10, 90, t)
    with pytest.raises(ValueError):
        rr.rows_of_terms(40, nl, nr, 10, 90, t + 0.5)


def test_plan_cases_are_in_their_regimes():
    S, P = rr.SWAP_ROUND, rr.SWAP_ROUND * rr.SWAP_PER
    assert (S, P, rr.SWAP_MAX) == (256, 768, 4096)
    assert rr.SWAP_LEN == [1, S - 1, S, S + 1, P - 1, P, P + 1, 2 * P, 2 * P + 1, rr.SWAP_MAX - 1, rr.SWAP_MAX]
    sw = rr.swap_plans()
    lens = sorted(e[2] for k, (ent, _) in sw.items() if k.startswith("len-") for e in ent)
    assert lens == rr.SWAP_LEN
    odd = cross = rev = 0
    for k, (ent, grp) in sw.items():
        for i, j, ln, kind in ent:
            assert kind == 0
            odd += i % 2 == 1 or j % 2 == 1
            cross += (i // 128 != (i + ln - 1) // 128) or (j // 128 != (j + ln - 1) // 128)
            rev += i > j
    assert odd >= 11 and cross >= 10 and rev >= 3
    (i, j, ln, _), = sw["adjacent"][0]
    assert j == i + ln
    ent, grp = sw["groups"]
    assert grp[1] > 0 and min(grp[q + 1] - grp[q] for q in range(len(grp) - 1)) >= 2

    def sites(es):
        s = set()
        for i, j, ln, _ in es:
            s |= set(range(i, i + ln)) | set(range(j, j + ln))
        return s
    for name in ("groups", "order"):  # a later group moves sites an earlier one moved, and the order shows
        ent, grp = sw[name]
        assert sites(ent[grp[0]:grp[1]]) & sites(ent[grp[1]:grp[2]])
        rows = rr.base_rows(rr.PLAN_N, 70000)
        back = (ent[grp[1]:] + ent[:grp[1]], [0, len(ent) - grp[1], len(ent)])
        assert rr.apply_plan(rows, ent, grp).tobytes() != rr.apply_plan(rows, *back).tobytes()
    ro = rr.rot_plans()
    want = {(ln, d, o) for ln in rr.ROT_LEN for d in rr.rot_ds(ln) for o in (1, -1)}
    got = {(ln, abs(i - j), 1 if i < j else -1) for k, (ent, _) in ro.items() if k.startswith("len-")
           for i, j, ln, kind in ent if kind == 1}
    assert got == want and {d for ln, d, _ in want if ln == 5000} == {1, 2, 2500, 4999}
    assert {d for ln, d, _ in want if ln == 2} == {1} and {d for ln, d, _ in want if ln == 3} == {1, 2}
    assert [e[3] for e in ro["between-swaps"][0]] == [0, 1, 0] and ro["d-0"][0][0][0] == ro["d-0"][0][0][1]
    (i, j, ln, kind), = rr.big_plan()[0]
    assert kind == 1 and ln + abs(i - j) == 270_000 > rr.ROT_GRID == 262_144 and max(i, j) + ln <= rr.BIG_N
    kinds = [e[3] for ent, _ in rr.random_plans() for e in ent]
    assert len(rr.random_plans()) == 20 and kinds.count(0) > 40 and kinds.count(1) >= 5
    assert max(grp[q + 1] - grp[q] for _, grp in rr.random_plans() for q in range(len(grp) - 1)) >= 4


@pytest.mark.parametrize("name", list(all_plans()))
def test_host_applier_is_the_sequential_statement(built, name):
    n, ent, grp = all_plans()[name]
    assert rr.plan_refusal(ent, grp, n) is None, name
    rows = rr.base_rows(n, 70000)
    want = rr.apply_plan(rows, ent, grp)
    assert host_apply(rows, n, ent, grp).tobytes() == want.tobytes()
    assert sorted(want.tolist()) == sorted(rows.tolist())  # a permutation of the rows
    if name != "rot d-0" and any(e[2] for e in ent):
        assert want.tobytes() != rows.tobytes()
    else:
        assert want.tobytes() == rows.tobytes()


def test_sequential_swaps_are_the_rotation():
    """The closed form the kernels use, against the element swaps, at the lengths and distances of the issue."""
    for ln in (2, 3, 7, 300, 1000):
        for d in sorted({0, 1, 2, 3, ln // 2, ln - 1}):
            if d >= ln:
                continue
            for i, j in ((50, 50 + d), (50 + d, 50)):
                rows = np.arange(2200, dtype=np.uint32)
                got = rr.apply_plan(rows, [(i, j, ln, 1)], [0, 1])
                want = rows.copy()
                t = np.arange(ln + d)
                if d:
                    want[50:50 + ln + d] = rows[50 + np.where(t < ln, d + t, t % d)]
                assert got.tolist() == want.tolist(), (ln, d, i, j)


def test_validator_restated():
    for r in rr.plan_refusals():
        assert not rr.plan_ok(r.ent, r.grp, rr.PLAN_N, r.n_grp), r.name
    assert len({r.name for r in rr.plan_refusals()}) == len(rr.plan_refusals())
    for name, (n, ent, grp) in all_plans().items():
        assert rr.plan_ok(ent, grp, n), name
    assert rr.plan_ok(None, None, rr.PLAN_N, 0) and rr.plan_ok([], [0], rr.PLAN_N)
    # the caller's contract, which the shim does not check: entries of one group on the same sites
    assert rr.plan_refusal([(0, 5000, 100, 0), (50, 7000, 100, 0)], [0, 2], rr.PLAN_N).endswith("(the caller's contract)")
    assert rr.plan_ok([(0, 5000, 100, 0), (50, 7000, 100, 0)], [0, 1, 2], rr.PLAN_N)
    assert rr.plan_ok([(0, 100, 100, 0), (200, 5000, 0, 0)], [0, 2], rr.PLAN_N)  # d = len; an empty entry
