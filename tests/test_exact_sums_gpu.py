"""The exact-sum fallback paths of the alpha search kernels on crafted terms.

With coef[row][iv] = (0, 0, 0, c3[row]) and nullrow = 0 a site's term is exactly c3[row], so
fsclg_search_points sums a sequence of doubles the test picked, from a null sum N the test picked.
Every case is compared with the plain sequential reference (tests/walk_ref.py) by bit pattern, in
three kernel shapes (1 point per call: 8 workgroups per point; 40 points: 6; 130 points: the unsplit
kernel), and the device counter that proves the path ran is asserted after each shape.
tests/test_walk_ref.py checks, without a GPU, that the reference equals the oracle and that every
vector is in the regime it is named for.
"""
from __future__ import annotations

import math

import pytest

import walk_ref as wr
from util import GOLD, read_dump

pytestmark = pytest.mark.gpu

FIELDS = ("lalpha", "sm_logl", "clr")


@pytest.fixture(scope="module")
def shim(built):
    s = wr.Shim()
    yield s
    s.close()


def run_shapes(shim, name, tables, points, want, counters, others=()):
    """The points in the three shapes against want (and others: further references of the same
    points); counters: name -> True (must be > 0 after each shape) or False (must be 0)."""
    try:
        shim.upload(tables)
        one, s40, s130 = wr.shapes(len(points))
        bad = []
        for shape, calls in (("1", one), ("40", [s40]), ("130", [s130])):
            shim.reset_stats()
            for idx in calls:
                got = shim.search([points[i] for i in idx])
                for i, g in zip(idx, got):
                    for ref in (want, *others):
                        for k, f in enumerate(FIELDS):
                            if not wr.same(g[k], ref[i][k]):
                                bad.append(f"shape {shape} point {i} N={points[i].null_logl!r} {f}: "
                                           f"{g[k]!r} ({float(g[k]).hex()}) != {ref[i][k]!r} ({float(ref[i][k]).hex()})")
            st = shim.stats()
            print(f"COUNTERS {name} shape {shape}: n_unsafe={st['n_unsafe']} n_slow={st['n_slow']} "
                  f"n_ties={st['n_ties']} n_walks={st['n_walks']}")
            for c, positive in counters.items():
                if positive and not st[c] > 0:
                    bad.append(f"shape {shape}: {c} == 0, the path did not run")
                if not positive and st[c] != 0:
                    bad.append(f"shape {shape}: {c} == {st[c]}, expected none")
    except RuntimeError as e:  # a device error: nothing more runs on the GPU in this session
        pytest.exit(f"{name}: {e}", returncode=3)
    assert not bad, f"{name}: {len(bad)} mismatches:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("name", list(wr.cases()))
def test_crafted_terms(shim, name):
    c = wr.cases()[name]
    want = [r[:3] for r in wr.expected(name)]
    if c.regime == "allequal":  # every candidate equals N: the first coarse alpha keeps the maximum
        assert all(w[0] == -20.0 for w in want)
    if name == "nogrid":  # N = NaN, -inf: the untouched prior
        for p, w in zip(c.points, want):
            if p.null_logl != p.null_logl or p.null_logl == -math.inf:
                assert w[0] == 4.0 and w[1] == -wr.DBL_MAX
    run_shapes(shim, name, c.tables, c.points, want, c.want)


def test_real_cubic_terms_with_crafted_null_sums(shim):
    """The g2 tables flattened from the oracle: the terms depend on x, so the uniform-interval and
    per-lane paths of the term loop and the slow path's own term evaluation must agree."""
    orc = wr.OracleTables(GOLD / "g2.snp")
    gold = wr.golden_points(read_dump(GOLD / "g2_p30.dump"))[::4]
    assert len(gold) == 10
    pts = [wr.Point(p.nearest_snp, p.sweep_pos, p.window_start, p.window_end, N) for N in wr.N_LIST for p in gold]
    want = [wr.search(orc.tables, p)[:3] for p in pts]
    oracle = [orc.search(p) for p in pts]
    run_shapes(shim, "real-g2", orc.tables, pts, want, {"n_unsafe": True, "n_slow": True},
               others=(oracle,))


@pytest.mark.parametrize("name", list(wr.profile_cases()))
def test_two_points_per_search(shim, name):
    """fsclg_profile: profile_kernel searches two positions at a time, so their candidates share the
    settle rounds.  One whole-chromosome window, its null sum set to the crafted N; the geometry
    from orc_init_scan_result."""
    c = wr.profile_cases()[name]
    start, step, count = wr.PROFILE_RUN
    pts = wr.oracle_init_points(c.tables.pos, [start + k * step for k in range(count)], wr.PROFILE_ER, c.N)
    want = [wr.search(c.tables, p)[:3] for p in pts]
    bad = []
    try:
        shim.upload(c.tables)
        shim.set_chr_null(c.N)
        if name == "edge":  # the pair in different regimes, each point alone first
            for k, slow in ((wr.PROFILE_SAFE, False), (wr.PROFILE_SLOW, True)):
                shim.reset_stats()
                got = shim.search([pts[k]])[0]
                st = shim.stats()
                print(f"COUNTERS profile-{name} point {k} alone: n_unsafe={st['n_unsafe']} n_slow={st['n_slow']}")
                assert all(wr.same(g, w) for g, w in zip(got, want[k]))
                assert (st["n_slow"] > 0) == slow and st["n_unsafe"] > 0
        shim.reset_stats()
        got = shim.profile(start, step, count, wr.PROFILE_ER)
        st = shim.stats()
    except RuntimeError as e:
        pytest.exit(f"profile {name}: {e}", returncode=3)
    print(f"COUNTERS profile-{name}: n_unsafe={st['n_unsafe']} n_slow={st['n_slow']} n_ties={st['n_ties']} "
          f"n_walks={st['n_walks']}")
    for i, ((gp, gv), p, w) in enumerate(zip(got, pts, want)):
        if (gp.nearest_snp, gp.sweep_pos, gp.window_start, gp.window_end) != \
                (p.nearest_snp, p.sweep_pos, p.window_start, p.window_end) or not wr.same(gp.null_logl, c.N):
            bad.append(f"point {i}: geometry {gp} != {p}")
        for k, f in enumerate(FIELDS):
            if not wr.same(gv[k], w[k]):
                bad.append(f"point {i} {f}: {gv[k]!r} ({float(gv[k]).hex()}) != {w[k]!r} ({float(w[k]).hex()})")
    for k, v in c.want.items():
        if v and not st[k] > 0:
            bad.append(f"{k} == 0, the path did not run")
    assert not bad, f"profile {name}: " + "\n".join(bad[:12])
