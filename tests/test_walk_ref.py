"""The plain reference of the alpha search (tests/walk_ref.py) against the oracle, bit for bit, and
the crafted vectors' regimes: what tests/test_exact_sums_gpu.py relies on, checked without a GPU."""
from __future__ import annotations

import math

import pytest

import walk_ref as wr
from util import GOLD, read_dump


@pytest.fixture(scope="module")
def g2(built):
    return wr.OracleTables(GOLD / "g2.snp"), wr.golden_points(read_dump(GOLD / "g2_p30.dump"))


def assert_same(got, want, what):
    for k, name in enumerate(("lalpha", "sm_logl", "clr")):
        assert wr.same(got[k], want[k]), f"{what}: {name} {got[k]!r} ({float(got[k]).hex()}) != {want[k]!r}"


def test_restatement_equals_the_oracle_on_the_golden_points(g2):
    orc, pts = g2
    dump = read_dump(GOLD / "g2_p30.dump")
    assert len(pts) == 40
    for i, p in enumerate(pts):
        got = wr.search(orc.tables, p)[:3]
        assert_same(got, orc.search(p), f"point {i} against orc_search_maxalpha")
        assert_same(got, (dump[i][3], dump[i][4], dump[i][2]), f"point {i} against the golden dump")


def test_restatement_equals_the_oracle_with_crafted_null_sums(g2):
    orc, pts = g2
    for i in range(0, 40, 4):
        for N in wr.N_LIST:
            p = wr.Point(pts[i].nearest_snp, pts[i].sweep_pos, pts[i].window_start, pts[i].window_end, N)
            assert_same(wr.search(orc.tables, p)[:3], orc.search(p), f"point {i} N = {N!r}")


def test_untouched_prior_for_nan_and_minus_inf(g2):
    orc, pts = g2
    for N in (math.nan, -math.inf):
        p = wr.Point(pts[0].nearest_snp, pts[0].sweep_pos, pts[0].window_start, pts[0].window_end, N)
        la, sm, _ = wr.search(orc.tables, p)[:3]
        assert la == 4.0 and sm == -wr.DBL_MAX


def test_geometry_covers_the_part_lengths(built):
    g, n = wr.geometry()
    assert n <= 40000 and g[0].ws == 0 and g[0].near == 128 and g[-1].we == n - 1
    want = {0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4097}
    assert {q.near - q.ws for q in g} == want and {q.we - q.near for q in g} == want
    assert {0, 127} <= {q.near % 128 for q in g}
    for a, b in zip(g, g[1:]):
        assert a.we < b.ws
    # the first coarse alpha's walk is the whole window, part for part
    c = wr.cases()["zero-exact"]
    for q, (_, _, _, D) in zip(g, wr.expected("zero-exact")):
        assert D.lens[0][0] == (q.near - q.ws, q.we - q.near)
        # the last coarse alpha (4.0) cuts at |d| <= 1: at most the nearest SNP and one neighbour
        assert D.lens[0][-1] in ((0, 0), (0, 1)) and sum(D.lens[0][-1]) < q.we - q.ws
    assert c.tables.coef.shape[0] <= 64


def regime_holds(regime: str, name: str, res) -> None:
    """The case's diagnostics show the regime it is named for (at least one point; every point where
    the regime is a property of N)."""
    Ds = [r[3] for r in res]
    per_walk = [t for D in Ds for ph in (0, 1) for t in D.ties[ph]]
    per_phase = [D.phase_ties(ph) for D in Ds for ph in (0, 1)]
    leaves = [any(D.leaves[0]) or any(D.leaves[1]) for D in Ds]
    equal = [D.equal_sums(0) or D.equal_sums(1) for D in Ds]
    if regime in ("sparse", "medium", "dense"):
        # safe by the kernels' own test (resolve_walk): N with every negative term, and N with every
        # positive one, inside the binade (512, 1024) with room for one unit per tie
        c = wr.cases()[name]
        for p in c.points:
            t, _ = wr.walk_terms(c.tables, p, -20.0)
            assert 520.0 < -(p.null_logl + t[t < 0].sum()) < 1020.0 and 520.0 < -(p.null_logl + t[t > 0].sum()) < 1020.0
    if regime == "sparse":
        assert max(per_walk) >= 1 and max(per_walk) <= 15 and not any(leaves)
        odd = [wr.bits(r[1]) & 1 for r in res]  # the sums end on odd and on even grid points
        assert len(set(odd)) == 2
    elif regime == "medium":
        assert any(100 <= t <= 500 for t in per_phase) and any(wr.XTIES < t <= wr.MAXTIES for t in per_walk)
        assert not any(leaves)
    elif regime == "dense":
        assert max(per_phase) > wr.MAXTIES and any(equal) and not any(leaves)
    elif regime == "leaves":
        # (-2^11 itself starts the next binade: negative terms keep it there)
        pts = wr.cases()[name].points
        assert all(lv or (p.null_logl == -2048.0 and "down" in name) for lv, p in zip(leaves, pts)) and all(equal)
        assert sum(leaves) >= len(pts) // 2
    elif regime == "nonneg":
        assert all(leaves) and all(equal) and all(r[1] >= 0.0 for r in res)
    elif regime == "ties1e18":
        assert max(per_walk) > 0 and all(equal)
    elif regime == "nogrid":
        assert all(wr.ulp_of(p.null_logl) == 0.0 for p in wr.cases()[name].points)
    elif regime == "big":
        assert all(max(D.max_r[0]) >= 2.0 ** 51 for D in Ds)
    elif regime == "nonfinite":
        # the long walks meet the non-finite row, the short walks do not and one of them wins
        assert all(any(not math.isfinite(s) for s in D.sums[0]) for D in Ds)
        if name == "row-inf-plus":  # +inf beats every finite sum: the first walk that meets it wins
            assert all(r[1] == math.inf for r in res)
        else:
            assert all(math.isfinite(r[1]) and r[1] > -wr.DBL_MAX for r in res)
    elif regime == "allequal":
        for p, r in zip(wr.cases()[name].points, res):
            assert r[0] == -20.0 and wr.same(r[1], p.null_logl)
    else:
        raise AssertionError(regime)


@pytest.mark.parametrize("name", list(wr.cases()))
def test_vectors_are_in_their_regime(built, name):
    c = wr.cases()[name]
    n = len(c.tables.pos)
    assert n <= 40000 and c.tables.coef.shape[0] <= 64 and int(c.tables.row.max()) < c.tables.coef.shape[0]
    for p in c.points:
        assert 0 <= p.window_start <= p.nearest_snp <= p.window_end < n
    regime_holds(c.regime, name, wr.expected(name))


def test_shapes_reach_every_null_sum(built):
    """The 40- and 130-point calls of the real-table case index a subset of its 190 points: every N
    of the list must be in each."""
    n = 10 * len(wr.N_LIST)
    for idx in wr.shapes(n)[1:]:
        assert {i // 10 for i in idx} == set(range(len(wr.N_LIST)))
    one = wr.shapes(n)[0]
    assert sorted(i for c in one for i in c) == list(range(n))


@pytest.mark.parametrize("name", list(wr.profile_cases()))
def test_profile_vectors(built, name):
    c = wr.profile_cases()[name]
    start, step, count = wr.PROFILE_RUN
    at = [start + k * step for k in range(count)]
    assert len(c.tables.pos) <= 2 * wr.PROFILE_ER + 1 and not set(at) & set(c.tables.pos.tolist())
    pts = wr.oracle_init_points(c.tables.pos, at, wr.PROFILE_ER, c.N)
    for p, x in zip(pts, at):
        assert (p.window_start, p.window_end, p.sweep_pos) == (0, len(c.tables.pos) - 1, x)
    res = [wr.search(c.tables, p) for p in pts]
    if name == "dense":
        assert all(D.phase_ties(0) > wr.MAXTIES and D.equal_sums(0) for *_, D in res)
    elif name == "edge":
        safe, slow = res[wr.PROFILE_SAFE], res[wr.PROFILE_SLOW]
        # the safe point's winner is a walk of zero terms; the walks that leave the binade lose by ~9
        assert wr.same(safe[1], c.N) and not any(lv for lv, s in zip(safe[3].leaves[0], safe[3].sums[0]) if s == c.N)
        assert all(s < c.N - 8.0 for lv, s in zip(safe[3].leaves[0], safe[3].sums[0]) if lv)
        # the other point's winner left the binade, and another walk has the same sum
        assert slow[1] > -1024.0 and slow[3].equal_sums(0)
    else:
        assert all(max(D.max_r[0]) == math.inf and math.isfinite(r1) for _, r1, _, D in res)
