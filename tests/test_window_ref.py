"""The window null-sum vectors of tests/window_ref.py, without a GPU: the wave model of
window_chunk_kernel equals the sequential sums bit for bit on every case, chunk_params' restatement
gives what each case is named for, and every case shows the events it lists -- so that a vector named
for a regime of the kernels is in it when tests/test_window_sums_gpu.py runs it on the device."""
from __future__ import annotations

import numpy as np
import pytest

import walk_ref as wr
import window_ref as w

CASES = list(w.cases())


@pytest.fixture(scope="module")
def counted(built):
    """name -> the events of the case's every window, in the default mode (block maps, two-level
    descent), filled by test_model_is_the_sequential_sum."""
    return {}


def _every_window(c, model):
    g, bad, n = c.geom, [], 0
    for cs, cn in zip(g.chr_start, g.chr_n):
        if cn <= g.W:
            continue
        nwin = cn - g.W + 1
        got = model.windows(cs, nwin)
        ref = w.seq_windows(c.values, g.W, range(cs, cs + nwin))
        bad += [f"start {cs + i}: {got[i]!r} ({float(got[i]).hex()}) != {ref[i]!r} ({float(ref[i]).hex()})"
                for i in range(nwin) if not wr.same(got[i], ref[i])]
        n += nwin
    return bad, n


@pytest.mark.parametrize("name", CASES)
def test_model_is_the_sequential_sum(built, counted, name):
    c = w.cases()[name]
    g = c.geom
    emin, ne, ok = w.chunk_params(c.nullrow, g.W)
    assert ok == c.expect.get("accepted", True)
    assert w.lmax_of(g.W) == {"small": 3, "long": 3, "mid": 7, "mid-odd": 6, "prod": 11, "cap": w.CT_LMAX}[g.name]
    assert c.on_device == (g.name != "cap")
    if not ok:  # the sequential kernels sum these; the reference is all there is to check
        assert not c.events
        return
    if "ne" in c.expect:
        assert ne == c.expect["ne"]
    if "ne_min" in c.expect:
        assert ne >= c.expect["ne_min"]
    if "top" in c.expect:
        assert emin + ne - 1 == c.expect["top"]
    model = c.model()
    bad, n = _every_window(c, model)
    assert n == {"small": 1511, "long": 2500, "mid": 701, "mid-odd": 701, "prod": 322, "cap": 65}[g.name]
    assert not bad, f"{name}: {len(bad)} of {n} windows:\n" + "\n".join(bad[:8])
    counted[name] = model.ev
    print(f"EVENTS {name}: emin {emin} ne {ne} " + " ".join(f"{k}={v}" for k, v in sorted(model.ev.items())))
    missing = [e for e in c.events if model.ev[e] <= 0]
    assert not missing, f"{name} is not in the regime it is named for: no {missing}"


@pytest.mark.parametrize("name", [n for n in CASES if w.cases()[n].expect.get("accepted", True)
                                  and w.cases()[n].geom.name in ("small", "mid", "mid-odd", "prod")])
@pytest.mark.parametrize("variant", ["no-descent", "no-tree"])
def test_model_variants_are_the_sequential_sum(built, name, variant):
    """The halving search one level per round trip (FSCLG_WIN_DESC=0) and one step per chunk in groups
    of 16 (FSCLG_WINDOW_TREE=0), as the child-process variants of the device test run them."""
    c = w.cases()[name]
    bad, _ = _every_window(c, c.model(tree=variant != "no-tree", wdesc=variant != "no-descent"))
    assert not bad, f"{name} {variant}: {len(bad)} windows:\n" + "\n".join(bad[:8])


def test_every_regime_is_in_some_case(built, counted):
    """Each regime of DESIGN.md §4.5's list, in the case that is named for it."""
    ev = {n: (counted[n] if n in counted else _counts(n)) for n in CASES if w.cases()[n].expect.get("accepted", True)}
    need = {
        "mid/ties": ["fast_tie", "all_tie_chunk", "dd_even", "dd_odd", "blk_dd_even", "blk_dd_odd"],
        "prod/crossings": [f"level{L}" for L in range(1, 11)] + ["fail_ge2", "desc_fit_fit", "desc_fit_fail",
                                                                 "desc_fail_fit", "desc_fail_fail", "break_chunk",
                                                                 "break_descent", "mixed_binade", "own_entry", "head"],
        "cap/crossings": ["level12"],
        "small/irregular": ["nan_block", "chunk_by_sites", "positive_sum", "binade_back"],
        "cap/ne13": ["k_ge_12"],
        "mid-odd/top_binade": ["fast_tie"],
        "small/real": ["head"],
    }
    for name, events in need.items():
        missing = [e for e in events if ev[name][e] <= 0]
        assert not missing, f"{name}: no {missing}"
    # a window whose sum never reaches 2^emin: the zero-valued stretch aside, only where the values allow
    assert ev["small/irregular"]["never_emin"] > 0
    # out of reach: the top level where only the block at chunk 0 fits, and the spare
    # binade index ne - 1 = 12 of prod
    assert ev["prod/crossings"]["level11"] == 0 and ev["mid/crossings"]["level7"] == 0
    assert all(ev[n]["k_ge_12"] == 0 for n in ev if n.startswith("prod/"))


def _counts(name):
    c = w.cases()[name]
    m = c.model()
    _every_window(c, m)
    return m.ev


def test_geometry_and_the_partial_rule(built):
    """The runs of the device test: the dense runs read every window start; the three partial runs are a
    partial set for the host (launch_partial_windows) only on the long chromosome."""
    for name, c in w.cases().items():
        g = c.geom
        exp_ws = set()
        for r in c.dense_runs():
            near, ws, we = w.point_geometry(g.chr_start, g.chr_n, g.er, r)
            assert np.all(we - ws + 1 == min(g.W, g.chr_n[r.chr])) and np.all((ws <= near) & (near <= we))
            exp_ws |= set(ws.tolist())
        for cs, cn in zip(g.chr_start, g.chr_n):
            if cn > g.W:
                assert set(range(cs, cs + cn - g.W + 1)) <= exp_ws, name
        _, partial = w.window_ranges(g.chr_start, g.chr_n, g.er, c.dense_runs())
        assert not partial, name
        pr = c.partial_runs()
        assert bool(pr) == (g.name in ("small", "long")), name
        if pr:
            assert [r.count for r in pr] == [1, 70, 300]
            rg, partial = w.window_ranges(g.chr_start, g.chr_n, g.er, pr)
            assert len(rg) == 3 and partial == (g.name == "long"), (name, rg)
            assert 2 * sum(b - a for a, b in rg) < sum(n - g.W + 1 for n in g.chr_n if n > g.W)
