"""The family-wise maxima on the GPU: maxt_kernel (through fscl_amd_familywise_runs) against the NumPy restatement
of tests/maxt_ref.py, every output bit for bit, and the unpruned pass (fscl_amd_familywise) end to end on the
two-chromosome golden input g1.snp.

End to end, M = 8: the throughput mode with --n-permute=8 prunes nothing on g1 (a prune needs 20 exceedances;
the oracle's restatement of the mode gives permute_n = 9 at all 30 points), so every one of the 30 x 8 (point,
trial) pairs is compared: float(T[t][i]) is the permute_clr[i][t] of that run under the same seed."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import fscl_amd
import maxt_ref as mr
from util import CLI, GOLD

pytestmark = pytest.mark.gpu

SEED = 0xFD821A6
KEYS = ("gmax", "garg", "chr_max", "chr_arg", "c_single", "c_chr", "c_step")


def runs(T, obs, group, G, order=None):
    try:
        return fscl_amd.familywise_runs(T, obs, group, G, order)
    except RuntimeError as e:  # a device error: nothing more runs on the GPU in this session
        pytest.exit(f"familywise_runs: {e}", returncode=3)


def same(got: dict, want: dict, what: str):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k]).astype(np.asarray(got[k]).dtype)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, a.ravel()[:8], b.ravel()[:8])


CASES = mr.cases()
SIZES = sorted({c[1].shape[1] for c in CASES})


def test_geometry(built):
    assert (fscl_amd.MAXT_WG, fscl_amd.MAXT_TILE) == (mr.WG, mr.TILE)
    assert {1, 63, 64, 65, mr.WG - 1, mr.WG, mr.WG + 1, 2 * mr.TILE + 1} <= set(SIZES)


@pytest.mark.parametrize("m", SIZES)
def test_kernel_against_restatement(built, m):
    n = 0
    for name, T, obs, group, G in CASES:
        if T.shape[1] != m:
            continue
        order = mr.order_of(obs)
        assert fscl_amd.familywise_order(obs).tobytes() == order.tobytes(), name
        got = runs(T, obs, group, G)
        same(got, mr.kernel(T, obs, order, group, G), name)
        n += 1
    assert n > 0 and fscl_amd.familywise_last_ms() > 0.0


def test_special_values(built):
    by = {c[0]: c for c in CASES}
    name, T, obs, group, G = by["special"]
    got = runs(T, obs, group, G)
    m = T.shape[1]
    assert got["gmax"][0] == 0.0 and not np.signbit(got["gmax"][0]) and got["garg"][0] == 0       # the all-zero trial
    assert got["gmax"][2] == -np.inf and got["garg"][2] == -1                                     # the all-NaN trial
    assert got["gmax"][3] == np.inf and got["garg"][3] == m // 2
    assert (got["garg"][4], got["garg"][5]) == (0, m - 1)                                         # first and last position
    assert got["gmax"][6] == 0.0 and not np.signbit(got["gmax"][6])                                # a maximum of -0.0 is +0.0
    assert (got["chr_max"][:, 7] == -np.inf).all() and (got["chr_arg"][:, 7] == -1).all()         # the empty group
    zero = np.flatnonzero(obs == 0.0)
    assert len(zero) > 100 and (got["c_single"][zero] == 6).all()    # >= counts ties: every trial but the all-NaN one
    assert got["c_single"][m - 2] == 0 and got["c_step"][m - 2] == 0                               # a NaN obs counts nothing
    # the same bytes again, with one trial per chunk, and with any other chunking
    again = runs(T, obs, group, G)
    same(again, got, "repeat")
    for cap in (8 * m, 3 * 8 * m):
        os.environ["FSCL_AMD_FWER_CAP"] = str(cap)
        try:
            assert fscl_amd.familywise_chunk(m, 7) == cap // (8 * m)
            same(runs(T, obs, group, G), got, f"cap {cap}")
        finally:
            del os.environ["FSCL_AMD_FWER_CAP"]
    # any permutation is accepted as the rank order and defines the suffixes
    order = np.random.default_rng(3).permutation(m).astype(np.int32)
    same(runs(T, obs, group, G, order), mr.kernel(T, obs, order, group, G), "random order")


def test_errors(built):
    T, obs, grp = np.zeros((2, 4)), np.zeros(4), np.zeros(4, np.int32)
    for kw in (dict(group=[0, 0, 0, 1], G=1), dict(group=[0, -1, 0, 0], G=1), dict(order=[0, 1, 2, 2]), dict(order=[0, 1, 2, 4]),
               dict(G=fscl_amd.MAXT_MAX_GROUPS + 1)):
        with pytest.raises(ValueError, match="code -1"):
            fscl_amd.familywise_runs(T, obs, kw.get("group", grp), kw.get("G", 1), kw.get("order"))
    got = runs(T, obs, grp, 1)   # the context still works
    assert (got["c_single"] == 2).all() and (got["gmax"] == 0.0).all()
    empty = runs(np.zeros((3, 0)), np.zeros(0), np.zeros(0, np.int32), 2)
    assert (empty["gmax"] == -np.inf).all() and (empty["garg"] == -1).all() and (empty["chr_arg"] == -1).all()


@pytest.fixture(scope="module")
def g1(built):
    """g1.snp scanned; the throughput mode's 8-permutation test on a scan of its own for the comparison."""
    def load():
        fscl_amd.get_lib().configure_logmsg(0)
        fscl_amd.init_log_table()
        scan = fscl_amd.load_snp_input(GOLD / "g1.snp")
        fsp = fscl_amd.background_fsp(scan)
        tab = fscl_amd.compute_sweep_model_tables(scan, fsp)
        fscl_amd.compute_snp_null_model(scan, fsp)
        fscl_amd.scan_chromosome(scan, tab)
        return scan, tab
    scan, tab = load()
    fw = fscl_amd.familywise(scan, tab, trials=8, seed=SEED, matrix=True)
    return scan, tab, fw


def test_end_to_end_against_throughput_mode(g1, tmp_path):
    scan, tab, fw = g1
    T = fw["familywise_matrix"]
    n = scan.contents.n_scan_pts
    assert T.shape == (8, n) and n == 30 and scan.contents.n_chromosomes == 2
    before = fscl_amd.points(scan).copy()
    ref = fscl_amd.run(GOLD / "g1.snp", None, n_permute=8, permute_mode="throughput", permute_seed=SEED, verbosity=0)
    fscl_amd.set_permute_mode("parity")
    recs = fscl_amd.tail_records(ref)
    compared = 0
    for i in range(n):
        for t in range(min(len(recs[i]), 8)):
            assert np.float32(T[t, i]) == recs[i][t], (i, t, T[t, i], recs[i][t])
            compared += 1
    print(f"compared {compared} of {8 * n} (point, trial) pairs")
    assert 2 * compared >= 8 * n
    assert fscl_amd.points(scan).tobytes() == before.tobytes()   # the pass touched no scan point


def test_counts_and_p_values(g1):
    scan, tab, fw = g1
    p = fscl_amd.points(scan)
    obs, grp = p["clr"].astype(np.float64), p["chr"].astype(np.int32)
    order = mr.order_of(obs)
    assert fw["order"].tobytes() == order.tobytes()
    same(fw, mr.kernel(fw["familywise_matrix"], obs, order, grp, 2), "pass")
    got = fscl_amd.familywise_combine(fw["c_single"], fw["c_chr"], fw["c_step"], fw["order"], 8)
    want = mr.combine(fw["c_single"], fw["c_chr"], fw["c_step"], order, 8)
    for k in ("rank", "p_single", "p_chr", "p_step"):
        assert got[k].tobytes() == want[k].astype(got[k].dtype).tobytes(), k
    # a suffix or chromosome maximum never exceeds the genome's, and the step-down value never falls down the ranks
    assert (got["p_step"] <= got["p_single"]).all() and (got["p_chr"] <= got["p_single"]).all()
    assert (np.diff(got["p_step"][order]) >= 0).all()
    assert fw["kernel_ms"] > 0.0 and fw["wall_s"] > 0.0


def test_independent_of_chunk_and_context(g1):
    scan, tab, fw = g1
    n = scan.contents.n_scan_pts
    os.environ["FSCL_AMD_FWER_CAP"] = str(8 * n)   # one trial per chunk
    os.environ["FSCL_AMD_DEPTH"] = "1"             # and no pipelining
    try:
        one = fscl_amd.familywise(scan, tab, trials=8, seed=SEED, matrix=True)
    finally:
        del os.environ["FSCL_AMD_FWER_CAP"], os.environ["FSCL_AMD_DEPTH"]
    for k in KEYS + ("order", "familywise_matrix"):
        assert np.asarray(one[k]).tobytes() == np.asarray(fw[k]).tobytes(), k
    fscl_amd.set_devices([0, 0])   # two contexts on the one GPU, as the other steps' tests do: two trials a round
    try:
        two = fscl_amd.familywise(scan, tab, trials=8, seed=SEED, matrix=True)
        assert fscl_amd.get_lib().fscl_amd_n_devices() == 2
    finally:
        fscl_amd.set_device(0)
    for k in KEYS + ("order", "familywise_matrix"):
        assert np.asarray(two[k]).tobytes() == np.asarray(fw[k]).tobytes(), k
    other = fscl_amd.familywise(scan, tab, trials=2, seed=SEED + 1, matrix=True)
    assert other["familywise_matrix"].tobytes() != fw["familywise_matrix"][:2].tobytes()   # the seed is used


def test_cli_side_effects(built, tmp_path):
    """The -o file, the null dump and a following permutation test are what they are without the option."""
    def cli(out, extra):
        r = subprocess.run([str(CLI), "-f", str(GOLD / "g1.snp"), "-o", str(out), "--n-permute=25", "--prepend-label=L"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r
    base, out, fwf, nul = tmp_path / "base.txt", tmp_path / "o.txt", tmp_path / "fw.txt", tmp_path / "null.txt"
    cli(base, [])
    r = cli(out, [f"--familywise-file={fwf}", "--familywise-trials=8", f"--familywise-null-file={nul}"])
    assert "Family-wise maxima: M 8 unpruned trials of 30 points" in r.stderr + r.stdout
    assert out.read_bytes() == base.read_bytes()
    assert [ln[2:] for ln in out.read_text().splitlines(True)] == (GOLD / "g1_p25.out").read_text().splitlines(True)   # less the label
    rows = [ln.split("\t") for ln in fwf.read_text().splitlines()]
    assert len(rows) == 30 + 2 + 1 and all(r[0] == "L" for r in rows)
    assert [r[1:3] for r in rows[30:]] == [["chr1", "summary"], ["chr2", "summary"], ["genome", "summary"]]
    assert len(nul.read_text().splitlines()) == 8
    # in process: the same file, the records of the permutation test untouched, and the next test's stream too
    o2, fw2 = tmp_path / "o2.txt", tmp_path / "fw2.txt"
    scan = fscl_amd.run(GOLD / "g1.snp", o2, n_permute=25, label="L", verbosity=0, familywise_file=fw2, familywise_trials=8)
    assert o2.read_bytes() == base.read_bytes() and fw2.read_bytes() == fwf.read_bytes()
    plain = fscl_amd.run(GOLD / "g1.snp", None, n_permute=25, verbosity=0)
    assert fscl_amd.points(scan).tobytes() == fscl_amd.points(plain).tobytes()
    for a, b in zip(fscl_amd.tail_records(scan), fscl_amd.tail_records(plain)):
        assert a.tobytes() == b.tobytes()
    # --n-permute=0 is allowed: the pass does not depend on the permutation test
    fw0 = tmp_path / "fw0.txt"
    r = subprocess.run([str(CLI), "-f", str(GOLD / "g1.snp"), "-o", str(tmp_path / "o0.txt"), f"--familywise-file={fw0}",
                        "--familywise-trials=8", "--prepend-label=L"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert fw0.read_bytes() == fwf.read_bytes()
