"""The sweep-model sampler (fsclg_sample_submit, fscl_amd_simulate) and the parametric bootstrap on
the GPU.

Every drawn count is compared with the NumPy restatement of tests/sample_ref.py.  That reference
leaves no site of any input here undecided (its threshold further than 1e-9, relative, from every
cumulative sum; tests/test_simulate_host.py checks it), so equality is demanded at every site.
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import fscl_amd
import sample_ref as sr
from util import CLI

pytestmark = pytest.mark.gpu

ER, RESL, GRID = 81920, 128, 100000


def draw(c, sweeps=None, seed=sr.SEED, rep=sr.REP):
    try:
        return fscl_amd.simulate(c.scan, c.tables, c.sweeps if sweeps is None else sweeps, seed, rep)
    except RuntimeError as e:  # a device error: nothing more runs on the GPU in this session
        pytest.exit(f"{c.name}: {e}", returncode=3)


def check_equal(name, f, want, what=""):
    bad = np.flatnonzero(f != want.f)
    assert not len(bad), (f"{name}{what}: {len(bad)} of {len(f)} sites differ, first site {bad[0]}: {f[bad[0]]} != "
                          f"{want.f[bad[0]]} (margin {want.margin[bad[0]]!r}, log_ad {want.log_ad[bad[0]]!r})")


@pytest.mark.parametrize("name", ["d2_3"] + [f"d{n}" for n in sr.WAVE_DEPTHS])
def test_exact_against_the_reference(built, name):
    c = sr.case(name)
    M = c.model
    want, neutral = sr.reference(name), sr.reference(name, True)
    assert want.undecided == 0 and neutral.undecided == 0
    f, deg = draw(c)
    f0, deg0 = draw(c, [])
    n = np.array(M.depth_n)[M.depth_p]
    assert f.dtype == np.int32 and len(f) == len(M.pos)
    assert ((f >= 1) & (f <= n - 1)).all() and ((f0 >= 1) & (f0 <= n - 1)).all()
    check_equal(name, f, want)
    check_equal(name, f0, neutral, " (neutral)")
    assert deg == want.n_degenerate == 0 and deg0 == 0
    near = want.log_ad <= sr.LOG_AD_MAX
    assert near.sum() >= 300
    assert int((f[near] != f0[near]).sum()) >= 100, "the sweep branch leaves the replicate neutral"
    assert (f[~near] == f0[~near]).all()
    assert fscl_amd.simulate_last_ms() > 0.0


def test_mixed_data(built):
    c = sr.case("mixed")
    M = c.model
    want, neutral = sr.reference("mixed"), sr.reference("mixed", True)
    f, deg = draw(c)
    f0, _ = draw(c, [])
    check_equal("mixed", f, want)
    check_equal("mixed", f0, neutral, " (neutral)")
    assert deg == want.n_degenerate
    third = M.chrom == 2
    assert third.sum() == 1001 and (f[third] == f0[third]).all()         # no sweep on the third chromosome
    assert int((f[~third] != f0[~third]).sum()) >= 100
    # the order of the sweeps does not matter, nor does a sweep on another chromosome
    f2, _ = draw(c, c.sweeps[::-1])
    assert (f2 == f).all()
    # the replicate folds at the folded sites
    r = fscl_amd.simulate_scan(c.scan, f)
    obs = np.array([r.contents.snps[i].obs_freq for i in range(len(f))])
    n = np.array(M.depth_n)[M.depth_p]
    assert (obs == np.where(M.folded == 1, np.minimum(f, n - f), f)).all()
    fscl_amd.scan_free(r)


def test_ascertained_tables(built):
    c = sr.case("asc")
    want = sr.reference("asc")
    f, deg = draw(c)
    check_equal("asc", f, want)
    assert deg == want.n_degenerate
    assert (f >= 2).all() and (f <= 38).all() and (want.p_drawn > 0.0).all()   # no count of probability 0


def test_errors(built):
    c = sr.case("mixed")
    for bad in ([(0, 5000, 0.0)], [(0, 5000, -1e-4)], [(3, 5000, 1e-4)], [(-1, 5000, 1e-4)], [(0, 5000, float("nan"))]):
        with pytest.raises(RuntimeError, match="code -1"):
            fscl_amd.simulate(c.scan, c.tables, bad, 1, 0)
    f, _ = draw(c)   # the context still works
    assert (f == sr.reference("mixed").f).all()


def test_determinism_and_independence(built, tmp_path):
    c = sr.case("boot")
    fscl_amd.scan_chromosome(c.scan, c.tables, ER, RESL, GRID)
    before = fscl_amd.points(c.scan).tobytes()
    a, _ = draw(c)
    b, _ = draw(c)
    assert a.tobytes() == b.tobytes()
    assert fscl_amd.points(c.scan).tobytes() == before, "a replicate changed the scan's points"
    other, _ = draw(c, rep=sr.REP + 1)
    seeded, _ = draw(c, seed=sr.SEED + 1)
    assert (other != a).sum() > 1000 and (seeded != a).sum() > 1000 and (other != seeded).sum() > 1000
    fscl_amd.srand()
    fscl_amd.scan_permute(c.scan, c.tables, 2, 0.1, 1.0, 1, ER, RESL, GRID, 1.0)
    after, _ = draw(c)
    assert after.tobytes() == a.tobytes(), "a replicate depends on a previous scan_permute"
    # and on nothing another input left on the device
    draw(sr.case("d65"))
    again, _ = draw(c)
    assert again.tobytes() == a.tobytes()


def test_bootstrap_composition(built, tmp_path):
    c = sr.case("boot")
    reps, seed, window = 8, 77, 200000
    fscl_amd.scan_chromosome(c.scan, c.tables, ER, RESL, GRID)
    o1, o2 = tmp_path / "before.txt", tmp_path / "after.txt"
    fscl_amd.scan_output(o1, c.scan)
    rows = fscl_amd.bootstrap(c.scan, c.tables, c.fsp, c.sweeps, reps, seed, window, ER, RESL, GRID)
    fscl_amd.scan_output(o2, c.scan)
    assert o1.read_bytes() == o2.read_bytes(), "the bootstrap changed the scan"
    assert rows.dtype == fscl_amd.BOOT_DTYPE and len(rows) == reps
    chrom, planted, alpha = c.sweeps[0]
    found = 0
    for rep in range(reps):
        f, _ = fscl_amd.simulate(c.scan, c.tables, c.sweeps, seed, rep)
        r = fscl_amd.simulate_scan(c.scan, f)
        fscl_amd.compute_snp_null_model(r, c.fsp)
        fscl_amd.scan_chromosome(r, c.tables, ER, RESL, GRID)
        p = fscl_amd.points(r)
        fscl_amd.scan_free(r)
        ok = np.flatnonzero((p["chr"] == chrom) & (np.abs(p["sweep_pos"].astype(np.int64) - planted) <= window))
        q = rows[rep]
        assert (q["sweep"], q["rep"], q["chr"], q["planted_pos"], q["planted_alpha"]) == (0, rep, chrom, planted, alpha)
        if not len(ok):
            assert q["est_pos"] == -1 and np.isnan(q["est_lalpha"]) and np.isnan(q["clr"])
            continue
        best = ok[int(np.argmax(p["clr"][ok]))]   # (argmax: the first of equal maxima)
        assert q["est_pos"] == p["sweep_pos"][best]
        assert q["est_lalpha"].tobytes() == p["lalpha"][best].tobytes() and q["clr"].tobytes() == p["clr"][best].tobytes()
        found += 1
    assert found >= reps // 2
    t = fscl_amd.bootstrap_times()
    assert t["total_s"] > 0.0 and t["simulate_s"] > 0.0 and t["scan_s"] > 0.0


def test_cli(built, tmp_path):
    c = sr.case("mixed")
    sim, out = tmp_path / "sim.snp", tmp_path / "out.txt"
    cmd = [str(CLI), "-f", str(c.path), "-o", str(out), "--no-scan", f"--simulate-file={sim}", f"--simulate-seed={sr.SEED}",
           f"--simulate-rep={sr.REP}"] + [f"--simulate-sweep={w}" for w in c.sweep_names]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert not out.exists()
    f, _ = draw(c)
    M = c.model
    n = np.array(M.depth_n)[M.depth_p]
    want = np.where(M.folded == 1, np.minimum(f, n - f), f)
    back = fscl_amd.load_snp_input(sim).contents
    assert back.n_snps == len(f) and back.n_chromosomes == 3
    got = np.array([(back.snps[i].chr, back.snps[i].pos, back.snps[i].obs_freq, back.sample_depths[back.snps[i].depth_p],
                     back.snps[i].folded) for i in range(back.n_snps)])
    assert (got[:, 0] == M.chrom).all() and (got[:, 1] == M.pos).all() and (got[:, 2] == want).all()
    assert (got[:, 3] == n).all() and (got[:, 4] == M.folded).all()
    # the bootstrap: reps * n_sweeps data rows and n_sweeps summary rows, after the scan's own output
    b = sr.case("boot")
    boot, reps = tmp_path / "boot.txt", 3
    name = b.sweep_names[0].split(":")[0]
    planted = [f"{name}:{b.sweeps[0][1]}:2e-4", f"{name}:{b.sweeps[0][1] // 3}:5e-5"]
    cmd = [str(CLI), "-f", str(b.path), "-o", str(out), f"--bootstrap-file={boot}", f"--bootstrap-reps={reps}",
           "--prepend-label=L"] + [f"--bootstrap-sweep={w}" for w in planted]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.exists()
    lines = [ln.split("\t") for ln in boot.read_text().splitlines()]
    assert len(lines) == 2 * reps + 2
    for k in range(2):
        blk = lines[k * (reps + 1):(k + 1) * (reps + 1)]
        assert all(ln[:3] == ["L", name, planted[k].split(":")[1]] for ln in blk)
        assert [ln[4] for ln in blk[:reps]] == [str(i) for i in range(reps)] and all(len(ln) == 8 for ln in blk[:reps])
        assert blk[reps][3:5] == ["summary", str(reps)] and len(blk[reps]) == 13
    # without --bootstrap-sweep: the --bootstrap-top scan points
    cmd = [str(CLI), "-f", str(b.path), "-o", str(out), f"--bootstrap-file={boot}", "--bootstrap-reps=1", "--bootstrap-top=2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split("\t") for ln in boot.read_text().splitlines()]
    assert len(lines) == 4 and lines[1][2] == "summary" and lines[3][2] == "summary"
    assert abs(int(lines[0][1]) - int(lines[2][1])) > GRID   # the second sweep lies outside the first one's window
