"""The host side of the sweep-model simulation and the bootstrap (no GPU): the uniform draw, the
nearest-sweep rule, the reference's own decidedness on every GPU input, the replicate scan and its
file, the bootstrap's quantile summary, and the CLI's refusals."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import fscl_amd
import sample_ref as sr
from util import GOLD, run_cli

NAN = math.nan


def test_exports_and_layout(built):
    L = fscl_amd.get_lib()
    for name in ("fsclg_sample_tables", "fsclg_sample_submit", "fsclg_sample_wait", "fsclg_sample_last_ms",
                 "fscl_amd_simulate", "fscl_amd_simulate_scan", "fscl_amd_scan_free", "fscl_amd_simulate_output",
                 "fscl_amd_bootstrap", "fscl_amd_bootstrap_output", "fscl_amd_parse_sweep", "fscl_amd_nearest_sweep"):
        assert hasattr(L, name)
    assert fscl_amd.SWEEP_DTYPE.itemsize == 16 and fscl_amd.BOOT_DTYPE.itemsize == 48


def test_uniform_draw(built):
    assert sr.mix64_py(0) == 0xE220A8397B1DCDAF  # splitmix64's first output for the seed 0
    for seed, rep in ((0, 0), (0xFD821A6, 0), (sr.SEED, sr.REP), (2 ** 64 - 1, 2 ** 31 - 1), (12345, -1)):
        u = sr.uniforms(seed, rep, 70000)
        for i in (0, 1, 63, 64, 4095, 65535, 65536, 69999):
            assert float(u[i]) == sr.uniform_py(seed, rep, i)
        assert 0.0 <= u.min() and u.max() < 1.0
    # the prune draw's constant is another one: the two streams are unrelated
    a = sr.mix64_py(sr.mix64_py(7 ^ sr.SAMPLE_KEY) ^ 5)
    b = sr.mix64_py(sr.mix64_py(7 ^ 0x632BE59BD9B4E019) ^ 5)
    assert a != b
    assert sr.uniform_py(1, 0, 5) != sr.uniform_py(1, 1, 5) != sr.uniform_py(2, 1, 5)


def test_nearest_sweep_rule(built):
    sweeps = [(0, 1000, 1e-3), (0, 3000, 2e-3), (2, 500, 1e-4), (0, 3000, 9e-3), (0, 2000, 5e-3)]
    cases = [(0, 0), (0, 1499), (0, 1500), (0, 1501), (0, 2500), (0, 2600), (0, 10 ** 9), (0, -5), (1, 1000), (2, 7),
             (3, 7), (0, 3000)]
    for c, p in cases:
        assert fscl_amd.nearest_sweep(sweeps, c, p) == sr.nearest_sweep(sweeps, c, p), (c, p)
    assert fscl_amd.nearest_sweep(sweeps, 0, 1500) == 0      # equidistant from 1000 and 2000: the lower position
    assert fscl_amd.nearest_sweep(sweeps, 0, 2500) == 4      # equidistant from 2000 and 3000
    assert fscl_amd.nearest_sweep(sweeps, 0, 3000) == 1      # two sweeps on one position: the first given
    assert fscl_amd.nearest_sweep(sweeps, 1, 1000) == -1     # a chromosome without a sweep
    assert fscl_amd.nearest_sweep([], 0, 1000) == -1
    # the vectorised rule of the reference is the scalar one
    M = sr.case("mixed").model
    x, which = sr.site_log_ad(M, sr.case("mixed").sweeps)
    for i in list(range(0, len(M.pos), 97)) + [1001 + 400]:
        assert which[i] == sr.nearest_sweep(sr.case("mixed").sweeps, M.chrom[i], M.pos[i])
    assert which[1001 + 400] == 2 and (which[2002:] == -1).all() and np.isnan(x[2002:]).all()
    assert x[500] == math.log(sr.ALPHA)                      # d = 0: log_ad = lalpha, as sm_likelihood


@pytest.mark.parametrize("name", sr.CASE_NAMES)
def test_inputs_leave_no_site_undecided(built, name):
    """The condition of the GPU tests' equality: the reference alone decides every site of every input,
    with the sweeps and as a neutral replicate."""
    c = sr.case(name)
    M = c.model
    for neutral in (False, True):
        d = sr.reference(name, neutral)
        assert d.undecided == 0, f"{name}: {d.undecided} undecided sites (margin {d.margin.min()!r})"
        n = np.array(M.depth_n)[M.depth_p]
        assert ((d.f >= 1) & (d.f <= n - 1)).all()
    d, d0 = sr.reference(name), sr.reference(name, True)
    near = d.log_ad <= sr.LOG_AD_MAX
    assert d.swept.sum() == near.sum() >= 300
    assert int((d.f[near] != d0.f[near]).sum()) >= 100, f"{name}: the sweeps change too few sites to show the sweep branch"
    if name == "d2_3":
        assert sorted(M.depth_n) == [2, 3]
    if name == "mixed":
        assert len(M.pos) % 4 != 0 and len(M.depth_n) == 2 and 0.2 < M.folded.mean() < 0.4
    if name == "asc":   # singletons are unascertainable under a minimum of 2: probability 0, never drawn
        assert M.fsp[0][0] == 0.0 and (sr.reference(name).p_drawn > 0.0).all()


POS = [100 * (i + 1) for i in range(10)]
FREQ = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3]
DEPTH_P = [0, 1, 0, 1, 0, 0, 1, 1, 0, 0]
FOLDED = [0, 0, 1, 0, 0, 1, 0, 0, 1, 0]
DEPTHS = [20, 12]
CHROM = [0] * 6 + [1] * 4


def fake_scan():
    snps = (fscl_amd.SnpT * len(POS))()
    for i, q in enumerate(snps):
        q.chr, q.pos, q.obs_freq, q.depth_p, q.folded, q.null_logl = CHROM[i], POS[i], FREQ[i], DEPTH_P[i], FOLDED[i], -1.5
    lim = (fscl_amd.ChrLimitsT * 2)()
    lim[0].chr, lim[0].name, lim[0].start_index, lim[0].n_snps, lim[0].start_pos, lim[0].bp_length = 0, b"chrA", 0, 6, 100, 600
    lim[1].chr, lim[1].name, lim[1].start_index, lim[1].n_snps, lim[1].start_pos, lim[1].bp_length = 1, b"b:2", 6, 4, 700, 1000
    depths = (C.c_int * 2)(*DEPTHS)
    s = fscl_amd.ScanT()
    s.n_snps, s.snps, s.n_depths, s.sample_depths = len(POS), snps, 2, depths
    s.chr_limits, s.n_chromosomes = lim, 2
    return C.pointer(s), (snps, lim, depths)


def test_simulate_scan_folds_and_round_trips(built, tmp_path):
    scan, keep = fake_scan()
    freq = [19, 11, 17, 6, 1, 10, 7, 1, 3, 12]
    want = [19, 11, 3, 6, 1, 10, 7, 1, 3, 12]   # folded sites 2, 5, 8: min(f, n - f)
    r = fscl_amd.simulate_scan(scan, freq)
    q = r.contents
    assert (q.n_snps, q.n_depths, q.n_chromosomes, q.n_scan_pts, bool(q.scan_pts)) == (10, 2, 2, 0, False)
    assert [q.snps[i].obs_freq for i in range(10)] == want
    for i in range(10):
        assert (q.snps[i].chr, q.snps[i].pos, q.snps[i].depth_p, q.snps[i].folded) == (CHROM[i], POS[i], DEPTH_P[i], FOLDED[i])
        assert q.snps[i].null_logl == 0.0
    assert C.addressof(q.snps.contents) != C.addressof(scan.contents.snps.contents)
    assert [q.sample_depths[d] for d in range(2)] == DEPTHS
    for c in range(2):
        a, b = q.chr_limits[c], scan.contents.chr_limits[c]
        assert (a.name, a.start_index, a.n_snps, a.start_pos, a.bp_length) == (b.name, b.start_index, b.n_snps, b.start_pos, b.bp_length)
    out = tmp_path / "rep.snp"
    fscl_amd.simulate_output(out, r)
    lines = out.read_text().splitlines()
    assert lines[0] == "chrA 100 19 20 0" and lines[2] == "chrA 300 3 20 1" and lines[6] == "b:2 700 7 12 0"
    back = fscl_amd.load_snp_input(out).contents
    assert back.n_snps == 10 and back.n_chromosomes == 2
    for i in range(10):
        p = back.snps[i]
        assert (p.chr, p.pos, p.obs_freq, back.sample_depths[p.depth_p], p.folded) == \
            (CHROM[i], POS[i], want[i], DEPTHS[DEPTH_P[i]], FOLDED[i])
    assert [back.chr_limits[c].name for c in range(2)] == [b"chrA", b"b:2"]
    fscl_amd.scan_free(r)
    with pytest.raises(ValueError):
        fscl_amd.simulate_scan(scan, freq[:-1])
    del keep


def test_parse_sweep(built):
    scan, keep = fake_scan()
    assert fscl_amd.parse_sweep(scan, "chrA:250:1e-4") == (0, 250, 1e-4)
    assert fscl_amd.parse_sweep(scan, "b:2:900:0.5") == (1, 900, 0.5)   # the last two colons separate
    for bad, what in (("chrB:250:1e-4", "unknown chromosome"), ("chrA:250:0", "alpha must be positive"),
                      ("chrA:250:-1e-4", "alpha must be positive"), ("chrA:250:nan", "alpha must be positive"),
                      ("chrA:250:inf", "alpha must be positive"), ("chrA:250", "expected"), ("chrA:x:1e-4", "expected"),
                      ("chrA:250:1e-4x", "expected"), (":250:1e-4", "expected"), ("chrA:2.5:1e-4", "expected"), ("", "expected")):
        with pytest.raises(ValueError, match=what):
            fscl_amd.parse_sweep(scan, bad)
    del keep


def boot_rows(spec):
    """BOOT_DTYPE rows from per sweep (chr, planted_pos, planted_alpha, [(est_pos, alpha, clr) or None per rep])."""
    reps = len(spec[0][3])
    rows = np.zeros(len(spec) * reps, dtype=fscl_amd.BOOT_DTYPE)
    for k, (c, p, a, est) in enumerate(spec):
        for r, e in enumerate(est):
            q = rows[k * reps + r]
            q["sweep"], q["rep"], q["chr"], q["planted_pos"], q["planted_alpha"] = k, r, c, p, a
            q["est_pos"], q["est_lalpha"], q["clr"] = (-1, NAN, NAN) if e is None else (e[0], math.log(e[1]), e[2])
    return rows, reps


def test_bootstrap_output_and_quantiles(built, tmp_path):
    scan, keep = fake_scan()
    est = [(450, 2e-3, 30.5), None, (250, 1e-3, 12.25), (350, 8e-3, 20.0), (300, 4e-3, 50.0), (200, 5e-3, 8.0)]
    sweeps = [(0, 300, 3e-3), (1, 800, 1e-4), (0, 500, 1.0)]
    rows, reps = boot_rows([(0, 300, 3e-3, est), (1, 800, 1e-4, [None] * 6),
                            (0, 500, 1.0, [(510, 1.0, 1.0)] + [None] * 5)])
    out = tmp_path / "boot.txt"
    fscl_amd.bootstrap_output(out, scan, sweeps, reps, rows)
    got = out.read_text().splitlines()
    assert len(got) == 3 * (reps + 1)
    assert got[0] == "chrA\t300\t3.000e-03\t0\t450\t2.000e-03\t30.50"
    assert got[1] == "chrA\t300\t3.000e-03\t1\tNA\tNA\tNA"
    assert got[5] == "chrA\t300\t3.000e-03\t5\t200\t5.000e-03\t8.00"
    # five found: sorted[floor(q * 4)] = sorted[0], sorted[2], sorted[3], each column on its own
    assert got[6] == ("chrA\t300\tsummary\t6\t5\t200\t300\t350\t1.000e-03\t4.000e-03\t5.000e-03\t20.00")
    assert got[7] == "b:2\t800\t1.000e-04\t0\tNA\tNA\tNA"
    assert got[13] == "b:2\t800\tsummary\t6\t0\tNA\tNA\tNA\tNA\tNA\tNA\tNA"
    assert got[14] == "chrA\t500\t1.000e+00\t0\t510\t1.000e+00\t1.00"
    assert got[20] == "chrA\t500\tsummary\t6\t1\t510\t510\t510\t1.000e+00\t1.000e+00\t1.000e+00\t1.00"   # one found: every quantile
    fscl_amd.bootstrap_output(out, scan, sweeps[1:2], reps, rows[reps:2 * reps], label="run7")
    got = out.read_text().splitlines()
    assert got[0] == "run7\tb:2\t800\t1.000e-04\t0\tNA\tNA\tNA" and got[-1].startswith("run7\tb:2\t800\tsummary\t6\t0\tNA")
    # the quantile index at other counts: floor(q * (n - 1))
    for n in (2, 3, 40, 41, 100):
        e = [(1000 + i, 1e-3 * (i + 1), float(i)) for i in range(n)]
        rows, reps = boot_rows([(0, 300, 3e-3, e[::-1])])
        fscl_amd.bootstrap_output(out, scan, sweeps[:1], reps, rows)
        f = out.read_text().splitlines()[-1].split("\t")
        idx = [math.floor(q * (n - 1)) for q in (0.025, 0.5, 0.975)]
        assert f[2:5] == ["summary", str(n), str(n)] and f[5:8] == [str(1000 + i) for i in idx]
        assert f[8:11] == ["%1.3e" % (1e-3 * (i + 1)) for i in idx] and f[11] == "%1.2f" % idx[1]
    with pytest.raises(ValueError):
        fscl_amd.bootstrap_output(out, scan, sweeps, reps, rows)
    del keep


def test_cli_refusals(built, tmp_path):
    b, s = tmp_path / "b.txt", tmp_path / "s.txt"
    for args, env, msg in (
            ([f"--bootstrap-file={b}", "--no-scan"], None, "--bootstrap-file with --no-scan needs --bootstrap-sweep"),
            ([f"--bootstrap-file={b}", "--scan-mode=grid"], None, "--bootstrap-file rescans by bisection"),
            ([f"--bootstrap-file={b}"], {"WORLD_SIZE": "2", "RANK": "0"}, "--bootstrap-file runs in one process"),
            ([f"--bootstrap-file={b}", "--bootstrap-sweep=no_such_chromosome:5000:1e-4"], None, "unknown chromosome name"),
            ([f"--simulate-file={s}", "--no-scan", "--simulate-sweep=no_such_chromosome:5000:1e-4"], None,
             "unknown chromosome name"),
            ([f"--bootstrap-file={b}", "--bootstrap-sweep=anything:5000:0"], None, "alpha must be positive"),
            ([f"--simulate-file={s}", "--simulate-sweep=anything:5000:-2e-4"], None, "alpha must be positive"),
            ([f"--bootstrap-file={b}", "--bootstrap-reps=-1"], None, "--bootstrap-reps must be >= 0")):
        r = run_cli(args, tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr + r.stdout, (args, r.returncode, r.stderr[-400:])
        assert not b.exists() and not s.exists() and not (tmp_path / "o.txt").exists()
    with pytest.raises(ValueError):
        fscl_amd.run(GOLD / "g2.snp", None, bootstrap_file=b, scan_mode="grid")
