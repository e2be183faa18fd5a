"""The host side of the family-wise adjusted p-values (no GPU): the combine on crafted counts (the rank order with
ties, the monotone step-down, the threshold rule and its agreement with p_single <= a, k = 0), the restatement of
tests/maxt_ref.py against a brute-force reading of the definitions, the --familywise-file writer byte for byte, the
stand-alone sanitizer check, and every refusal of the CLI and of run()."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import fscl_amd
import maxt_ref as mr
from util import GOLD, ROOT, run_cli, run_host_check


def test_exports(built):
    L = fscl_amd.get_lib()
    for name in ("fsclg_maxt_submit", "fsclg_maxt_wait", "fsclg_maxt_last_ms", "fscl_amd_familywise", "fscl_amd_familywise_runs",
                 "fscl_amd_familywise_combine", "fscl_amd_familywise_output", "fscl_amd_familywise_last_ms"):
        assert hasattr(L, name)
    assert (fscl_amd.MAXT_WG, fscl_amd.MAXT_TILE) == (mr.WG, mr.TILE)
    hdr = (ROOT / "include" / "fsclg.h").read_text()
    assert f"#define FSCLG_MAXT_WG {mr.WG}" in hdr and f"#define FSCLG_MAXT_TILE {mr.TILE}" in hdr
    assert f"#define FSCLG_MAXT_MAX_GROUPS {fscl_amd.MAXT_MAX_GROUPS}" in hdr


def test_rank_order_with_ties(built):
    obs = [3.0, 12.5, 3.0, 0.0, 40.0, 12.5, 0.0, math.nan, -1.0, math.inf]
    want = [9, 4, 1, 5, 0, 2, 3, 6, 8, 7]
    assert fscl_amd.familywise_order(obs).tolist() == want == mr.order_of(obs).tolist()
    g = np.random.default_rng(1)
    x = g.choice([0.0, 0.0, 1.5, 7.0], size=500)
    assert fscl_amd.familywise_order(x).tobytes() == mr.order_of(x).tobytes()
    assert len(fscl_amd.familywise_order([])) == 0


def test_restatement_against_brute_force(built):
    """maxt_ref.kernel, which the GPU is held to bit for bit, against loops that read the definitions literally."""
    g = np.random.default_rng(2)
    m, nt, G = 37, 6, 4
    T = g.choice([0.0, 0.0, 0.5, 2.0, 7.5, math.nan], size=(nt, m))
    T[3, :] = math.nan
    obs = g.choice([0.0, 0.5, 2.0, 9.0], size=m)
    grp = np.sort(g.choice([0, 1, 3], size=m)).astype(np.int32)   # group 2 is empty
    order = mr.order_of(obs)
    res = mr.kernel(T, obs, order, grp, G)
    for t in range(nt):
        vals = [(T[t, i], i) for i in range(m) if not math.isnan(T[t, i])]
        mx = max((v for v, _ in vals), default=-math.inf)
        assert res["gmax"][t] == mx and res["garg"][t] == min((i for v, i in vals if v == mx), default=-1)
        for c in range(G):
            sub = [(v, i) for v, i in vals if grp[i] == c]
            cm = max((v for v, _ in sub), default=-math.inf)
            assert res["chr_max"][t, c] == cm and res["chr_arg"][t, c] == min((i for v, i in sub if v == cm), default=-1)
    for j, i in enumerate(order):
        later = set(order[j:].tolist())
        cs = cc = ct = 0
        for t in range(nt):
            cs += res["gmax"][t] >= obs[i]
            cc += res["chr_max"][t, grp[i]] >= obs[i]
            ct += max((T[t, k] for k in later if not math.isnan(T[t, k])), default=-math.inf) >= obs[i]
        assert (res["c_single"][i], res["c_chr"][i], res["c_step"][i]) == (cs, cc, ct), (j, i)
    assert (res["chr_max"][:, 2] == -math.inf).all() and (res["chr_arg"][:, 2] == -1).all() and res["garg"][3] == -1
    # the crafted GPU fixtures cover what they claim
    names = {c[0] for c in mr.cases()}
    for m_ in (1, 63, 64, 65, mr.WG - 1, mr.WG, mr.WG + 1, 2 * mr.TILE + 1):
        assert {f"m{m_}_t1_g1", f"m{m_}_t5_g22"} <= names
    for name, T_, obs_, grp_, G_ in mr.cases():
        assert T_.shape[1] == len(obs_) == len(grp_) and (len(grp_) == 0 or grp_.max() < G_)
        if G_ == 22:
            assert 7 not in set(grp_.tolist())


def test_combine_monotone_step_down(built):
    obs = [3.0, 12.5, 3.0, 0.0, 40.0]
    order = fscl_amd.familywise_order(obs)
    cs, cc, ct = [17, 7, 17, 19, 0], [16, 6, 16, 19, 0], [1, 2, 5, 19, 0]
    got = fscl_amd.familywise_combine(cs, cc, ct, order, 19)
    assert got["rank"].tolist() == [3, 2, 4, 5, 1]
    assert got["p_single"].tolist() == [18 / 20, 8 / 20, 18 / 20, 1.0, 1 / 20]
    assert got["p_chr"].tolist() == [17 / 20, 7 / 20, 17 / 20, 1.0, 1 / 20]
    assert got["p_step"].tolist() == [3 / 20, 3 / 20, 6 / 20, 1.0, 1 / 20]   # rank 3 is lifted to rank 2's value
    want = mr.combine(cs, cc, ct, order, 19)
    for k in ("rank", "p_single", "p_chr", "p_step"):
        assert got[k].tobytes() == want[k].astype(got[k].dtype).tobytes()
    with pytest.raises(ValueError):
        fscl_amd.familywise_combine(cs, cc, ct, [0, 1, 2, 3, 3], 19)
    with pytest.raises(ValueError):
        fscl_amd.familywise_combine(cs, cc, ct, order, 0)


@pytest.mark.parametrize("M", [1, 8, 9, 19, 20, 39, 99, 100, 199, 1000])
def test_threshold_rule_agrees_with_p_single(built, M):
    g = np.random.default_rng(M)
    maxima = g.choice([0.0, 1.0, 2.5, 2.5, 4.0, 7.0, 11.0], size=M) + g.integers(0, 3, size=M)
    obs = np.concatenate([np.unique(maxima), np.unique(maxima) + 0.25, [0.0, 100.0]])
    c = np.array([(maxima >= x).sum() for x in obs], dtype=np.int32)
    p = fscl_amd.familywise_combine(c, c, c, fscl_amd.familywise_order(obs), M)["p_single"]
    for a in (0.10, 0.05, 0.01):
        k, thr = fscl_amd.familywise_threshold(maxima, a)
        assert (k, thr) == mr.threshold(maxima, a)
        assert k == int(math.floor(a * (M + 1) + 1e-9)) and k <= M
        if k == 0:
            assert thr is None and not (p <= a).any()   # 1 / (M + 1) > a: nothing can be significant
        else:
            assert thr == np.sort(maxima)[::-1][k - 1]
            assert ((obs > thr) == (p <= a)).all(), (M, a, k, thr)
    assert fscl_amd.familywise_threshold([], 0.05) == (0, None)


POS = [1000, 2500, 4000, 900, 5000]
CLR = [3.0, 12.345, 3.0, 0.0, 40.5]
LA = [math.log(1e-3), math.log(2.5e-2), 0.0, -20.0, math.log(7.0)]
CHR = [0, 0, 0, 1, 1]


def fake_scan():
    pts = (fscl_amd.ScanPtT * 5)()
    for i, q in enumerate(pts):
        q.chr, q.sweep_pos, q.clr, q.lalpha = CHR[i], POS[i], CLR[i], LA[i]
    lim = (fscl_amd.ChrLimitsT * 2)()
    lim[0].chr, lim[0].name = 0, b"chrA"
    lim[1].chr, lim[1].name = 1, b"chrB"
    s = fscl_amd.ScanT()
    s.n_scan_pts, s.scan_pts, s.chr_limits, s.n_chromosomes = 5, pts, lim, 2
    return C.pointer(s), (pts, lim)


def test_output_format(built, tmp_path):
    scan, keep = fake_scan()
    M = 19
    gmax = np.array([30.0 if t == 4 else float(t) for t in range(M)])
    chr_max = np.stack([np.arange(M, dtype=np.float64), np.where(np.arange(M) == 3, -np.inf, 0.5 * np.arange(M))], axis=1)
    res = {"order": fscl_amd.familywise_order(CLR), "c_single": [17, 7, 17, 19, 0], "c_chr": [16, 6, 16, 19, 0],
           "c_step": [1, 2, 5, 19, 0], "gmax": gmax, "garg": [(-1 if t == 3 else t % 5) for t in range(M)], "chr_max": chr_max,
           "chr_arg": [[0, -1 if t == 3 else 3] for t in range(M)], "trials": M}
    out = tmp_path / "fw.txt"
    fscl_amd.familywise_output(out, scan, res)
    got = out.read_text().splitlines()
    assert got == ["chrA\t1000\t3.00\t1.000e-03\t3\t8.500e-01\t9.000e-01\t1.500e-01\t0.824",
                   "chrA\t2500\t12.35\t2.500e-02\t2\t3.500e-01\t4.000e-01\t1.500e-01\t0.824",
                   "chrA\t4000\t3.00\t1.000e+00\t4\t8.500e-01\t9.000e-01\t3.000e-01\t0.523",
                   "chrB\t900\t0.00\t2.061e-09\t5\t1.000e+00\t1.000e+00\t1.000e+00\t0.000",
                   "chrB\t5000\t40.50\t7.000e+00\t1\t5.000e-02\t5.000e-02\t5.000e-02\t1.301",
                   "chrA\tsummary\t19\t3\t9.00\t17.00\t18.00\tNA\t0\t0",
                   "chrB\tsummary\t19\t2\t4.50\t8.50\t9.00\tNA\t1\t0",
                   "genome\tsummary\t19\t5\t10.00\t18.00\t30.00\tNA\t1\t0"]
    want = mr.output_rows(["chrA", "chrB"], CHR, POS, CLR, LA, res, M)
    assert [ln.split("\t") for ln in got] == want
    fscl_amd.familywise_output(out, scan, res, label="run7")
    assert [ln.split("\t") for ln in out.read_text().splitlines()] == mr.output_rows(["chrA", "chrB"], CHR, POS, CLR, LA, res, M, "run7")
    nul = tmp_path / "null.txt"
    fscl_amd.familywise_null_output(nul, scan, res, label="run7")
    rows = nul.read_text().splitlines()
    assert len(rows) == M
    assert rows[0] == "run7\t0\t0.0000\tchrA\t1000\t0.0000\t0.0000"
    assert rows[3] == "run7\t3\t3.0000\tNA\tNA\t3.0000\tNA"
    assert rows[4] == "run7\t4\t30.0000\tchrB\t5000\t4.0000\t2.0000"
    bad = dict(res, c_step=[1, 2, 5, 19])
    with pytest.raises(ValueError):
        fscl_amd.familywise_output(out, scan, bad)
    with pytest.raises(ValueError):
        fscl_amd.familywise_output(out, scan, dict(res, trials=18))
    with pytest.raises(OSError):
        fscl_amd.familywise_output(tmp_path / "no_such_dir" / "t.txt", scan, res)
    del keep


def test_chunk_and_cap_refusal(built, monkeypatch):
    assert fscl_amd.familywise_chunk(10, 5, 80) == 1 and fscl_amd.familywise_chunk(10, 5, 79) == 0
    assert fscl_amd.familywise_chunk(10, 5, 10 ** 6) == 5 and fscl_amd.familywise_chunk(50006, 1000) == (1 << 28) // (8 * 50006)
    monkeypatch.setenv("FSCL_AMD_FWER_CAP", "31")
    assert fscl_amd.familywise_chunk(4, 3) == 0
    # refused before the device is opened: one trial of 4 points needs 32 bytes
    with pytest.raises(ValueError, match="FSCL_AMD_FWER_CAP=31"):
        fscl_amd.familywise_runs(np.zeros((3, 4)), np.zeros(4), np.zeros(4, np.int32), 1)
    with pytest.raises(ValueError):
        fscl_amd.familywise_runs(np.zeros((3, 4)), np.zeros(5), np.zeros(4, np.int32), 1)


def test_host_check_under_sanitizers(built, tmp_path):
    """tools/familywise_host_check.c: the order, the chunk, the refusals, the combine, the thresholds and the writers
    under ASan and UBSan, as a stand-alone program (no device library, nothing loaded into Python)."""
    run_host_check("familywise_host_check", ["familywise.c", "util.c"], tmp_path, [tmp_path])


def test_cli_refusals(built, tmp_path):
    t = tmp_path / "fw.txt"
    for args, env, msg in (
            (["--familywise-trials=10"], None, "need --familywise-file"),
            (["--familywise-seed=5"], None, "need --familywise-file"),
            ([f"--familywise-null-file={tmp_path / 'n.txt'}"], None, "need --familywise-file"),
            ([f"--familywise-file={t}", "--no-scan"], None, "--familywise-file needs the scan"),
            ([f"--familywise-file={t}", "--scan-mode=grid", "-g", "5000"], None, "not with --scan-mode=grid"),
            ([f"--familywise-file={t}"], {"WORLD_SIZE": "2", "RANK": "0"}, "--familywise-file runs in one process"),
            ([f"--familywise-file={t}", "--familywise-trials=0"], None, "--familywise-trials must be an integer >= 1"),
            ([f"--familywise-file={t}", "--familywise-trials=ten"], None, "--familywise-trials must be an integer >= 1"),
            ([f"--familywise-file={t}", "--familywise-trials=2.5"], None, "--familywise-trials must be an integer >= 1"),
            # g1 has 30 cells: one trial needs 240 bytes; refused once the data is loaded, before any device work
            ([f"--familywise-file={t}"], {"FSCL_AMD_FWER_CAP": "239"}, "FSCL_AMD_FWER_CAP=239")):
        r = run_cli(args, tmp_path, env, snp="g1.snp")
        assert r.returncode != 0 and msg in r.stderr + r.stdout, (args, r.returncode, r.stderr[-400:])
        assert not t.exists() and not (tmp_path / "o.txt").exists()
    scan = fscl_amd.load_snp_input(GOLD / "g1.snp")
    L = fscl_amd.get_lib()
    assert L.fscl_amd_familywise_check(scan, 100000, 8) == 0
    assert L.fscl_amd_familywise_check(scan, 100000, 0) == -1 and b"--familywise-trials" in L.fscl_amd_familywise_error()
    for kw in (dict(familywise_trials=10), dict(familywise_seed=5), dict(familywise_null_file=t),
               dict(familywise_file=t, familywise_trials=0), dict(familywise_file=t, scan_mode="grid")):
        with pytest.raises(ValueError):
            fscl_amd.run(GOLD / "g1.snp", None, **kw)
