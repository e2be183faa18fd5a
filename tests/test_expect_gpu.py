"""The expected terms under the model (fsclg_expect_submit, fscl_amd_scan_expect) on the GPU.

Per-site moments and totals are compared with the NumPy restatement of tests/expect_ref.py within 64
times that restatement's own measured error (E_M1, E_M2), relative to the scales it defines; the walks,
the counts and the observed terms are compared exactly with fscl_amd.scan_sites.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import expect_ref as er
import fscl_amd
import sample_ref as sr

pytestmark = pytest.mark.gpu

ER, BINS = 81920, 24
EPS = 2.0 ** -52


def alphas_of(name):
    """The sweep's own log alpha and a 5-alpha list around it whose last walk is empty unless a site stands
    within 1 bp of the sweep (logt(0) = logt(1) = 0)."""
    la0 = math.log(sr.case(name).sweeps[0][2])
    return la0, [la0 - 3.0, la0 - 1.0, la0, la0 + 1.5, 4.0]


def call(fn, *a, **k):
    try:
        return fn(*a, **k)
    except RuntimeError as e:  # a device error: nothing more runs on the GPU in this session
        pytest.exit(f"{fn.__name__}: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def device(name):
    c = sr.case(name)
    chrom, pos, _a = c.sweeps[0]
    _la0, las = alphas_of(name)
    return call(fscl_amd.expect_runs, c.scan, c.tables, c.fsp, [(chrom, pos, las[2])], [las], BINS, ER)


@functools.lru_cache(maxsize=None)
def walks(name):
    c = sr.case(name)
    chrom, pos, _a = c.sweeps[0]
    _la0, las = alphas_of(name)
    return call(fscl_amd.scan_sites, c.scan, c.tables, [(chrom, pos, la) for la in las], ER)


def terms_by_site(h, terms):
    """The walk's terms in ascending site index (fsclg_site_hdr_t's walk order undone)."""
    t = terms[int(h["off"]):int(h["off"]) + int(h["len"])]
    nl = int(h["nl"])
    return np.concatenate([t[1:nl + 1][::-1], t[:1], t[nl + 1:]]) if len(t) else t


@pytest.mark.parametrize("name", sr.CASE_NAMES)
def test_moments_and_totals_against_the_reference(built, name):
    E = er.expect_model(name)
    la0, las = alphas_of(name)
    tot, hdr, sites = device(name)
    shdr, terms = walks(name)
    assert tot.shape == (5, BINS + 1) and len(hdr) == 5
    assert int(hdr["len"].sum()) == len(sites)
    # at log alpha 4 the walk is empty unless the nearest SNP is within 1 bp of the sweep (logt(0) = logt(1) = 0)
    d_near = abs(int(E.M.pos[int(hdr["pt"]["nearest_snp"][4])]) - int(hdr["pt"]["sweep_pos"][4]))
    assert (int(hdr["len"][4]) == 0) == (d_near > 1) and int(tot[4, BINS]["n_sites"]) == int(hdr["len"][4])
    assert int(hdr["len"][2]) >= 1000
    for k in range(5):
        h, s = hdr[k], shdr[k]
        # the walk is scan_sites' walk
        for fld in ("nl", "nr", "len"):
            assert int(h[fld]) == int(s[fld]), (name, k, fld)
        assert h["pt"]["nearest_snp"] == s["pt"]["nearest_snp"] and h["pt"]["sweep_pos"] == s["pt"]["sweep_pos"]
        n = int(h["len"])
        rec = sites[int(h["off"]):int(h["off"]) + n]
        idx = np.arange(int(h["pt"]["nearest_snp"]) - int(h["nl"]), int(h["pt"]["nearest_snp"]) + int(h["nr"]) + 1) if n else \
            np.zeros(0, dtype=np.int64)
        assert (rec["site"] == idx).all()
        obs = terms_by_site(s, terms)
        assert (rec["obs"].view(np.uint64) == obs.view(np.uint64)).all(), "obs is the site's term, bit for bit"
        x = er.walk_x(E, idx, int(h["pt"]["sweep_pos"]), las[k])
        assert (rec["x"].view(np.uint64) == x.view(np.uint64)).all()
        mom = er.site_moments(E, idx, x)
        assert mom["y_margin"].min() > 1.0 if n else True
        assert (rec["degenerate"].astype(bool) == mom["degenerate"]).all()
        assert (rec["bin"] == er.bin_of(x, BINS)).all()
        for tag in ("s", "0"):
            e1 = np.abs(rec[f"m1_{tag}"] - mom[f"m1_{tag}"])
            e2 = np.abs(rec[f"m2_{tag}"] - mom[f"m2_{tag}"])
            b1, b2 = er.tol_m1() * mom[f"scale1_{tag}"], er.tol_m2() * mom[f"scale2_{tag}"]
            if n:
                j1, j2 = int(np.argmax(e1 - b1)), int(np.argmax(e2 - b2))
                print(f"{name} alpha {k} {tag}: worst m1 error {e1[j1]:.3e} of bound {b1[j1]:.3e} (site {idx[j1]}), "
                      f"m2 {e2[j2]:.3e} of {b2[j2]:.3e} (site {idx[j2]})")
            assert (e1 <= b1).all() and (e2 <= b2).all(), (name, k, tag)
            assert np.abs(rec[f"lost_{tag}"] - mom[f"lost_{tag}"]).max(initial=0.0) <= 1e-12
        # totals: counts exactly, obs as the ascending sequential fold bit for bit, sums within the scaled bounds
        want = er.totals(mom, BINS)
        b = er.bin_of(x, BINS)
        for j in range(BINS + 1):
            o = tot[k, j]
            assert int(o["n_sites"]) == want["n_sites"][j] and int(o["n_degenerate"]) == want["n_degenerate"][j], (name, k, j)
            acc = 0.0
            for v in (obs if j == BINS else obs[b == j]):
                acc += float(v)
            assert np.float64(acc).view(np.uint64) == o["obs"].view(np.uint64), (name, k, j)
            cnt = max(want["n_sites"][j], 1)
            for tag in ("s", "0"):
                # the device folds its own site values: the sites' bounds add up, plus the fold's own rounding
                be = er.tol_m1() * want[f"se_{tag}"][j] + cnt * EPS * want[f"se_{tag}"][j]
                bv = er.GPU_FACTOR * max(er.E_M1, er.E_M2) * want[f"sv_{tag}"][j] + cnt * EPS * want[f"sv_{tag}"][j]
                assert abs(o[f"e_{tag}"] - want[f"e_{tag}"][j]) <= be, (name, k, j, tag, o[f"e_{tag}"], want[f"e_{tag}"][j], be)
                assert abs(o[f"v_{tag}"] - want[f"v_{tag}"][j]) <= bv, (name, k, j, tag, o[f"v_{tag}"], want[f"v_{tag}"][j], bv)
        if n:
            ok = ~mom["degenerate"]
            assert abs(tot[k, BINS]["max_lost_s"] - mom["lost_s"][ok].max(initial=0.0)) <= 1e-12
            assert abs(tot[k, BINS]["max_lost_0"] - mom["lost_0"][ok].max(initial=0.0)) <= 1e-12
    assert fscl_amd.expect_last_ms() > 0.0


def test_folded_sites_take_the_folded_row(built):
    """`mixed` has folded sites whose two halves differ: with the unfolded row of f in place of the folded row of
    min(f, n - f) the reference itself moves by far more than the tolerance, so the comparison above tells them apart."""
    name = "mixed"
    E = er.expect_model(name)
    _la0, las = alphas_of(name)
    _tot, hdr, sites = device(name)
    h = hdr[2]
    rec = sites[int(h["off"]):int(h["off"]) + int(h["len"])]
    idx = rec["site"].astype(np.int64)
    fold = E.M.folded[idx] != 0
    assert fold.sum() >= 100
    x = er.walk_x(E, idx, int(h["pt"]["sweep_pos"]), las[2])
    mom = er.site_moments(E, idx, x)
    saved = E.M.folded.copy()
    try:
        E.M.folded[:] = 0
        wrong = er.site_moments(E, idx, x)
    finally:
        E.M.folded[:] = saved
    gap = np.abs(wrong["m1_s"] - mom["m1_s"])[fold]
    bound = (er.tol_m1() * mom["scale1_s"])[fold]
    assert (gap > 10.0 * bound).sum() >= 50
    assert (np.abs(rec["m1_s"] - mom["m1_s"]) <= er.tol_m1() * mom["scale1_s"]).all()


@pytest.mark.parametrize("name", ["mixed", "d130"])
def test_same_bytes_alone_among_others_and_on_either_batch(built, name):
    c = sr.case(name)
    chrom, pos, _a = c.sweeps[0]
    _la0, las = alphas_of(name)
    tot, hdr, sites = device(name)
    others = [(chrom, pos + 137 * (j + 1), las[2]) for j in range(8)]
    reqs = others[:6] + [(chrom, pos, las[2])] + others[6:]
    for batch in (0, 1):
        t9, h9, s9 = call(fscl_amd.expect_runs, c.scan, c.tables, c.fsp, reqs, [las] * 9, BINS, ER, batch)
        assert t9[30:35].tobytes() == tot.tobytes(), (name, batch)
        o = int(h9["off"][30])
        assert s9[o:o + len(sites)].tobytes() == sites.tobytes(), (name, batch)
        for fld in ("nl", "nr", "len"):
            assert (h9[fld][30:35] == hdr[fld]).all()
    t1, _h1, s1 = call(fscl_amd.expect_runs, c.scan, c.tables, c.fsp, [(chrom, pos, las[2])], [las], BINS, ER, 1)
    assert t1.tobytes() == tot.tobytes() and s1.tobytes() == sites.tobytes()
    for k, la in enumerate(las):  # the alpha list one alpha at a time
        tk, hk, sk = call(fscl_amd.expect_runs, c.scan, c.tables, c.fsp, [(chrom, pos, la)], [[la]], BINS, ER)
        assert tk[0].tobytes() == tot[k].tobytes(), (name, k)
        o = int(hdr["off"][k])
        assert sk.tobytes() == sites[o:o + int(hdr["len"][k])].tobytes(), (name, k)


def test_scan_expect_inserts_the_own_alpha(built):
    """fscl_amd_scan_expect: the shared list with each request's alpha inserted in order; its tasks are the raw
    handle's, byte for byte."""
    name = "d65"
    c = sr.case(name)
    chrom, pos, _a = c.sweeps[0]
    la0, las = alphas_of(name)
    tot, hdr, _sites = device(name)
    grid = [las[0], las[1], las[3], las[4]]
    r = call(fscl_amd.scan_expect, c.scan, c.tables, c.fsp, [(chrom, pos, la0), (chrom, pos, las[1])], grid, BINS, ER)
    assert r["evaluated"] and list(r["first"]) == [0, 5, 9] and list(r["own"]) == [2, 1]
    assert list(r["la"][:5]) == las and list(r["la"][5:]) == grid
    assert r["tot"][:5].tobytes() == tot.tobytes()
    assert r["tot"][6].tobytes() == tot[1].tobytes()
    assert (r["hdr"]["len"][:5] == hdr["len"]).all()
    assert r["kernel_ms"] > 0.0


def test_sampler_agrees_with_the_expectation(built):
    """d66: the mean over 64 simulated replicates of the term sum at the truth (NumPy, from the replicate's counts)
    lies within 5 SD_sweep / sqrt(64) of E_sweep.  The replicates' sites are independent by construction, so the SD
    applies; seed and replicate numbers are fixed, so the test is deterministic."""
    name = "d66"
    c = sr.case(name)
    E = er.expect_model(name)
    M = E.M
    _la0, las = alphas_of(name)
    tot, hdr, sites = device(name)
    h = hdr[2]
    rec = sites[int(h["off"]):int(h["off"]) + int(h["len"])]
    idx = rec["site"].astype(np.int64)
    x = rec["x"]
    d = 0
    assert (M.depth_p[idx] == d).all() and not M.folded[idx].any()
    n_iv = M.coef[d].shape[1]
    iv = np.clip(np.trunc((x - er.LOG_AD_MIN) / M.step), 0, n_iv - 1).astype(np.int64)
    sums = []
    for rep in range(64):
        f, _deg = call(fscl_amd.simulate, c.scan, c.tables, c.sweeps, sr.SEED, rep)
        cf = M.coef[d][f[idx] - 1, iv, :]
        t = x * (cf[:, 0] * x * x + cf[:, 1] * x + cf[:, 2]) + cf[:, 3] - E.null_u[d][f[idx] - 1]
        assert np.isfinite(t).all()
        sums.append(float(t.sum()))
    T = tot[2, BINS]
    mean, sd = float(np.mean(sums)), math.sqrt(float(T["v_s"]))
    print(f"d66: replicate mean {mean:.4f}, E_sweep {T['e_s']:.4f}, SD_sweep {sd:.4f} (log-likelihood scale)")
    assert T["n_degenerate"] == 0 and sd > 0.0
    assert abs(mean - float(T["e_s"])) <= 5.0 * sd / math.sqrt(64.0)


def test_inputs_exercise_what_they_are_for(built):
    """d2_3 holds sites of n - 1 = 1 and 2 in its walk.  d129 has classes the background never saw (null value -inf):
    unusable under the sweep, which gives them mass (max_lost_s > 0), and without neutral mass (max_lost_0 = 0 exactly).
    asc has classes of probability 0 -- q_f = 0 and no finite spline row -- which are unusable and carry no mass under
    either spectrum: both losses are 0 to rounding."""
    _tot, hdr, sites = device("d2_3")
    E = er.expect_model("d2_3")
    rec = sites[int(hdr["off"][2]):int(hdr["off"][2]) + int(hdr["len"][2])]
    n = np.array(E.M.depth_n)[E.M.depth_p[rec["site"]]]
    assert set(np.unique(n)) == {2, 3} and not rec["degenerate"].any()
    tot, _hdr, _sites = device("d129")
    assert tot[2, BINS]["max_lost_s"] > 1e-3 and tot[2, BINS]["max_lost_0"] == 0.0
    tot, _hdr, _sites = device("asc")
    Ea = er.expect_model("asc")
    assert (Ea.q[0] <= 0.0).sum() >= 2 and np.isnan(Ea.M.coef[0]).any()
    assert tot[2, BINS]["max_lost_0"] == 0.0 and tot[2, BINS]["max_lost_s"] <= 1e-12 and tot[2, BINS]["n_degenerate"] == 0


def test_scan_point_expect_takes_the_surface_top_points(built):
    """The top-K choice: descending CLR, none within the spacing of one already taken -- the points
    scan_point_surfaces takes for the same top and halfwidth -- each at its fitted alpha."""
    c = sr.case("boot")
    call(fscl_amd.scan_chromosome, c.scan, c.tables, ER, 128, 100000)
    pts = fscl_amd.points(c.scan)
    assert len(pts) >= 20
    grid = fscl_amd.surface_alphas(-20.0, 4.0, 5)
    for top, spacing in ((4, 100000), (3, 400000), (0, 100000)):
        r = call(fscl_amd.scan_point_expect, c.scan, c.tables, c.fsp, grid, top, spacing, BINS, ER)
        sf = call(fscl_amd.scan_point_surfaces, c.scan, c.tables, top, spacing, 50000, (-20.0, 4.0, 5), ER)
        want = [int(s.hdr["point"]) for s in sf]
        assert list(r["point"]) == want and len(want) == top
        for i, k in enumerate(want):
            assert r["req"]["pos"][i] == pts["sweep_pos"][k] and r["req"]["lalpha"][i] == pts["lalpha"][k]
            own = int(r["first"][i] + r["own"][i])
            assert r["la"][own] == pts["lalpha"][k]
            # obs of the walk at the fitted alpha: the point's CLR but for the order of addition
            assert abs(2.0 * r["tot"][own, BINS]["obs"] - pts["clr"][k]) <= 1e-9 * max(1.0, abs(pts["clr"][k]))
        if top == 3:
            pos = sorted(int(p) for p in r["req"]["pos"])
            assert all(b - a > spacing for a, b in zip(pos, pos[1:]))


def test_cli_end_to_end(built, tmp_path):
    """`mixed` through the CLI: the file parses, the summary's obs is the --sites-file total of the same point, and the
    -o output (with a permutation test, so the rand() stream too) is byte-identical with and without --expect-file."""
    import subprocess

    from util import CLI
    c = sr.case("mixed")
    base = [str(CLI), "-f", str(c.path), "--n-permute=5", "-v", "0"]
    o1, o2, ef, sf = (tmp_path / n for n in ("o1.txt", "o2.txt", "e.txt", "s.txt"))
    for cmd in (base + ["-o", str(o1)],
                base + ["-o", str(o2), f"--expect-file={ef}", f"--sites-file={sf}", "--expect-bins=12", "--prepend-label=L"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            pytest.exit(f"fscl exited {r.returncode}: {r.stderr[-500:]}", returncode=3)
    strip = lambda t: "\n".join(l[2:] if l.startswith("L\t") else l for l in t.splitlines())  # noqa: E731
    assert strip(o2.read_text()) == strip(o1.read_text()) and o1.stat().st_size > 0
    site_tot = {}
    n_terms = {}
    for l in sf.read_text().splitlines():
        f = l.split("\t")[1:]
        if f[2] != "summary":
            site_tot[(f[0], f[1])] = site_tot.get((f[0], f[1]), 0.0) + float(f[8])
            n_terms[(f[0], f[1])] = n_terms.get((f[0], f[1]), 0) + 1
    rows = [l.split("\t") for l in ef.read_text().splitlines()]
    assert all(r[0] == "L" for r in rows)
    rows = [r[1:] for r in rows]
    summ = [r for r in rows if r[3] == "summary"]
    assert len(summ) == 3 and all(len(r) == 15 for r in summ)
    for r in rows:
        assert len(r) == {"bin": 14, "curve": 11, "summary": 15}[r[3]]
        assert all(v == "NA" or np.isfinite(float(v)) for v in r[4:])
    for r in summ:
        key = (r[0], r[1])
        mine = [q for q in rows if (q[0], q[1]) == key]
        bins = [q for q in mine if q[3] == "bin"]
        assert 1 <= len(bins) <= 12 and len([q for q in mine if q[3] == "curve"]) in (33, 34)
        assert sum(int(q[6]) for q in bins) == int(r[4]) == n_terms[key]
        # the sites file prints each term with four decimals: the totals agree to that rounding
        assert abs(float(r[6]) - 2.0 * site_tot[key]) <= 2.0 * n_terms[key] * 5e-5 + 1e-4, (key, r[6], site_tot[key])
