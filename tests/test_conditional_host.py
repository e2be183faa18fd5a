"""The host-only side of the conditional sweep scan (csrc/host/conditional.c): the sites a candidate owns against
brute force, the base fold, the writer, the refusals that come before any device work, and
tools/conditional_host_check.c under the sanitizers.  It also pins the NumPy restatement tests/cond_ref.py, which
the GPU tests compare the kernel with.  No GPU."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import cond_ref as cr
import fscl_amd
import walk_ref as wr
from fscl_amd import synth
from util import GOLD, run_cli, run_host_check

NAN = float("nan")


@pytest.fixture(scope="module")
def scan(built, tmp_path_factory):
    """Three chromosomes; the first has runs of sites at consecutive positions (the de-collision), the later ones too
    (where the reference's rule never de-collides)."""
    rng = np.random.default_rng(11)
    chrs = []
    for name, pos, k, nn, fold in synth.generate(n_chr=3, chr_len=40_000, snps_per_chr=120, n=12, seed=77):
        pos, k, nn, fold = (np.asarray(v) for v in (pos, k, nn, fold))
        pick = np.flatnonzero(rng.integers(0, 9, len(pos)) == 0)  # a site one and two bp after about every 9th site
        add = np.concatenate([pos[pick] + 1, pos[pick] + 2])
        src = np.concatenate([pick, pick])
        keep = ~np.isin(add, pos)
        allpos, first = np.unique(np.concatenate([pos, add[keep]]), return_index=True)
        idx = np.concatenate([np.arange(len(pos)), src[keep]])[first]
        chrs.append((name, allpos, k[idx], nn[idx], fold[idx]))
    path = tmp_path_factory.mktemp("cond") / "c.snp"
    synth.write_snp_file(str(path), chrs)
    fscl_amd.get_lib().configure_logmsg(1)
    return fscl_amd.load_snp_input(path)


def layout(scan):
    s = scan.contents
    pos = np.array([s.snps[i].pos for i in range(s.n_snps)], dtype=np.int64)
    return pos, [s.chr_limits[c].start_index for c in range(s.n_chromosomes)], [s.chr_limits[c].n_snps for c in range(s.n_chromosomes)]


def test_fixture_has_what_the_cases_need(scan):
    pos, cs, cn = layout(scan)
    assert len(cs) == 3 and all(n > 100 for n in cn)
    for c in range(3):
        p = pos[cs[c]:cs[c] + cn[c]]
        assert (np.diff(p) > 0).all() and (np.diff(p) == 1).any(), "no sites at consecutive positions"


def test_clip_against_brute_force(scan):
    """Random candidates and given sweeps on every chromosome: candidates on sites (de-collided only where the
    global index is below the chromosome's count: the reference's comparison, never on the last chromosome here), between sites, beyond
    the ends; one, two and five given sweeps, none on a side, some equal to the candidate."""
    pos, cs, cn = layout(scan)
    rng = np.random.default_rng(5)
    moved = [0, 0, 0]
    for c in range(3):
        p = pos[cs[c]:cs[c] + cn[c]]
        cands = [int(x) for x in rng.choice(p, 40)] + [int(x) for x in rng.integers(p[0] - 500, p[-1] + 500, 40)]
        for x in cands:
            for ng in (0, 1, 2, 5):
                gp = [int(v) for v in rng.integers(p[0] - 200, p[-1] + 200, ng)]
                if ng == 2:
                    gp[1] = int(rng.choice(p))
                given = [(c, q, 1e-3) for q in gp] + [((c + 1) % 3, x, 1e-3)]  # (another chromosome's: skipped)
                sp, lo, hi = fscl_amd.cond_clip(scan, given, c, x)
                near, want_sp, _, _ = cr.init_point(pos, cs[c], cn[c], x, 50)
                assert sp == want_sp, (c, x)
                moved[c] += sp != x
                wl, wh = cr.clip(pos, cs[c], cn[c], gp, sp)
                assert (lo > hi and wl > wh) or (lo, hi) == (wl, wh), (c, x, gp, (lo, hi), (wl, wh))
    # (the second chromosome's first sites may still have a global index below its own count)
    assert moved[0] > 0 and moved[2] == 0 and cs[2] >= cn[2], moved


def test_clip_tie_rule_and_edges(scan):
    pos, cs, cn = layout(scan)
    c = 1
    p = pos[cs[c]:cs[c] + cn[c]]
    i = int(np.flatnonzero(np.diff(p) >= 4)[3])
    x = int(p[i])  # a site with room on either side: s = x - 2, q = x + 2 ties on it (s + q even)
    for s_, q, own_x in ((x - 2, x + 2, True), (x + 2, x - 2, False), (x - 2, x + 3, True), (x - 3, x + 2, False)):
        sp, lo, hi = fscl_amd.cond_clip(scan, [(c, q, 1e-3)], c, s_)
        assert sp == s_
        assert (lo <= cs[c] + i <= hi) == own_x, (s_, q, lo, hi)
        assert (lo, hi) == cr.clip(pos, cs[c], cn[c], [q], s_)
    sp, lo, hi = fscl_amd.cond_clip(scan, [(c, x - 2, 1e-3)], c, x - 2)  # q = s
    assert lo > hi
    # a candidate whose nearest SNP lies beyond q: s just right of q, both between site i and site i + 1
    sp, lo, hi = fscl_amd.cond_clip(scan, [(c, x + 1, 1e-3)], c, x + 2)
    assert cr.init_point(pos, cs[c], cn[c], x + 2, 50)[0] == cs[c] + i and lo == cs[c] + i + 1 and hi == cs[c] + cn[c] - 1
    assert fscl_amd.cond_clip(scan, [], c, x + 2) == (x + 2, cs[c], cs[c] + cn[c] - 1)  # no given sweep on either side
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            fscl_amd.cond_clip(scan, [], bad, x)


def test_base_fold(built):
    g = np.array([0.1, 0.0, -0.0, 0.2, 0.3, NAN, 1e300, -1e300, 0.7])
    cases = [(10, 13, 10, 18), (10, 18, 11, 14), (16, 18, 10, 18), (10, 18, 10, 18), (11, 12, 10, 18), (14, 13, 10, 18),
             (-5, 100, 12, 16), (16, 17, 10, 18)]
    for lo, hi, ws, we in cases:
        got, n = fscl_amd.cond_base(g, 10, lo, hi, ws, we)
        want, wn = cr.base(g, 10, lo, hi, ws, we)
        assert wr.same(got, want) and n == wn, (lo, hi, ws, we, got, want)
    assert wr.same(fscl_amd.cond_base(g, 10, 10, 14, 10, 18)[0], ((0.1 + 0.2) + 0.3))
    assert math.isnan(fscl_amd.cond_base(g, 10, 10, 18, 10, 18)[0])      # the NaN reaches every fold over it
    assert fscl_amd.cond_base(g, 10, 16, 18, 10, 18)[0] == (1e300 + -1e300) + 0.7  # not a difference of prefix sums
    assert wr.bits(fscl_amd.cond_base(g, 10, 11, 12, 10, 18)[0]) == wr.bits(0.0)   # +0.0, never -0.0
    assert wr.bits(cr.cond_clr(-10.0, -12.5, 0.75)) == wr.bits(2.0 * ((-10.0 - -12.5) - 0.75))


def test_cond_ref_clipped_value(built):
    """The restatement itself: with the clip covering the window the clipped value is the plain walk's sum; an empty
    clip gives the null sum; the parts' sites are taken from the part lengths."""
    c = wr.cases()["edge-nonneg"]
    g, _ = wr.geometry()
    q = g[5]
    pt = wr.Point(q.near, q.sweep, q.ws, q.we, -700.5)
    for la in (-20.0, -6.0, -3.0, 4.0):
        t, lens = wr.walk_terms(c.tables, pt, la)
        full = wr.seq_sum(pt.null_logl, t)[0]
        v, n = cr.clipped_value(c.tables, pt, la, q.ws, q.we)
        assert wr.same(v, full) and n == len(t)
        assert cr.clipped_value(c.tables, pt, la, q.near + 1, q.near) == (pt.null_logl, 0)
        idx = cr.walk_sites(pt, lens)
        assert len(idx) == len(t) and (len(t) == 0 or (idx[0] == q.near and len(set(idx)) == len(idx)))
        if lens[0] > 0:
            v, n = cr.clipped_value(c.tables, pt, la, q.near - 1, q.near - 1)
            assert n == 1 and wr.same(v, pt.null_logl + t[1])
    assert cr.row_maximum([NAN, -5.0, -5.0, -7.0], [1.0, 2.0, 3.0, 4.0]) == (2.0, -5.0)
    assert cr.row_maximum([NAN], [1.0]) == (wr.LOG_AD_MAX, -wr.DBL_MAX)


def blocks_for_output():
    rows = np.zeros(3, dtype=fscl_amd.COND_ROW_DTYPE)
    rows[0] = (25_000, 3, 7, 5, math.log(1e-4), -1.25, 2.5, -10.0, -12.0)
    rows[1] = (26_000, 8, 9, 2, math.log(1e-2), 12.5, -0.75, -9.0, -12.0)
    rows[2] = (27_000, 9, 8, 0, 4.0, NAN, 0.0, NAN, -12.0)
    h0 = np.zeros(1, dtype=fscl_amd.COND_BLOCK_DTYPE)[0]
    h0["chr"], h0["round"], h0["max_row"], h0["added"] = 0, 1, 1, 1
    h1 = h0.copy()
    h1["chr"], h1["round"], h1["max_row"], h1["added"] = 2, 2, -1, 0
    gv = np.array([(0, 20_000, 1e-3), (0, 30_000, 2e-5)], dtype=fscl_amd.SWEEP_DTYPE)
    return [fscl_amd.CondBlock(h0, rows[:2], gv), fscl_amd.CondBlock(h1, rows[2:], gv[:1])]


def test_output_format(scan, tmp_path):
    s = scan.contents
    name = [s.chr_limits[c].name.decode() for c in range(3)]
    p = [s.snps[i].pos for i in range(10)]
    fscl_amd.conditional_output(tmp_path / "c.txt", scan, blocks_for_output(), "lab")
    lines = (tmp_path / "c.txt").read_text().splitlines()
    assert lines == [
        f"lab\t{name[0]}\t1\t25000\t1.000e-04\t-1.25\t{p[3]}\t{p[7]}\t5\t2.5000",
        f"lab\t{name[0]}\t1\t26000\t1.000e-02\t12.50\t{p[8]}\t{p[9]}\t2\t-0.7500",
        f"lab\t{name[0]}\t1\tsummary\t2\t2\t20000:1.000e-03,30000:2.000e-05\t26000\t1.000e-02\t12.50\t1",
        lines[3],
        f"lab\t{name[2]}\t2\tsummary\t1\t1\t20000:1.000e-03\tNA\tNA\tNA\t0"]
    f = lines[3].split("\t")
    assert f[:5] == ["lab", name[2], "2", "27000", "5.460e+01"] and f[5] in ("nan", "-nan") and f[6:] == ["NA", "NA", "0", "0.0000"]
    fscl_amd.conditional_output(tmp_path / "d.txt", scan, blocks_for_output())
    assert [ln.split("\t", 1)[1] for ln in lines] == (tmp_path / "d.txt").read_text().splitlines()
    fscl_amd.conditional_output(tmp_path / "e.txt", scan, [])
    assert (tmp_path / "e.txt").read_text() == ""
    bad = blocks_for_output()
    bad[0].hdr["chr"] = 3
    with pytest.raises(ValueError):
        fscl_amd.conditional_output(tmp_path / "f.txt", scan, bad)
    with pytest.raises(ValueError):
        fscl_amd.conditional_output(tmp_path / "no-such-dir" / "f.txt", scan, blocks_for_output())


def test_refusals_before_any_device_call(scan, monkeypatch):
    """FSCLG_E_ARG with no tables set (the pointer is never dereferenced): every refusal names its option."""
    L = fscl_amd.get_lib()
    tab = C.cast(C.c_void_p(1), C.POINTER(fscl_amd.SmPtableT))
    la = fscl_amd.surface_alphas()

    def refused(given, what, halfwidth=0, step=1000, alphas=la, rounds=1, min_clr=0.0):
        with pytest.raises(ValueError, match=what):
            fscl_amd.scan_conditional(scan, tab, given, halfwidth, step, alphas, rounds, min_clr)

    ok = [(0, 20_000, 1e-3)]
    refused([(3, 100, 1e-3)], "--given-sweep: unknown chromosome")
    refused([(-1, 100, 1e-3)], "--given-sweep: unknown chromosome")
    for a in (0.0, -1.0, NAN, math.inf, math.exp(-20.5), math.exp(4.5)):
        refused([(0, 100, a)], "--given-sweep: alpha")
    refused([(1, 100 + i, 1e-3) for i in range(65)], "--given-sweep: more than 64")
    refused(ok, "--conditional-step", step=0)
    refused(ok, "--conditional-halfwidth", halfwidth=-1)
    for r in (0, 9):
        refused(ok, "--conditional-rounds", rounds=r)
    refused(ok, "--conditional-min-clr", min_clr=NAN)
    for bad in ([], [0.0, 0.0], [1.0, 0.0], [-20.5, 0.0], [0.0, NAN], list(np.linspace(-20, 4, 65))):
        refused(ok, "--conditional-alphas", alphas=bad)
    assert fscl_amd.conditional_cap() == 2 ** 30
    monkeypatch.setenv("FSCL_AMD_COND_CAP", "1000")
    assert fscl_amd.conditional_cap() == 1000
    refused(ok, "FSCL_AMD_COND_CAP")  # 40 positions x 56 bytes
    # the bound counts the grid positions an interval of 2 halfwidth bp can hold: 2 halfwidth / step + 1, here two rows
    monkeypatch.setenv("FSCL_AMD_COND_CAP", str(2 * fscl_amd.COND_ROW_DTYPE.itemsize - 1))
    refused(ok, "FSCL_AMD_COND_CAP", halfwidth=5, step=10)
    monkeypatch.setenv("FSCL_AMD_COND_CAP", str(2 * fscl_amd.COND_ROW_DTYPE.itemsize))
    L.fscl_amd_conditional_check.restype = C.c_int
    L.fscl_amd_conditional_check.argtypes = [C.POINTER(fscl_amd.ScanT), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_int, C.c_double]
    g1 = fscl_amd._sweeps(ok)
    assert L.fscl_amd_conditional_check(scan, g1.ctypes.data, 1, 5, 10, la.ctypes.data, len(la), 1, 0.0) == 0
    monkeypatch.delenv("FSCL_AMD_COND_CAP")


def test_host_check_under_sanitizers(built, tmp_path):
    """tools/conditional_host_check.c: the clip, the given terms, the base fold and the writer under ASan and UBSan, as
    a stand-alone program (no device library, nothing loaded into Python)."""
    run_host_check("conditional_host_check", ["conditional.c", "util.c"], tmp_path, [tmp_path])


@pytest.mark.parametrize("args, msg", [
    (["--no-scan"], "--conditional-file with --no-scan needs explicit --given-sweep"),
    (["--conditional-step=0"], "--conditional-step must be at least 1"),
    (["--conditional-halfwidth=-5"], "--conditional-halfwidth must be >= 0"),
    (["--conditional-rounds=0"], "--conditional-rounds must be 1 .. 8"),
    (["--conditional-rounds=9"], "--conditional-rounds must be 1 .. 8"),
    (["--conditional-alphas=-20:4:64"], "--conditional-alphas must be LO:HI:N"),
    (["--conditional-step=-1"], "--conditional-step must be at least 1"),
    (["--conditional-step=7x"], "--conditional-step must be at least 1"),
    (["--conditional-min-clr=nan"], "--conditional-min-clr must be a number"),
    (["--given-sweep=chr1:1000:0"], "expected chr:pos:alpha, alpha positive with its natural log"),
    (["--given-sweep=chr1:1000:1e9"], "expected chr:pos:alpha, alpha positive with its natural log"),
    (["--given-sweep=chr1"], "expected chr:pos:alpha, alpha positive with its natural log"),
    # refused once the data is loaded, before the tables, the scan and any device work
    (["--given-sweep=no-such-chromosome:1000:1e-3"], "--given-sweep=no-such-chromosome:1000:1e-3: unknown chromosome name"),
    ([f"--given-sweep=@CHR@:{1000 + i}:1e-3" for i in range(65)], "more than 64 given sweeps on one chromosome"),
])
def test_cli_refusals(built, tmp_path, args, msg):
    """Refused before the data is loaded: no device is touched and no file is written."""
    first = (GOLD / "g1.snp").read_text().split(None, 1)[0]  # (the first chromosome's name)
    args = [a.replace("@CHR@", first) for a in args]
    r = run_cli([f"--conditional-file={tmp_path / 'c.txt'}"] + args, tmp_path, snp="g1.snp")
    assert r.returncode != 0 and msg in r.stderr + r.stdout, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "c.txt").exists() and not (tmp_path / "o.txt").exists()


def test_cli_cap_refused_before_the_scan(built, tmp_path, monkeypatch):
    monkeypatch.setenv("FSCL_AMD_COND_CAP", "100")
    first = (GOLD / "g1.snp").read_text().split(None, 1)[0]
    r = run_cli([f"--conditional-file={tmp_path / 'c.txt'}", f"--given-sweep={first}:1000:1e-3"], tmp_path, snp="g1.snp")
    assert r.returncode != 0 and "FSCL_AMD_COND_CAP" in r.stderr + r.stdout, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "c.txt").exists() and not (tmp_path / "o.txt").exists()


@pytest.mark.parametrize("opt", ["--given-sweep=chr1:1000:1e-3", "--conditional-step=500", "--conditional-halfwidth=0",
                                 "--conditional-rounds=1", "--conditional-min-clr=0", "--conditional-alphas=-20:4:7"])
def test_cli_options_need_the_file(built, tmp_path, opt):
    r = run_cli([opt], tmp_path, snp="g1.snp")
    assert r.returncode != 0 and "need --conditional-file" in r.stderr + r.stdout, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "o.txt").exists()


def test_run_keyword_refusals(built):
    for kw in (dict(conditional_step=0), dict(conditional_halfwidth=-1), dict(conditional_rounds=0), dict(conditional_rounds=9),
               dict(conditional_alphas=(-20.0, 4.0, 64))):
        with pytest.raises(ValueError):
            fscl_amd.run(GOLD / "g1.snp", conditional_file="unused.txt", **kw)
