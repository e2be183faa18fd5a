"""The fine-grid CLR profile (-g) on the GPU against the oracle, bit for bit.

Every profile point is init_scan_result(chr, pos) followed by search_maxalpha on the data as
loaded; the oracle exposes both (orc_init_scan_result, orc_search_maxalpha), so each field of
each point is compared by bit pattern.
"""
from __future__ import annotations

import ctypes as C
import math
import subprocess
import sys

import numpy as np
import pytest

from util import CLI, ROOT, read_dump, run_oracle, same_bits
import fscl_amd
import walk_ref as wr
from fscl_amd import synth

sys.path.insert(0, str(ROOT / "oracle"))
import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("chr", "nearest_snp", "sweep_pos", "n_snps", "window_start", "window_end", "null_logl", "lalpha", "sm_logl",
          "clr")


class OrcChr(C.Structure):  # orc_chr_t
    _fields_ = [("chr", C.c_int), ("name", C.c_char_p), ("start_index", C.c_int), ("n_snps", C.c_int),
                ("start_pos", C.c_int), ("bp_length", C.c_int)]


class Oracle:
    """An SNP file in the oracle (input, background, tables, null model) and its per-point loop."""

    def __init__(self, snp, eval_range=81920):
        self.o = orc.OracleScan(snp)
        L = self.o.L
        L.orc_init_scan_result.argtypes = [C.POINTER(orc.OrcPt), C.c_int, C.c_void_p, C.POINTER(OrcChr), C.c_int, C.c_int,
                                           C.POINTER(orc.OrcStats)]
        L.orc_init_scan_result.restype = None
        L.orc_search_maxalpha.argtypes = [C.POINTER(orc.OrcPt), C.c_void_p, C.c_void_p, C.POINTER(orc.OrcStats)]
        L.orc_search_maxalpha.restype = None
        self.er = eval_range

    def points(self, chr_pos) -> list[tuple]:
        L, s, st = self.o.L, self.o.s.contents, self.o.stats
        lim = C.cast(s.chr, C.POINTER(OrcChr))  # orc_init_scan_result takes the chromosome's own limits
        out = []
        for ch, pos in chr_pos:
            pt = orc.OrcPt()
            L.orc_init_scan_result(C.byref(pt), int(ch), s.snps, C.byref(lim[int(ch)]), self.er, int(pos), C.byref(st))
            L.orc_search_maxalpha(C.byref(pt), s.snps, self.o.tab, C.byref(st))
            out.append(tuple(getattr(pt, k) for k in FIELDS))
        return out


def rows_of(arr) -> list[tuple]:
    return [tuple(p[k].item() for k in FIELDS) for p in arr]


def assert_points_equal(got, want, what=""):
    assert len(got) == len(want), f"{what}: {len(got)} points vs {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(g, w)):
            ok = same_bits(x, y) if isinstance(x, float) else x == y
            assert ok, f"{what}: point {i} field {FIELDS[k]}: {x!r} != {y!r} (row {g} vs {w})"


def py_grid(scan, g, G):
    """Restatement of the grid: per chromosome from the first cell's start in steps of g to the
    last cell's clipped end, the end appended when the step misses it; (chr, pos, cell)."""
    s = scan.contents
    out, cell0 = [], 0
    for c in range(s.n_chromosomes):
        start, end = s.chr_limits[c].start_pos, s.chr_limits[c].bp_length
        if start >= end:
            continue
        n_cells = -(-(end - start) // G)
        pos = list(range(start, end + 1, g))
        if pos[-1] != end:
            pos.append(end)
        for p in pos:
            k = 0 if p == start else min((p - start - 1) // G, n_cells - 1)
            out.append((c, p, cell0 + k))
        cell0 += n_cells
    return out


def setup(snp):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    scan = fscl_amd.load_snp_input(snp)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp)
    fscl_amd.compute_snp_null_model(scan, fsp)
    return scan, tab


def check_profile(snp, g, G, er=81920, what="", limit=5000):
    scan, tab = setup(snp)
    grid = py_grid(scan, g, G)
    assert len(grid) <= limit
    prof = fscl_amd.scan_profile(scan, tab, er, g, G)
    assert [(int(p["chr"]), int(p["grid_pos"]), int(p["cell"])) for p in prof] == grid
    assert_points_equal(rows_of(prof), Oracle(snp, er).points([(c, p) for c, p, _ in grid]), what)
    return scan, tab, prof


def test_tiny_chromosomes_whole_chromosome_windows(built, tmp):
    """1, 2, 3, 64, 65 and 130 SNPs and one larger chromosome, folded sites, two depths."""
    chrs = []
    for i, (k, length) in enumerate(((1, 50_000), (2, 90_000), (3, 150_000), (64, 700_000), (65, 900_000),
                                     (130, 1_300_000), (3000, 3_000_000))):
        chrs += synth.generate(n_chr=1, chr_len=length, snps_per_chr=k, n=16, seed=170 + i, chr_names=[f"t{i}"],
                               sweeps_per_chr=1 if k >= 64 else 0, folded=0.3 if k >= 64 else 0.0,
                               missing=0.2 if k >= 64 else 0.0, max_missing=2)
    snp = tmp / "tiny.snp"
    synth.write_snp_file(str(snp), chrs)
    # (the chromosomes and -g 1000 -G 20000 as specified: 6.19 Mb in all, 6 197 points, most of them on
    # chromosomes of a few SNPs whose points cost the oracle nothing: 0.65 s for the whole case)
    check_profile(snp, 1000, 20000, what="tiny", limit=6200)


def test_a_batch_holds_one_kind_of_call(built, tmp):
    """On a context of its own with the tiny chromosomes' tables, one run of two positions: a batch that
    holds a profile is rejected by the search's and the cell maxima's wait (FSCLG_E_STATE) and stays
    submitted; its own wait then returns the points of a plain fsclg_profile call, and a search on
    batch 0 runs after it.  Then the accounting of three calls of different kinds: one launch each, and
    their kernel times added to kernel_ms in call order."""
    chrs = []
    for i, (k, length) in enumerate(((1, 50_000), (2, 90_000), (3, 150_000), (64, 700_000), (65, 900_000),
                                     (130, 1_300_000))):
        chrs += synth.generate(n_chr=1, chr_len=length, snps_per_chr=k, n=16, seed=170 + i, chr_names=[f"t{i}"],
                               sweeps_per_chr=1 if k >= 64 else 0, folded=0.3 if k >= 64 else 0.0,
                               missing=0.2 if k >= 64 else 0.0, max_missing=2)
    snp = tmp / "tiny6.snp"
    synth.write_snp_file(str(snp), chrs)
    ot = wr.OracleTables(snp)
    s = ot.o.s.contents
    lim = C.cast(s.chr, C.POINTER(OrcChr))
    chr_start, chr_n = [lim[c].start_index for c in range(6)], [lim[c].n_snps for c in range(6)]
    assert chr_n == [1, 2, 3, 64, 65, 130]
    E_STATE, er, vp = -3, 81920, C.c_void_p
    RunT, PointT = fscl_amd.RunT, fscl_amd.PointT
    shim = wr.Shim()
    try:
        L, ctx = shim.L, shim.ctx
        for name, res, args in (("fsclg_profile_submit", C.c_int, [vp, C.POINTER(RunT), C.c_int, C.c_int]),
                                ("fsclg_profile_wait", C.c_int, [vp, C.POINTER(PointT)]),
                                ("fsclg_search_wait", C.c_int, [vp, C.c_int, C.POINTER(PointT)]),
                                ("fsclg_search_maxpos", C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PointT)]),
                                ("fsclg_cellmax_submit", C.c_int, [vp, C.c_int, C.c_int, C.POINTER(RunT), C.c_int, C.c_int]),
                                ("fsclg_cellmax_wait", C.c_int, [vp, C.c_int, C.POINTER(PointT)]),
                                ("fsclg_curve_submit", C.c_int, [vp, C.c_int, C.c_int, C.POINTER(RunT), C.c_int, C.c_int]),
                                ("fsclg_curve_wait", C.c_int, [vp, C.c_int, vp]),
                                ("fsclg_profile_last_ms", C.c_double, [vp]),
                                ("fsclg_cellmax_last_ms", C.c_double, [vp, C.c_int]),
                                ("fsclg_curve_last_ms", C.c_double, [vp, C.c_int])):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
        shim.upload(ot.tables, chr_start, chr_n)
        shim.set_chr_null(-123.25, 6)
        runs = (RunT * 1)(RunT(5, 400_000, 1000, 2))
        want, got, other = (PointT * 2)(), (PointT * 2)(), (PointT * 2)()
        shim._ok(L.fsclg_profile(ctx, runs, 1, er, want), "fsclg_profile")
        assert [q.sweep_pos > 0 and q.flags == 0 and math.isfinite(q.clr) for q in want] == [True, True]

        shim._ok(L.fsclg_profile_submit(ctx, runs, 1, er), "fsclg_profile_submit")
        assert L.fsclg_search_wait(ctx, 0, other) == E_STATE
        assert L.fsclg_cellmax_wait(ctx, 0, other) == E_STATE
        assert bytes(other) == bytes(2 * C.sizeof(PointT)), "a rejected wait wrote points"
        shim._ok(L.fsclg_profile_wait(ctx, got), "fsclg_profile_wait")
        assert bytes(got) == bytes(want)
        cell = np.array([5, 380_000, 420_000, 0], dtype=np.int32)  # fsclg_cell_t
        shim._ok(L.fsclg_search_maxpos(ctx, cell.ctypes.data, 1, er, 100, other), "fsclg_search_maxpos")
        assert other[0].flags == 0 and other[0].chr == 5

        st0, st1 = wr.StatsT(), wr.StatsT()
        shim._ok(L.fsclg_get_stats(ctx, C.byref(st0)), "fsclg_get_stats")
        shim._ok(L.fsclg_profile(ctx, runs, 1, er, got), "fsclg_profile")
        shim._ok(L.fsclg_cellmax_submit(ctx, 1, 0, runs, 1, er), "fsclg_cellmax_submit")
        shim._ok(L.fsclg_cellmax_wait(ctx, 1, other), "fsclg_cellmax_wait")
        curves = np.zeros(2, dtype=fscl_amd.CURVE_DTYPE)
        shim._ok(L.fsclg_curve_submit(ctx, 2, 0, runs, 1, er), "fsclg_curve_submit")
        shim._ok(L.fsclg_curve_wait(ctx, 2, curves.ctypes.data), "fsclg_curve_wait")
        shim._ok(L.fsclg_get_stats(ctx, C.byref(st1)), "fsclg_get_stats")
        ms = [L.fsclg_profile_last_ms(ctx), L.fsclg_cellmax_last_ms(ctx, 1), L.fsclg_curve_last_ms(ctx, 2)]
        print(f"launches {st0.n_launches} -> {st1.n_launches}, kernel_ms {st0.kernel_ms!r} -> {st1.kernel_ms!r}, "
              f"last_ms {ms!r}")
        assert all(m > 0.0 for m in ms)
        assert st1.n_launches - st0.n_launches == 3
        acc = st0.kernel_ms
        for m in ms:
            acc += m
        assert abs(st1.kernel_ms - acc) <= 1e-9
        assert bytes(got) == bytes(want)
    finally:
        shim.close()


def test_positions_on_snps(built, tmp):
    """Runs of step 1 over exact SNP positions, over SNPs at consecutive base pairs (the
    de-collision moves a point more than once), before the first SNP and after the last.
    With one device fscl_amd_profile_runs hands the runs to fsclg_profile as they are."""
    (nm, pos, k, nn, fold), = synth.generate(n_chr=1, chr_len=400_000, snps_per_chr=1500, n=16, seed=181)
    pos = np.array(sorted(set(int(p) for p in pos)))
    i0 = len(pos) // 2
    pos = np.concatenate([pos[:i0], [pos[i0 - 1] + 1, pos[i0 - 1] + 2, pos[i0 - 1] + 3], pos[i0:]])
    pos = np.array(sorted(set(int(p) for p in pos)))
    m = len(pos)
    chrs = [(nm, pos, np.resize(k, m), np.resize(nn, m), np.resize(fold, m))]
    snp = tmp / "onsnp.snp"
    synth.write_snp_file(str(snp), chrs)
    scan, tab = setup(snp)
    s = scan.contents
    p = [s.snps[i].pos for i in range(s.n_snps)]
    j = next(i for i in range(s.n_snps - 2) if p[i + 1] == p[i] + 1 and p[i + 2] == p[i] + 2)
    runs = [(0, p[j] - 2, 1, 8), (0, p[10], 1, 1), (0, max(p[0] - 5, 0), 1, 7), (0, p[-1] - 1, 1, 5), (0, p[200], 1, 3)]
    got = fscl_amd.profile_runs(scan, tab, runs)
    want = Oracle(snp).points([(c, a + t * st) for c, a, st, n in runs for t in range(n)])
    assert any(w[2] - (runs[0][1] + t) >= 2 for t, w in enumerate(want[:8])), "no point moved more than once"
    assert_points_equal(rows_of(got), want, "on snps")


@pytest.fixture(scope="module")
def edge_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("edges")
    snp = d / "edges.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=1, chr_len=2_000_000, snps_per_chr=2000, n=16, seed=182,
                                                   sweeps_per_chr=1))
    return dict(snp=snp, want={})


@pytest.mark.parametrize("chunk", [None, 1, 3])
def test_chunk_edges(built, edge_case, monkeypatch, chunk):
    """Runs of 1, 2, 3, CHUNK-1, CHUNK, CHUNK+1 and 2*CHUNK+1 positions in one call, at the
    default chunk length and at 1 and 3 (odd tails, one-position chunks).  The runs reach
    fsclg_profile whole (one device), so its own cutting into chunks and their output offsets
    are what is checked."""
    if chunk is None:
        monkeypatch.delenv("FSCLG_PROFILE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("FSCLG_PROFILE_CHUNK", str(chunk))
    ch = fscl_amd.profile_chunk()
    assert ch == (chunk or ch) and ch >= 1
    dflt = edge_case.setdefault("default_chunk", ch) if chunk is None else edge_case.get("default_chunk", 16)
    runs, a = [], 20_000
    for n in (1, 2, 3, dflt - 1, dflt, dflt + 1, 2 * dflt + 1):
        runs.append((0, a, 1500, n))
        a += 1500 * n + 777
    assert a < 2_000_000
    scan, tab = setup(edge_case["snp"])
    got = fscl_amd.profile_runs(scan, tab, runs)
    if "pts" not in edge_case["want"]:
        edge_case["want"]["pts"] = Oracle(edge_case["snp"]).points(
            [(c, s + t * st) for c, s, st, n in runs for t in range(n)])
    assert_points_equal(rows_of(got), edge_case["want"]["pts"], f"chunk {ch}")


@pytest.mark.parametrize("name,er,g,G,parts", [
    ("long", 300, 2000, 40000, [dict(n_chr=2, chr_len=4_000_000, snps_per_chr=4000, n=30, seed=51, sweeps_per_chr=1)]),
    ("mixed", 700, 4000, 40000, [dict(n_chr=1, chr_len=900_000, snps_per_chr=900, n=24, seed=52, chr_names=["a"]),
                                 dict(n_chr=1, chr_len=1_500_000, snps_per_chr=1401, n=24, seed=53, chr_names=["b"]),
                                 dict(n_chr=1, chr_len=9_000_000, snps_per_chr=7000, n=24, seed=54, chr_names=["c"],
                                      sweeps_per_chr=2, missing=0.2, max_missing=2)]),
])
def test_windowed_null_sums(built, tmp, name, er, g, G, parts):
    """Chromosomes shorter than, equal to and longer than the window 2*er+1: each point's
    null_logl is its own window's sequential sum, from the window kernels."""
    chrs = []
    for p in parts:
        chrs += synth.generate(**p)
    snp = tmp / f"{name}.snp"
    synth.write_snp_file(str(snp), chrs)
    fscl_amd.reset_stats()
    check_profile(snp, g, G, er, name)
    assert fscl_amd.get_stats()["window_ms"] > 0


@pytest.fixture(scope="module")
def sweep_case(tmp_path_factory):
    """A genome with planted sweeps, its oracle scan dump and its oracle profile (computed once)."""
    d = tmp_path_factory.mktemp("sweeps")
    snp = d / "sweeps.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=2, chr_len=2_000_000, snps_per_chr=2500, n=20, seed=183,
                                                   sweeps_per_chr=2))
    return dict(dir=d, snp=snp, g=1000, G=50000)


def oracle_profile(case):
    if "want" not in case:
        scan, _ = setup(case["snp"])
        case["grid"] = py_grid(scan, case["g"], case["G"])
        case["want"] = Oracle(case["snp"]).points([(c, p) for c, p, _ in case["grid"]])
    return case["grid"], case["want"]


def test_profile_is_of_the_unpermuted_rows(built, sweep_case):
    """Profile, scan_permute with 4 trials, profile again: identical bits; the scan and the
    permutation results equal a run without any profile call."""
    snp, g, G = sweep_case["snp"], sweep_case["g"], sweep_case["G"]
    grid, want = oracle_profile(sweep_case)
    ref = fscl_amd.points(fscl_amd.run(snp, None, n_permute=4, large_grid_sp=G))
    scan, tab = setup(snp)
    fscl_amd.srand()
    fscl_amd.set_permute_mode("parity")
    fscl_amd.scan_chromosome(scan, tab, large_grid_sp=G)
    p1 = fscl_amd.scan_profile(scan, tab, small_grid_sp=g, large_grid_sp=G)
    fscl_amd.scan_permute(scan, tab, 4, large_grid_sp=G)
    p2 = fscl_amd.scan_profile(scan, tab, small_grid_sp=g, large_grid_sp=G)
    assert p1.tobytes() == p2.tobytes()
    assert_points_equal(rows_of(p2), want, "after scan_permute")
    assert fscl_amd.points(scan).tobytes() == ref.tobytes()


def test_two_devices_in_one_process(built, sweep_case):
    snp, g, G = sweep_case["snp"], sweep_case["g"], sweep_case["G"]
    grid, want = oracle_profile(sweep_case)
    fscl_amd.set_devices([0, 0])
    try:
        scan, tab = setup(snp)
        prof = fscl_amd.scan_profile(scan, tab, small_grid_sp=g, large_grid_sp=G)
        assert fscl_amd.get_lib().fscl_amd_n_devices() == 2
    finally:
        fscl_amd.set_device(0)
    assert_points_equal(rows_of(prof), want, "two devices")
    one = fscl_amd.scan_profile(scan, tab, small_grid_sp=g, large_grid_sp=G)
    assert one.tobytes() == prof.tobytes()


def test_cell_maxima(built, sweep_case):
    """profile_cell_max against a NumPy restatement over the oracle's profile (first point of
    strictly greatest CLR), n_missed against the oracle's scan dump."""
    snp, g, G, d = sweep_case["snp"], sweep_case["g"], sweep_case["G"], sweep_case["dir"]
    grid, want = oracle_profile(sweep_case)
    run_oracle(snp, d / "o.txt", [f"--coarse-grid-spacing={G}"], d / "o.dump")
    dump = read_dump(d / "o.dump")
    scan, tab = setup(snp)
    fscl_amd.scan_chromosome(scan, tab, large_grid_sp=G)
    prof = fscl_amd.scan_profile(scan, tab, small_grid_sp=g, large_grid_sp=G)
    got, n_missed = fscl_amd.profile_cell_max(prof, scan)
    s = scan.contents
    clr = np.array([w[FIELDS.index("clr")] for w in want])
    gch = np.array([c for c, _, _ in grid])
    gpos = np.array([p for _, p, _ in grid])
    cells = []
    for c in range(s.n_chromosomes):
        a, e = s.chr_limits[c].start_pos, s.chr_limits[c].bp_length
        while a < e:
            cells.append((c, a, min(a + G, e)))
            a += G
    assert len(cells) == len(dump) == len(got)
    missed = 0
    for k, (c, a, e) in enumerate(cells):
        idx = np.flatnonzero((gch == c) & (gpos >= a) & (gpos <= e))
        best = idx[int(np.argmax(clr[idx]))]  # argmax: the first of the greatest
        assert_points_equal([tuple(got[k][f].item() for f in FIELDS)], [want[best]], f"cell {k}")
        missed += clr[best] > dump[k][2]
        assert clr[best] >= max(clr[idx[0]], clr[idx[-1]])  # (a check on this test)
    assert n_missed == missed


@pytest.mark.parametrize("nperm", [0, 3])
def test_cli_profile_file(built, sweep_case, tmp, nperm):
    snp, g, G = sweep_case["snp"], sweep_case["g"], sweep_case["G"]
    grid, want = oracle_profile(sweep_case)
    base = [str(CLI), "-f", str(snp), "-G", str(G), "-g", str(g)] + ([f"--n-permute={nperm}"] if nperm else [])
    r0 = subprocess.run(base + ["-o", str(tmp / "a.txt")], capture_output=True, text=True, timeout=600)
    r1 = subprocess.run(base + ["-o", str(tmp / "b.txt"), f"--profile-file={tmp / 'p.txt'}"], capture_output=True,
                        text=True, timeout=600)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert (tmp / "a.txt").read_bytes() == (tmp / "b.txt").read_bytes()
    assert "Profile:" in r1.stderr + r1.stdout
    scan, _ = setup(snp)
    s = scan.contents
    f = {k: i for i, k in enumerate(FIELDS)}
    text = "".join("%s\t%d\t%1.2f\t%1.3e\t%d\t%d\t%d\n" % (
        s.chr_limits[w[f["chr"]]].name.decode(), w[f["sweep_pos"]], w[f["clr"]], math.exp(w[f["lalpha"]]),
        w[f["n_snps"]], s.snps[w[f["window_start"]]].pos, s.snps[w[f["window_end"]]].pos) for w in want)
    assert (tmp / "p.txt").read_text() == text
