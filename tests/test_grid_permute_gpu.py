"""The grid-maximum scan and permutation test (--scan-mode=grid) against the oracle, bit for bit.

A cell's statistic is the first position of strictly greatest CLR among its -g spaced positions
(scan-chromosome.c:269-296, `>` at :287); a trial takes the same maximum on the permuted SNPs
(the reference's disabled fine-grid trial, :505-523, inside its trial loop :441-502).  The oracle
side is composed here from what liboracle exports: orc_init_scan_result + orc_search_maxalpha per
position, orc_block_permute and orc_rand for the trial loop.
"""
from __future__ import annotations

import ctypes as C
import math
import subprocess
import sys

import numpy as np
import pytest

from util import CLI, ROOT, same_bits
import fscl_amd
from fscl_amd import synth

sys.path.insert(0, str(ROOT / "oracle"))
import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("chr", "nearest_snp", "sweep_pos", "n_snps", "window_start", "window_end", "null_logl", "lalpha", "sm_logl",
          "clr")
CLR = FIELDS.index("clr")
SEED = 0xFD821A6
SAVE = 10000  # CLR_NULL_DIST_SAVE
ORC_SNP = np.dtype([("chr", "<i4"), ("pos", "<i4"), ("null_logl", "<f8"), ("obs_freq", "<i4"), ("depth_p", "<i4"),
                    ("folded", "<i4"), ("pad", "<i4")])


class OrcChr(C.Structure):  # orc_chr_t
    _fields_ = [("chr", C.c_int), ("name", C.c_char_p), ("start_index", C.c_int), ("n_snps", C.c_int),
                ("start_pos", C.c_int), ("bp_length", C.c_int)]


class OrcRand(C.Structure):  # orc_rand_t
    _fields_ = [("r", C.c_int32 * 31), ("f", C.c_int), ("b", C.c_int)]


class Oracle:
    """An SNP file in the oracle and its per-point loop, on its own SNPs or on a permuted copy."""

    def __init__(self, snp, eval_range=81920):
        self.o = orc.OracleScan(snp)
        L = self.o.L
        L.orc_init_scan_result.argtypes = [C.POINTER(orc.OrcPt), C.c_int, C.c_void_p, C.POINTER(OrcChr), C.c_int, C.c_int,
                                           C.POINTER(orc.OrcStats)]
        L.orc_init_scan_result.restype = None
        L.orc_search_maxalpha.argtypes = [C.POINTER(orc.OrcPt), C.c_void_p, C.c_void_p, C.POINTER(orc.OrcStats)]
        L.orc_search_maxalpha.restype = None
        L.orc_block_permute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.POINTER(OrcRand),
                                        C.POINTER(orc.OrcStats)]
        L.orc_block_permute.restype = None
        L.orc_srand.argtypes = [C.POINTER(OrcRand), C.c_uint]
        L.orc_srand.restype = None
        L.orc_rand.argtypes = [C.POINTER(OrcRand)]
        L.orc_rand.restype = C.c_int
        self.er = eval_range
        self.n = self.o.s.contents.n_snps
        self.perm = np.zeros(max(self.n, 1), ORC_SNP)  # orc_block_permute's output

    def snps(self) -> np.ndarray:
        return np.frombuffer((C.c_char * (ORC_SNP.itemsize * self.n)).from_address(self.o.s.contents.snps), ORC_SNP)

    def permute(self, g, nbp=0.1, width=1.0):
        self.o.L.orc_block_permute(self.perm.ctypes.data, self.o.s.contents.snps, self.n, nbp, width, C.byref(g),
                                   C.byref(self.o.stats))

    def points(self, chr_pos, permuted=False) -> list[tuple]:
        L, s, st = self.o.L, self.o.s.contents, self.o.stats
        snps = self.perm.ctypes.data if permuted else s.snps
        lim = C.cast(s.chr, C.POINTER(OrcChr))
        out = []
        for ch, pos in chr_pos:
            pt = orc.OrcPt()
            L.orc_init_scan_result(C.byref(pt), int(ch), snps, C.byref(lim[int(ch)]), self.er, int(pos), C.byref(st))
            L.orc_search_maxalpha(C.byref(pt), snps, self.o.tab, C.byref(st))
            out.append(tuple(getattr(pt, k) for k in FIELDS))
        return out

    def run_max(self, run, permuted=False):
        """The first point of strictly greatest clr of one (chr, start, step, count) run; None if empty."""
        c, a, st, n = run
        return first_max(self.points([(c, a + t * st) for t in range(n)], permuted))


def first_max(pts):
    best = None
    for p in pts:
        if best is None or p[CLR] > best[CLR]:
            best = p
    return best


ZERO = tuple(0.0 if k in ("null_logl", "lalpha", "sm_logl", "clr") else 0 for k in FIELDS)


def rows_of(arr) -> list[tuple]:
    return [tuple(p[k].item() for k in FIELDS) for p in arr]


def assert_points_equal(got, want, what=""):
    assert len(got) == len(want), f"{what}: {len(got)} points vs {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(g, w)):
            ok = same_bits(x, y) if isinstance(x, float) else x == y
            assert ok, f"{what}: point {i} field {FIELDS[k]}: {x!r} != {y!r} (row {g} vs {w})"


def setup(snp):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    scan = fscl_amd.load_snp_input(snp)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp)
    fscl_amd.compute_snp_null_model(scan, fsp)
    return scan, tab


def scan_cells(scan, G):
    s = scan.contents
    cells = []
    for c in range(s.n_chromosomes):
        a, e = s.chr_limits[c].start_pos, s.chr_limits[c].bp_length
        while a < e:
            cells.append((c, a, min(a + G, e)))
            a += G
    return cells


def cell_positions(cell, g):
    """start + j*g with start <= pos <= end, the end appended when the step misses it."""
    c, a, e = cell
    pos = list(range(a, e + 1, g))
    if pos[-1] != e:
        pos.append(e)
    return [(c, p) for p in pos]


def set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("FSCLG_PROFILE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("FSCLG_PROFILE_CHUNK", str(chunk))
    return fscl_amd.profile_chunk()


# ------------------------------------------------------------------ 1. chunk edges
@pytest.fixture(scope="module")
def edge_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gedges")
    snp = d / "edges.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=1, chr_len=2_000_000, snps_per_chr=2000, n=16, seed=182,
                                                   sweeps_per_chr=1))
    return dict(snp=snp)


@pytest.mark.parametrize("chunk", [None, 1, 3])
def test_chunk_edges(built, edge_case, monkeypatch, chunk):
    """Runs of 1, 2, 3, CH-1, CH, CH+1 and 2*CH+1 positions (CH: the default chunk) and an empty
    run in one call, at the default chunk length and at 1 and 3: every run's point is the first
    strict maximum of the oracle's points of the run."""
    ch = set_chunk(monkeypatch, chunk)
    assert ch == (chunk or ch) and ch >= 1
    dflt = edge_case.setdefault("default_chunk", ch) if chunk is None else edge_case.get("default_chunk", 16)
    runs, a = [], 20_000
    for n in (1, 2, 3, dflt - 1, 0, dflt, dflt + 1, 2 * dflt + 1):
        runs.append((0, a, 1500, n))
        a += 1500 * n + 777
    assert a < 2_000_000
    scan, tab = setup(edge_case["snp"])
    got = fscl_amd.cellmax_runs(scan, tab, runs)
    if "want" not in edge_case:
        o = Oracle(edge_case["snp"])
        edge_case["want"] = [o.run_max(r) or ZERO for r in runs]
    assert_points_equal(rows_of(got), edge_case["want"], f"chunk {ch}")
    assert int(got[4]["n_snps"]) == 0


# ------------------------------------------------------------------ 2. ties
@pytest.fixture(scope="module")
def tie_case(tmp_path_factory):
    """A one-SNP chromosome (beside a larger one that gives the background spectrum)."""
    d = tmp_path_factory.mktemp("gties")
    chrs = synth.generate(n_chr=1, chr_len=50_000, snps_per_chr=1, n=16, seed=170, chr_names=["t0"])
    chrs += synth.generate(n_chr=1, chr_len=1_000_000, snps_per_chr=1500, n=16, seed=171, chr_names=["t1"],
                           sweeps_per_chr=1)
    snp = d / "ties.snp"
    synth.write_snp_file(str(snp), chrs)
    return dict(snp=snp)


@pytest.mark.parametrize("chunk", [None, 1, 3])
def test_ties_the_first_wins(built, tie_case, monkeypatch, chunk):
    """With one SNP at p, CLR depends only on |pos - p| (sm-search.c:114): the runs p-3s .. p+3s and
    p-5s .. p+5s in steps of 2s attain their maximum at p-s and at p+s, and p-s must be returned.
    Chunk length 1 puts the two in different chunks, 3 and the default in one pair or one chunk."""
    set_chunk(monkeypatch, chunk)
    scan, tab = setup(tie_case["snp"])
    s = scan.contents
    assert s.chr_limits[0].n_snps == 1
    p = s.snps[s.chr_limits[0].start_index].pos
    sp = min(1000, (p - 1) // 5)
    assert sp >= 2
    runs = [(0, p - 3 * sp, 2 * sp, 4), (0, p - 5 * sp, 2 * sp, 6)]
    if "want" not in tie_case:
        o = Oracle(tie_case["snp"])
        want = []
        for c, a, st, n in runs:
            pts = o.points([(c, a + t * st) for t in range(n)])
            clr = [q[CLR] for q in pts]
            hit = [t for t in range(n) if clr[t] == max(clr)]
            assert hit == [n // 2 - 1, n // 2], (hit, clr)  # (a check on this test: the maximum occurs twice)
            assert pts[hit[0]][FIELDS.index("sweep_pos")] == p - sp
            want.append(pts[hit[0]])
        tie_case["want"] = want
    got = fscl_amd.cellmax_runs(scan, tab, runs)
    assert_points_equal(rows_of(got), tie_case["want"], f"ties, chunk {chunk}")


# ------------------------------------------------------------------ 3. permuted rows, non-zero slot
def test_permuted_rows_in_another_slot(built, tmp):
    """eval_range 300 on chromosomes of 4 000 and 900 SNPs (longer than the window 601: window
    null sums of the slot's rows) and of 500 (shorter: the slot's whole-chromosome sums).  The rows
    are the product's own host block permutation of the sites' rows, which the oracle's
    orc_block_permute with the same stream reproduces (checked here on the null rows)."""
    er = 300
    chrs = synth.generate(n_chr=1, chr_len=4_000_000, snps_per_chr=4000, n=20, seed=61, chr_names=["a"], sweeps_per_chr=1)
    chrs += synth.generate(n_chr=1, chr_len=900_000, snps_per_chr=900, n=20, seed=62, chr_names=["b"])
    chrs += synth.generate(n_chr=1, chr_len=500_000, snps_per_chr=500, n=20, seed=63, chr_names=["c"])
    snp = tmp / "perm.snp"
    synth.write_snp_file(str(snp), chrs)
    scan, tab = setup(snp)
    s = scan.contents
    n = s.n_snps
    assert [s.chr_limits[c].n_snps > 2 * er + 1 for c in range(3)] == [True, True, False]
    lib = fscl_amd.get_lib()
    lib.fscl_amd_plan_permute_test.restype = C.c_int
    lib.fscl_amd_plan_permute_test.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                               C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    pos = np.array([s.snps[i].pos for i in range(n)], dtype=np.int32)
    cs = np.array([s.chr_limits[c].start_index for c in range(3)], dtype=np.int32)
    cn = np.array([s.chr_limits[c].n_snps for c in range(3)], dtype=np.int32)
    g_prod = (C.c_int32 * 33)()
    lib.fh_srand(g_prod, SEED)
    perm = np.arange(n, dtype=np.uint32)
    out = (C.c_longlong * 4)()
    assert lib.fscl_amd_plan_permute_test(n, pos.ctypes.data, cs.ctypes.data, cn.ctypes.data, 3, 0.1, 1.0, g_prod,
                                          perm.ctypes.data, out) == 0
    assert (perm != np.arange(n)).sum() > n // 2
    o = Oracle(snp, er)
    g_orc = OrcRand()
    o.o.L.orc_srand(C.byref(g_orc), SEED)
    o.permute(g_orc)
    assert np.array_equal(o.perm["null_logl"][:n].view("u8"), o.snps()["null_logl"][perm].view("u8"))
    rows = fscl_amd.site_rows(scan, tab)[perm]
    runs = [(0, 10_000, 35_000, 40), (0, 3_990_000, 1000, 11), (1, 0, 45_000, 21), (2, 5_000, 49_000, 11), (2, 500_000, 1, 1)]
    before = fscl_amd.scan_profile(scan, tab, er, 20_000, 400_000)
    got = fscl_amd.cellmax_runs(scan, tab, runs, er, rows=rows)
    assert_points_equal(rows_of(got), [o.run_max(r, permuted=True) for r in runs], "permuted rows")
    plain = fscl_amd.cellmax_runs(scan, tab, runs, er)
    assert_points_equal(rows_of(plain), [o.run_max(r) for r in runs], "uploaded rows")
    assert rows_of(plain) != rows_of(got)
    after = fscl_amd.scan_profile(scan, tab, er, 20_000, 400_000)
    assert before.tobytes() == after.tobytes()
    assert_points_equal(rows_of(after), o.points([(int(q["chr"]), int(q["grid_pos"])) for q in after]), "profile after")


# ------------------------------------------------------------------ 4. scan_chromosome_grid
def check_grid_scan(snp, g, G, what):
    scan, tab = setup(snp)
    fscl_amd.scan_chromosome_grid(scan, tab, small_grid_sp=g, large_grid_sp=G)
    got = fscl_amd.points(scan)
    prof = fscl_amd.scan_profile(scan, tab, small_grid_sp=g, large_grid_sp=G)
    mx, _ = fscl_amd.profile_cell_max(prof, scan)
    assert got.tobytes() == mx.tobytes(), f"{what}: not profile_cell_max(scan_profile)"
    cells = scan_cells(scan, G)
    assert len(got) == len(cells)
    assert not got["permute_n"].any() and not got["permute_p"].any() and not got["permute_finished"].any()
    o = Oracle(snp)
    memo = {}
    want = []
    for cell in cells:
        cp = cell_positions(cell, g)
        new = [q for q in cp if q not in memo]
        memo.update(zip(new, o.points(new)))
        want.append(first_max([memo[q] for q in cp]))
    assert_points_equal(rows_of(got), want, what)
    return cells


def test_scan_chromosome_grid_sweeps(built, tmp):
    snp = tmp / "sweeps.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=2, chr_len=2_000_000, snps_per_chr=2500, n=20, seed=183,
                                                   sweeps_per_chr=2))
    check_grid_scan(snp, 1000, 50000, "sweeps")


def test_scan_chromosome_grid_tiny_chromosomes(built, tmp):
    """1-, 2-, 3-SNP chromosomes, an appended end point (two runs for the last cell), a one-position tail."""
    chrs = []
    for i, (k, length) in enumerate(((1, 50_000), (2, 90_000), (3, 150_000), (64, 700_000), (65, 900_000),
                                     (130, 1_300_000), (3000, 3_000_000))):
        chrs += synth.generate(n_chr=1, chr_len=length, snps_per_chr=k, n=16, seed=170 + i, chr_names=[f"t{i}"],
                               sweeps_per_chr=1 if k >= 64 else 0, folded=0.3 if k >= 64 else 0.0,
                               missing=0.2 if k >= 64 else 0.0, max_missing=2)
    snp = tmp / "tiny.snp"
    synth.write_snp_file(str(snp), chrs)
    cells = check_grid_scan(snp, 1000, 20000, "tiny")
    assert any((e - a) % 1000 for _, a, e in cells), "no cell with an appended end"


def test_grid_spacing_must_divide(built, tmp):
    snp = tmp / "g.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=1, chr_len=200_000, snps_per_chr=300, n=16, seed=5))
    r = subprocess.run([str(CLI), "-f", str(snp), "-o", str(tmp / "o.txt"), "--scan-mode=grid", "-g", "3000", "-G", "50000"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "evenly divide" in r.stderr + r.stdout


# ------------------------------------------------------------------ 5-8. the whole grid job
G_JOB, g_JOB = 50000, 5000


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """One 600 kb chromosome, 1 500 SNPs, one planted sweep: 12 cells x 11 positions."""
    d = tmp_path_factory.mktemp("gjob")
    snp = d / "job.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=1, chr_len=600_000, snps_per_chr=1500, n=20, seed=JOB_SEED,
                                                   sweeps_per_chr=1))
    return dict(dir=d, snp=snp, want={})


JOB_SEED = 7


def oracle_job(job, n_perm):
    """The trial loop (scan-chromosome.c:441-502) restated over the oracle's functions, a cell's
    search_maxpos replaced by its grid maximum on the permuted SNPs; per point (fields, permute_n,
    permute_p, permute_finished, saved float CLRs)."""
    if n_perm in job["want"]:
        return job["want"][n_perm]
    scan, _ = setup(job["snp"])
    cells = scan_cells(scan, G_JOB)
    o = Oracle(job["snp"])
    L = o.o.L
    pts = [dict(pt=first_max(o.points(cell_positions(c, g_JOB))), n=0, p=0, fin=0, clr=[]) for c in cells]
    g = OrcRand()
    L.orc_srand(C.byref(g), SEED)
    L.orc_rand(C.byref(g))  # scan-chromosome.c:440: the usleep draw
    act, trial = list(range(len(pts))), -1
    while True:
        o.permute(g)
        trial += 1
        act = [i for i in act if not pts[i]["fin"]]
        if not act or trial > n_perm:
            break
        for i in act:
            q = pts[i]
            clr = first_max(o.points(cell_positions(cells[i], g_JOB), permuted=True))[CLR]
            if clr >= q["pt"][CLR]:
                q["p"] += 1
                if q["p"] >= 20 and q["p"] / float(q["n"]) >= L.orc_rand(C.byref(g)) / (2147483647 + 1.0):
                    q["fin"] = 1
            if q["n"] < SAVE:
                q["clr"].append(np.float32(clr))
            q["n"] += 1
    job["want"][n_perm] = (cells, pts, trial)
    return job["want"][n_perm]


def job_result(scan):
    """The product's points in the layout of oracle_job's."""
    s = scan.contents
    arr = fscl_amd.points(scan)
    out = []
    for i, row in enumerate(rows_of(arr)):
        q = s.scan_pts[i]
        out.append(dict(pt=row, n=q.permute_n, p=q.permute_p, fin=q.permute_finished,
                        clr=[np.float32(q.permute_clr[k]) for k in range(min(q.permute_n, SAVE))]))
    return out


def assert_job_equal(got, want, what):
    assert_points_equal([q["pt"] for q in got], [q["pt"] for q in want], what)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a["n"], a["p"], a["fin"]) == (b["n"], b["p"], b["fin"]), f"{what}: point {i}: {a['n'], a['p'], a['fin']} != {b['n'], b['p'], b['fin']}"
        assert np.array(a["clr"], dtype=np.float32).tobytes() == np.array(b["clr"], dtype=np.float32).tobytes(), \
            f"{what}: point {i}: saved CLRs differ"


def run_job(job, n_perm):
    return fscl_amd.run(job["snp"], None, n_permute=n_perm, large_grid_sp=G_JOB, small_grid_sp=g_JOB, scan_mode="grid")


def test_whole_grid_job(built, job):
    cells, want, trials = oracle_job(job, 60)
    assert len(cells) == 12 and all(len(cell_positions(c, g_JOB)) == 11 for c in cells)
    # (conditions on the input, on the oracle's result alone: a point pruned before the last trial,
    # and a point that ran every trial)
    assert any(q["fin"] and q["n"] < 61 for q in want), [(q["n"], q["p"]) for q in want]
    assert any(q["n"] == 61 for q in want), [(q["n"], q["p"]) for q in want]
    fscl_amd.reset_stats()
    scan = run_job(job, 60)
    assert_job_equal(job_result(scan), want, "grid job")
    st = fscl_amd.get_stats()
    assert st["trials"] == max(q["n"] for q in want)
    assert st["gp_evals"] == 11 * (12 + sum(q["n"] for q in want))


def test_two_devices_in_one_process(built, job):
    cells, want, _ = oracle_job(job, 60)
    fscl_amd.set_devices([0, 0])
    try:
        scan = run_job(job, 60)
        assert fscl_amd.get_lib().fscl_amd_n_devices() == 2
        two = job_result(scan)
    finally:
        fscl_amd.set_device(0)
    assert_job_equal(two, want, "two devices")
    assert_job_equal(two, job_result(run_job(job, 60)), "two devices vs one")


def test_cli_grid_mode(built, job, tmp):
    cells, want, _ = oracle_job(job, 10)
    base = [str(CLI), "-f", str(job["snp"]), "-G", str(G_JOB), "-g", str(g_JOB), "--n-permute=10"]
    r = subprocess.run(base + ["--scan-mode=grid", "-o", str(tmp / "g.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "scan mode grid" in r.stderr + r.stdout
    scan, _ = setup(job["snp"])
    name = scan.contents.chr_limits[0].name.decode()
    f = {k: i for i, k in enumerate(FIELDS)}
    text = ""
    for q in want:
        w = q["pt"]
        pv = 1.0 / q["n"] if q["p"] < 2 else (q["p"] - 1.0) / (q["n"] - 1.0)
        text += "%s\t%d\t%1.2f\t%1.3e\t%d\t%d\t%1.3f\n" % (name, w[f["sweep_pos"]], w[f["clr"]], math.exp(w[f["lalpha"]]),
                                                          q["p"], q["n"], -math.log10(pv))
    assert (tmp / "g.txt").read_text() == text
    # without --scan-mode (and with bisection named): the default mode's output
    fscl_amd.run(job["snp"], tmp / "ref.txt", n_permute=10, large_grid_sp=G_JOB)
    for k, extra in enumerate(([], ["--scan-mode=bisection"])):
        r = subprocess.run(base + extra + ["-o", str(tmp / f"d{k}.txt")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert (tmp / f"d{k}.txt").read_bytes() == (tmp / "ref.txt").read_bytes()


@pytest.mark.parametrize("extra,env,msg", [
    (["--scan-mode=fine"], {}, "--scan-mode must be bisection or grid"),
    (["--scan-mode=grid", "--permute-mode=throughput"], {}, "parity stream only"),
    (["--scan-mode=grid"], {"WORLD_SIZE": "2", "RANK": "0"}, "one process"),
])
def test_cli_refuses(built, job, tmp, extra, env, msg):
    import os
    r = subprocess.run([str(CLI), "-f", str(job["snp"]), "-G", str(G_JOB), "-g", str(g_JOB), "--n-permute=3", "-o",
                        str(tmp / "x.txt")] + extra, capture_output=True, text=True, timeout=120, env={**os.environ, **env})
    assert r.returncode != 0
    assert msg in r.stderr + r.stdout
    assert not (tmp / "x.txt").exists()


def test_state_after_the_grid_test(built, job, tmp):
    """After scan_permute_grid, the bisection scan + scan_permute(4) and scan_profile give what a
    fresh process gives; scan_permute_grid on scan_chromosome's own points is refused."""
    code = ("import sys; sys.path.insert(0, %r); import fscl_amd, numpy as np\n"
            "s = fscl_amd.run(%r, None, n_permute=4, large_grid_sp=%d)\n"
            "sys.stdout.buffer.write(fscl_amd.points(s).tobytes())\n" % (str(ROOT), str(job["snp"]), G_JOB))
    fresh = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=600)
    assert fresh.returncode == 0, fresh.stderr.decode()
    scan, tab = setup(job["snp"])
    p0 = fscl_amd.scan_profile(scan, tab, small_grid_sp=g_JOB, large_grid_sp=G_JOB)
    fscl_amd.srand()
    fscl_amd.set_permute_mode("parity")
    fscl_amd.scan_chromosome_grid(scan, tab, small_grid_sp=g_JOB, large_grid_sp=G_JOB)
    fscl_amd.scan_permute_grid(scan, tab, 5, small_grid_sp=g_JOB, large_grid_sp=G_JOB)
    assert fscl_amd.scan_profile(scan, tab, small_grid_sp=g_JOB, large_grid_sp=G_JOB).tobytes() == p0.tobytes()
    fscl_amd.srand()
    fscl_amd.scan_chromosome(scan, tab, large_grid_sp=G_JOB)
    fscl_amd.scan_permute(scan, tab, 4, large_grid_sp=G_JOB)
    assert fscl_amd.points(scan).tobytes() == fresh.stdout
    # the refusal is fatal (the library exits, as logmsg(MSG_FATAL) does): in a child process
    code = ("import sys; sys.path.insert(0, %r); import fscl_amd\n"
            "L = fscl_amd.get_lib(); L.configure_logmsg(1); fscl_amd.init_log_table()\n"
            "s = fscl_amd.load_snp_input(%r); f = fscl_amd.background_fsp(s)\n"
            "t = fscl_amd.compute_sweep_model_tables(s, f); fscl_amd.compute_snp_null_model(s, f)\n"
            "fscl_amd.scan_chromosome(s, t, large_grid_sp=%d)\n"
            "fscl_amd.scan_permute_grid(s, t, 3, small_grid_sp=%d, large_grid_sp=%d)\n"
            "print('NOT REFUSED')\n" % (str(ROOT), str(job["snp"]), G_JOB, g_JOB, G_JOB))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout
    assert "fscl_amd_scan_chromosome_grid" in r.stderr + r.stdout
