"""The alpha likelihood curves (fsclg_curve_submit, --alpha-file) on the GPU.

Every sm[k] of a curve is compared by bit pattern (NaN equal to NaN) with the plain sequential
reference of tests/walk_ref.py -- the null sum plus the walk's terms in walk order -- and the
curve's first strict maximum with the compiled oracle's search_maxalpha.
"""
from __future__ import annotations

import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import fscl_amd
import walk_ref as wr
from fscl_amd import synth
from util import CLI, GOLD, ROOT, read_dump, same_bits

sys.path.insert(0, str(ROOT / "oracle"))
import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

PT_FIELDS = ("chr", "nearest_snp", "sweep_pos", "n_snps", "window_start", "window_end", "null_logl", "lalpha",
             "sm_logl", "clr")
SENTINEL = 0xA5


def argmax_of(rec):
    """search_maxalpha's two loops over the curve: the first strict maximum in evaluation order
    from the -DBL_MAX / LOG_AD_MAX state (sm-search.c:272-298)."""
    best, la = -wr.DBL_MAX, wr.LOG_AD_MAX
    for k in range(int(rec["n_coarse"]) + int(rec["n_refine"])):
        if rec["sm"][k] > best:
            best, la = float(rec["sm"][k]), float(rec["la"][k])
    return la, best


def expected_curve(T, pt):
    """(la list, sm list) of the sequential reference: the coarse list, then the refine list of the
    coarse winner wr.search finds (its Diag keeps every walk's sequential sum)."""
    coarse, refine = wr.alpha_grid()
    D = wr.search(T, pt)[3]
    best, ci = -wr.DBL_MAX, len(coarse)
    for j, s in enumerate(D.sums[0]):
        if s > best:
            best, ci = s, j
    return list(coarse) + list(refine[ci]), list(D.sums[0]) + list(D.sums[1])


def check_record(rec, T, what, bad):
    """One record against the sequential reference on the record's own geometry; the argmax is the point's."""
    q = rec["pt"]
    pt = wr.Point(int(q["nearest_snp"]), int(q["sweep_pos"]), int(q["window_start"]), int(q["window_end"]),
                  float(q["null_logl"]))
    la, sm = expected_curve(T, pt)
    n = int(rec["n_coarse"]) + int(rec["n_refine"])
    if int(rec["n_coarse"]) != 11 or n != len(la):
        bad.append(f"{what}: {int(rec['n_coarse'])} + {int(rec['n_refine'])} entries, expected {len(la)}")
        return
    for k in range(n):
        if not wr.same(float(rec["la"][k]), la[k]):
            bad.append(f"{what} la[{k}]: {rec['la'][k]!r} != {la[k]!r}")
        if not wr.same(float(rec["sm"][k]), sm[k]):
            bad.append(f"{what} sm[{k}] (la {la[k]!r}): {float(rec['sm'][k]).hex()} != {float(sm[k]).hex()}")
    if rec["la"][n:].any() or rec["sm"][n:].any():
        bad.append(f"{what}: entries past n_coarse + n_refine are not zero")
    ala, asm = argmax_of(rec)
    if not (wr.same(ala, float(q["lalpha"])) and wr.same(asm, float(q["sm_logl"]))):
        bad.append(f"{what}: argmax ({ala!r}, {asm!r}) != point ({q['lalpha']!r}, {q['sm_logl']!r})")


def no_sentinel(arr, what):
    words = arr.view(np.uint8).reshape(len(arr), -1).view(np.uint32)
    assert not (words == int.from_bytes(bytes([SENTINEL] * 4), "little")).any(), f"{what}: a record was left unwritten"


def sentinel_array(n):
    out = np.zeros(max(n, 1), dtype=fscl_amd.CURVE_DTYPE)
    out.view(np.uint8)[:] = SENTINEL
    return out


# ------------------------------------------------------------------ 1. crafted terms, the shim alone
class CurveShim(wr.Shim):
    def __init__(self):
        super().__init__()
        L, vp = self.L, C.c_void_p
        L.fsclg_curve_submit.restype, L.fsclg_curve_submit.argtypes = C.c_int, [vp, C.c_int, C.c_int, C.POINTER(wr.RunT),
                                                                                C.c_int, C.c_int]
        L.fsclg_curve_wait.restype, L.fsclg_curve_wait.argtypes = C.c_int, [vp, C.c_int, vp]
        L.fsclg_curve_forced.restype, L.fsclg_curve_forced.argtypes = C.c_ulonglong, [vp]
        L.fsclg_slot_set_rows.restype, L.fsclg_slot_set_rows.argtypes = C.c_int, [vp, C.c_int, vp, vp]

    def curves(self, runs, eval_range):
        run = (wr.RunT * len(runs))(*[wr.RunT(*r) for r in runs])
        out = sentinel_array(sum(r[3] for r in runs))
        self._ok(self.L.fsclg_slot_set_rows(self.ctx, 0, None, None), "fsclg_slot_set_rows")  # the uploaded rows
        self._ok(self.L.fsclg_curve_submit(self.ctx, 0, 0, run, len(runs), eval_range), "fsclg_curve_submit")
        self._ok(self.L.fsclg_curve_wait(self.ctx, 0, out.ctypes.data), "fsclg_curve_wait")
        return out[:sum(r[3] for r in runs)]

    def forced(self) -> int:
        return int(self.L.fsclg_curve_forced(self.ctx))


@pytest.fixture(scope="module")
def shim(built):
    s = CurveShim()
    yield s
    s.close()


CASE_ER = 5000  # above every window of the geometry: each chromosome is one whole-chromosome window


def case_chromosomes():
    """The 15 windows of walk_ref.geometry() as 15 chromosomes (each runs up to the next window's
    first site: the sites between two windows have the all-zero row)."""
    g, n = wr.geometry()
    start = [q.ws for q in g]
    return start, [b - a for a, b in zip(start, start[1:] + [n])]


@pytest.mark.parametrize("name", list(wr.cases()))
def test_crafted_terms_every_alpha(shim, name):
    """Each point of the crafted cases as a position of its own chromosome, the chromosome's null sum
    set to the case's N: every entry of the curve is the sequential sum, the point is the profile's,
    and the forced-exact pass ran where walks were left inexact."""
    c = wr.cases()[name]
    g, _ = wr.geometry()
    cs, cn = case_chromosomes()
    runs = [(k, q.sweep, 1, 1) for k, q in enumerate(g)]
    Ns = list({wr.bits(p.null_logl): p.null_logl for p in c.points}.values())  # (by bit pattern: 0.0 and -0.0 both)
    bad, forced, unsafe, slow = [], 0, 0, 0
    try:
        shim.upload(c.tables, cs, cn)
        for N in Ns:
            shim.set_chr_null(N, len(cs))
            prof = shim.profile(runs, eval_range=CASE_ER)
            shim.reset_stats()
            got = shim.curves(runs, CASE_ER)
            forced += shim.forced()
            unsafe += shim.stats()["n_unsafe"]
            slow += shim.stats()["n_slow"]
            no_sentinel(got, name)
            for k, (rec, (pp, pv)) in enumerate(zip(got, prof)):
                q = rec["pt"]
                geo = (int(q["nearest_snp"]), int(q["sweep_pos"]), int(q["window_start"]), int(q["window_end"]))
                if geo != (pp.nearest_snp, pp.sweep_pos, pp.window_start, pp.window_end) or int(q["chr"]) != k or \
                        not all(wr.same(float(q[f]), v) for f, v in zip(("null_logl", "lalpha", "sm_logl", "clr"),
                                                                        (pp.null_logl,) + tuple(pv))):
                    bad.append(f"N={N!r} point {k}: record point {q} != profile {pp} {pv}")
                if not wr.same(float(q["null_logl"]), N):
                    bad.append(f"N={N!r} point {k}: null_logl {q['null_logl']!r}")
                check_record(rec, c.tables, f"N={N!r} point {k}", bad)
    except RuntimeError as e:  # a device error: nothing more runs on the GPU in this session
        pytest.exit(f"{name}: {e}", returncode=3)
    print(f"COUNTERS curve {name}: forced={forced} n_unsafe={unsafe} n_slow={slow}")
    # n_unsafe counts the walks left inexact by the integer path, n_slow those of them an argmax had to
    # settle: the rest lose whatever their exact value, and are exact only through the new pass.  (Where the
    # candidates are nearly equal -- edge-up-tiny -- the argmax settles every one of them and none is forced.)
    assert forced <= max(unsafe - slow, 0), f"{name}: {forced} forced walks of {unsafe} - {slow}"
    if c.want.get("n_unsafe") and unsafe > slow and c.regime != "nonfinite":
        assert forced > 0, f"{name}: no walk was forced exact"
    if c.want.get("n_unsafe") is False:  # every walk safe: nothing to force
        assert forced == 0, f"{name}: {forced} forced walks"
    assert not bad, f"{name}: {len(bad)} mismatches:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ helpers of the whole-library tests
def setup(snp):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    scan = fscl_amd.load_snp_input(snp)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp)
    fscl_amd.compute_snp_null_model(scan, fsp)
    return scan, tab


class OrcChr(C.Structure):  # orc_chr_t
    _fields_ = [("chr", C.c_int), ("name", C.c_char_p), ("start_index", C.c_int), ("n_snps", C.c_int),
                ("start_pos", C.c_int), ("bp_length", C.c_int)]


class Oracle:
    """orc_init_scan_result + orc_search_maxalpha per position (as test_grid_permute_gpu composes them)."""

    def __init__(self, snp, eval_range=81920):
        self.o = orc.OracleScan(snp)
        L = self.o.L
        L.orc_init_scan_result.argtypes = [C.POINTER(orc.OrcPt), C.c_int, C.c_void_p, C.POINTER(OrcChr), C.c_int, C.c_int,
                                           C.POINTER(orc.OrcStats)]
        L.orc_init_scan_result.restype = None
        L.orc_search_maxalpha.argtypes = [C.POINTER(orc.OrcPt), C.c_void_p, C.c_void_p, C.POINTER(orc.OrcStats)]
        L.orc_search_maxalpha.restype = None
        self.er = eval_range

    def points(self, chr_pos):
        L, s, st = self.o.L, self.o.s.contents, self.o.stats
        lim = C.cast(s.chr, C.POINTER(OrcChr))
        out = []
        for ch, pos in chr_pos:
            pt = orc.OrcPt()
            L.orc_init_scan_result(C.byref(pt), int(ch), s.snps, C.byref(lim[int(ch)]), self.er, int(pos), C.byref(st))
            L.orc_search_maxalpha(C.byref(pt), s.snps, self.o.tab, C.byref(st))
            out.append(tuple(getattr(pt, k) for k in PT_FIELDS))
        return out


def assert_argmax_is_oracle(curves, want, what):
    assert len(curves) == len(want)
    for i, (rec, w) in enumerate(zip(curves, want)):
        for k, f in enumerate(PT_FIELDS):
            x, y = rec["pt"][f].item(), w[k]
            assert same_bits(x, y) if isinstance(x, float) else x == y, f"{what}: point {i} {f}: {x!r} != {y!r}"
        la, sm = argmax_of(rec)
        assert same_bits(la, w[PT_FIELDS.index("lalpha")]) and same_bits(sm, w[PT_FIELDS.index("sm_logl")]), \
            f"{what}: point {i}: curve argmax ({la!r}, {sm!r}) != oracle {w}"


# ------------------------------------------------------------------ 2. against the compiled oracle
def test_argmax_is_the_oracles_golden(built):
    pts = read_dump(GOLD / "g2_p30.dump")
    chr_pos = [(r[0], r[1]) for r in pts]
    scan, tab = setup(GOLD / "g2.snp")
    got = fscl_amd.scan_curves(scan, tab, chr_pos)
    assert_argmax_is_oracle(got, Oracle(GOLD / "g2.snp").points(chr_pos), "g2")
    for rec, r in zip(got, pts):  # the golden points themselves: sweep_pos is a fixed point of init_scan_result
        assert same_bits(float(rec["pt"]["lalpha"]), r[3]) and same_bits(float(rec["pt"]["sm_logl"]), r[4])


@pytest.fixture(scope="module")
def window_case(tmp_path_factory):
    """2 000 SNPs with one planted sweep and a 500-SNP chromosome; eval_range 300: window null sums
    on the first, the whole-chromosome sum on the second."""
    d = tmp_path_factory.mktemp("curvewin")
    chrs = synth.generate(n_chr=1, chr_len=2_000_000, snps_per_chr=2000, n=16, seed=182, sweeps_per_chr=1, chr_names=["a"])
    chrs += synth.generate(n_chr=1, chr_len=500_000, snps_per_chr=500, n=16, seed=63, chr_names=["b"])
    snp = d / "win.snp"
    synth.write_snp_file(str(snp), chrs)
    return dict(snp=snp)


def test_argmax_is_the_oracles_windows(built, window_case):
    er = 300
    chr_pos = [(0, 3_000 + 66_077 * k) for k in range(30)] + [(1, 1_000 + 49_000 * k) for k in range(10)]
    scan, tab = setup(window_case["snp"])
    s = scan.contents
    assert s.chr_limits[0].n_snps > 2 * er + 1 >= s.chr_limits[1].n_snps
    got = fscl_amd.scan_curves(scan, tab, chr_pos, er)
    assert_argmax_is_oracle(got, Oracle(window_case["snp"], er).points(chr_pos), "windows")
    T = wr.OracleTables(window_case["snp"]).tables
    bad = []
    for i in range(0, len(got), 3):  # every entry, on the product's real tables
        check_record(got[i], T, f"position {chr_pos[i]}", bad)
    assert not bad, "\n".join(bad[:12])


# ------------------------------------------------------------------ 3. chunk edges
@pytest.mark.parametrize("chunk", [None, 1, 3])
def test_chunk_edges(built, window_case, monkeypatch, chunk):
    """Runs of 1, 2, 3, CH-1, CH, CH+1 and 2*CH+1 positions and an empty run in one call: the
    records do not depend on the chunk length, and every record's point is the profile's."""
    if chunk is None:
        monkeypatch.delenv("FSCLG_PROFILE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("FSCLG_PROFILE_CHUNK", str(chunk))
    assert fscl_amd.profile_chunk() == (chunk or fscl_amd.profile_chunk())
    monkeypatch.delenv("FSCLG_PROFILE_CHUNK", raising=False)
    dflt = fscl_amd.profile_chunk()
    if chunk is not None:
        monkeypatch.setenv("FSCLG_PROFILE_CHUNK", str(chunk))
    runs, a = [], 20_000
    for n in (1, 2, 3, dflt - 1, 0, dflt, dflt + 1, 2 * dflt + 1):
        runs.append((0, a, 1500, n))
        a += 1500 * n + 777
    scan, tab = setup(window_case["snp"])
    total = sum(r[3] for r in runs)
    got = fscl_amd.curve_runs(scan, tab, runs, 300, out=sentinel_array(total))
    assert len(got) == total
    no_sentinel(got, f"chunk {chunk}")
    prof = fscl_amd.profile_runs(scan, tab, runs, 300)
    for f in PT_FIELDS:
        assert got["pt"][f].tobytes() == prof[f].tobytes(), f
    got["pt"]["cost"] = 0  # (the terms the point's chunk had spent: a scheduling hint that depends on the chunk)
    if "records" not in window_case:
        window_case["records"] = got.tobytes()
        bad = []
        T = wr.OracleTables(window_case["snp"]).tables
        for i in range(0, total, 7):
            check_record(got[i], T, f"record {i}", bad)
        assert not bad, "\n".join(bad[:12])
    assert got.tobytes() == window_case["records"], f"chunk {chunk}: the records depend on the chunk length"


# ------------------------------------------------------------------ 4. permuted rows in a non-zero slot
def test_permuted_rows_in_another_slot(built, tmp):
    """The sites' rows rearranged within their chromosomes, set into slot 1: the curves are the
    sequential reference's on the rearranged sites; a profile taken before equals one taken after."""
    er = 300
    chrs = synth.generate(n_chr=1, chr_len=4_000_000, snps_per_chr=4000, n=20, seed=61, chr_names=["a"], sweeps_per_chr=1)
    chrs += synth.generate(n_chr=1, chr_len=500_000, snps_per_chr=500, n=20, seed=63, chr_names=["c"])
    snp = tmp / "perm.snp"
    synth.write_snp_file(str(snp), chrs)
    scan, tab = setup(snp)
    s = scan.contents
    rng = np.random.default_rng(4)
    perm = np.concatenate([s.chr_limits[c].start_index + rng.permutation(s.chr_limits[c].n_snps) for c in range(2)])
    rows = fscl_amd.site_rows(scan, tab)
    runs = [(0, 10_000, 350_000, 11), (0, 3_990_000, 1000, 3), (1, 5_000, 98_000, 5)]
    before = fscl_amd.scan_profile(scan, tab, er, 20_000, 400_000)
    got = fscl_amd.curve_runs(scan, tab, runs, er, rows=rows[perm])
    plain = fscl_amd.curve_runs(scan, tab, runs, er)
    after = fscl_amd.scan_profile(scan, tab, er, 20_000, 400_000)
    assert before.tobytes() == after.tobytes()
    assert got.tobytes() != plain.tobytes()
    O = wr.OracleTables(snp)
    T = O.tables
    # the device row r of a site is its flattened table row in the library's own numbering: map it
    # through the sites (site i has device row rows[i] and reference row T.row[i])
    dev2ref = {}
    for d, r in zip(rows.tolist(), T.row.tolist()):
        assert dev2ref.setdefault(d, r) == r or same_rows(T, dev2ref[d], r)
    Tp = wr.Tables(T.pos, np.array([dev2ref[d] for d in rows[perm].tolist()], dtype=np.uint32), T.coef, T.nullrow,
                   T.log_table, T.step)
    bad = []
    for i, rec in enumerate(plain):
        check_record(rec, T, f"uploaded rows, record {i}", bad)
    for i, rec in enumerate(got):
        check_record(rec, Tp, f"permuted rows, record {i}", bad)
    assert not bad, "\n".join(bad[:12])


def same_rows(T, a, b):
    return T.coef[a].tobytes() == T.coef[b].tobytes() and wr.same(float(T.nullrow[a]), float(T.nullrow[b]))


# ------------------------------------------------------------------ 5. the whole path
G_JOB, g_JOB = 50000, 5000


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """One 600 kb chromosome, 1 500 SNPs, one planted sweep (the grid tests' job)."""
    d = tmp_path_factory.mktemp("curvejob")
    snp = d / "job.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=1, chr_len=600_000, snps_per_chr=1500, n=20, seed=7,
                                                   sweeps_per_chr=1))
    return dict(dir=d, snp=snp)


def parse_alpha_file(path):
    """[(chr name, pos, [(alpha text, stat text, mark)], summary fields)] per point."""
    out = []
    for line in path.read_text().splitlines():
        f = line.split("\t")
        if f[2] == "support":
            out[-1][3].extend(f[3:])
            continue
        if not out or out[-1][3]:
            out.append((f[0], int(f[1]), [], []))
        out[-1][2].append((f[2], f[3], f[4]))
    return out


@pytest.mark.parametrize("mode", ["bisection", "grid"])
def test_whole_path(built, job, mode):
    d = job["dir"]
    kw = dict(large_grid_sp=G_JOB, small_grid_sp=g_JOB, scan_mode=mode, n_permute=5)
    s0 = fscl_amd.run(job["snp"], d / f"o0_{mode}.txt", **kw)
    p0 = fscl_amd.points(s0).tobytes()
    s1 = fscl_amd.run(job["snp"], d / f"o1_{mode}.txt", alpha_file=d / f"a_{mode}.txt", **kw)
    assert fscl_amd.points(s1).tobytes() == p0, "the permutation test's stream was disturbed"
    assert (d / f"o0_{mode}.txt").read_bytes() == (d / f"o1_{mode}.txt").read_bytes()
    # the scan points as they were before the test, and their curves
    s2 = fscl_amd.run(job["snp"], None, large_grid_sp=G_JOB, small_grid_sp=g_JOB, scan_mode=mode)
    pts = fscl_amd.points(s2)
    scan, tab = setup(job["snp"])
    if mode == "grid":
        fscl_amd.scan_chromosome_grid(scan, tab, small_grid_sp=g_JOB, large_grid_sp=G_JOB)
    else:
        fscl_amd.scan_chromosome(scan, tab, large_grid_sp=G_JOB)
    cv = fscl_amd.scan_point_curves(scan, tab)
    assert len(cv) == len(pts) == 12
    for rec, p in zip(cv, pts):
        la, sm = argmax_of(rec)
        assert same_bits(la, float(p["lalpha"])) and same_bits(sm, float(p["sm_logl"]))
        for f in PT_FIELDS:
            assert rec["pt"][f].tobytes() == p[f].tobytes(), f
    fscl_amd.curve_output(d / f"b_{mode}.txt", scan, cv, 2.0)
    assert (d / f"a_{mode}.txt").read_bytes() == (d / f"b_{mode}.txt").read_bytes()
    rows = parse_alpha_file(d / f"a_{mode}.txt")
    assert len(rows) == 12
    for (name, pos, ent, summ), rec in zip(rows, cv):
        assert pos == int(rec["pt"]["sweep_pos"]) and [m for _, _, m in ent].count("*") == 1 and len(summ) == 4
        assert [float(a) for a, _, _ in ent] == sorted(float(a) for a, _, _ in ent)
        assert len(ent) == len(set(rec["la"][:int(rec["n_coarse"]) + int(rec["n_refine"])].tolist()))
    job[mode] = (d / f"a_{mode}.txt").read_bytes()


def test_two_devices_give_the_same_file(built, job):
    d = job["dir"]
    fscl_amd.set_devices([0, 0])
    try:
        fscl_amd.run(job["snp"], None, large_grid_sp=G_JOB, alpha_file=d / "two.txt")
        assert fscl_amd.get_lib().fscl_amd_n_devices() == 2
    finally:
        fscl_amd.set_device(0)
    fscl_amd.run(job["snp"], None, large_grid_sp=G_JOB, alpha_file=d / "one.txt")
    assert (d / "two.txt").read_bytes() == (d / "one.txt").read_bytes()
    if "bisection" in job:
        assert job["bisection"] == (d / "one.txt").read_bytes()


def test_cli(built, job, tmp):
    base = [str(CLI), "-f", str(job["snp"]), "-G", str(G_JOB), "-g", str(g_JOB)]
    r = subprocess.run(base + ["-o", str(tmp / "o.txt"), f"--alpha-file={tmp / 'a.txt'}", "--n-permute=5"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    fscl_amd.run(job["snp"], tmp / "ref.txt", large_grid_sp=G_JOB, n_permute=5, alpha_file=tmp / "ref_a.txt")
    assert (tmp / "o.txt").read_bytes() == (tmp / "ref.txt").read_bytes()
    assert (tmp / "a.txt").read_bytes() == (tmp / "ref_a.txt").read_bytes()
    r = subprocess.run(base + ["-o", str(tmp / "x.txt"), f"--alpha-file={tmp / 'x_a.txt'}", "--no-scan"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--alpha-file needs the scan" in r.stderr + r.stdout
    assert not (tmp / "x_a.txt").exists()


# ------------------------------------------------------------------ 6. tiny chromosomes
def test_tiny_chromosomes(built, tmp):
    chrs = []
    for i, (k, length) in enumerate(((1, 50_000), (2, 90_000), (3, 150_000), (64, 700_000), (3000, 3_000_000))):
        chrs += synth.generate(n_chr=1, chr_len=length, snps_per_chr=k, n=16, seed=170 + i, chr_names=[f"t{i}"],
                               sweeps_per_chr=1 if k >= 64 else 0)
    snp = tmp / "tiny.snp"
    synth.write_snp_file(str(snp), chrs)
    scan, tab = setup(snp)
    s = scan.contents
    assert [s.chr_limits[c].n_snps for c in range(4)] == [1, 2, 3, 64]
    p1 = s.snps[s.chr_limits[0].start_index].pos
    runs = [(0, max(p1 - 3000, 0), 1000, 7), (1, 0, 30_000, 4), (2, 0, 37_500, 5), (3, 0, 100_000, 8), (0, p1, 1, 1)]
    total = sum(r[3] for r in runs)
    got = fscl_amd.curve_runs(scan, tab, runs, out=sentinel_array(total))
    no_sentinel(got, "tiny")
    assert (got["n_coarse"] == 11).all() and (got["n_refine"] >= 14).all()
    chr_pos = [(c, a + t * st) for c, a, st, n in runs for t in range(n)]
    assert_argmax_is_oracle(got, Oracle(snp).points(chr_pos), "tiny")
    T = wr.OracleTables(snp).tables
    bad = []
    for i in list(range(7)) + [total - 1] + list(range(7, total - 1, 4)):  # the one-SNP chromosome: every record
        check_record(got[i], T, f"record {i} {chr_pos[i]}", bad)
    assert not bad, "\n".join(bad[:12])
