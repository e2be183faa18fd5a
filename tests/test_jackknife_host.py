"""The host-only side of the delete-one-block jackknife (--jackknife-file): fscl_amd_jackknife_combine on
hand-made block sums, the writer's bytes, the refusals made before any device call, and
tools/jackknife_host_check.c under the sanitizers.  No GPU."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import blocks_ref as br
import fscl_amd
from util import GOLD, run_cli, run_host_check

NAN = math.nan
POS = [2000, 3000, 4000]
LA = [-3.0, -1.0]


def peak():
    """3 positions x 4 blocks x 2 alphas: block 1 carries the peak at position 1; without it position 2 wins;
    block 3 holds no term."""
    bs, cnt = np.zeros((3, 4, 2)), np.zeros((3, 4, 2), dtype=np.uint32)
    bs[:, 0, 0], cnt[:, 0, 0] = 1.0, 2
    bs[:, 2, 0], cnt[:, 2, 0] = 1.0, 1
    bs[1, 1, 0], cnt[1, 1, 0] = 10.0, 5
    bs[2, 2, 0] = 1.5
    return bs, cnt


def combine(bs, cnt, pos=POS, la=LA):
    blocks, summ = fscl_amd.jackknife_combine(bs, cnt, pos, la)
    bad = br.same_combine(blocks, summ, br.jackknife_combine(np.asarray(bs, dtype=np.float64), np.asarray(cnt), pos, la))
    assert not bad, "\n".join(bad)
    return blocks, summ


def test_combine_hand_computed(built):
    blocks, s = combine(*peak())
    assert (int(s["ipos"]), int(s["ila"]), float(s["v"]), int(s["g"])) == (1, 0, 12.0, 3)
    assert [int(b["has_terms"]) for b in blocks] == [1, 1, 1, 0]
    assert [(int(b["ipos"]), int(b["ila"]), float(b["v"])) for b in blocks[:3]] == [(1, 0, 11.0), (2, 0, 2.5), (1, 0, 11.0)]
    assert [int(b["n_terms"]) for b in blocks] == [2, 5, 1, 0]
    assert int(blocks[3]["ipos"]) == -1 and math.isnan(float(blocks[3]["v"]))
    # theta_b = 3000, 4000, 3000: se^2 = (g - 1) / g * sum (theta_b - mean)^2, bias = (g - 1) (mean - theta)
    mean = 10000.0 / 3.0
    assert float(s["se_pos"]) == pytest.approx(math.sqrt(2.0 / 3.0 * (2 * (3000 - mean) ** 2 + (4000 - mean) ** 2)), rel=1e-14)
    assert float(s["bias_pos"]) == pytest.approx(2.0 * (mean - 3000.0), rel=1e-12)
    assert float(s["se_la"]) == 0.0 and float(s["bias_la"]) == 0.0
    mc = (22.0 + 5.0 + 22.0) / 3.0
    assert float(s["se_clr"]) == pytest.approx(math.sqrt(2.0 / 3.0 * (2 * (22 - mc) ** 2 + (5 - mc) ** 2)), rel=1e-14)
    assert (int(s["top_shift"]), int(s["top_loss"])) == (1, 1)


def test_combine_edge_counts(built):
    """Position 0 or n_pos - 1 and alpha 0 or n_la - 1 are the grid's edges: the open_* warning."""
    blocks, s = combine(*peak())
    assert (int(s["n_edge_pos"]), int(s["n_edge_la"])) == (1, 3)  # block 1's maximum at position 2; every alpha 0 of 2
    bs, cnt = np.zeros((3, 2, 3)), np.ones((3, 2, 3), dtype=np.uint32)
    bs[1, :, 1] = 1.0  # the centre cell whichever block is left out
    blocks, s = combine(bs, cnt, la=[-3.0, -2.0, -1.0])
    assert (int(s["n_edge_pos"]), int(s["n_edge_la"])) == (0, 0) and float(s["se_pos"]) == 0.0


def test_combine_nan_cells(built):
    bs, cnt = peak()
    bs[1, 1, 0] = NAN  # the full surface's cell (1, 0) is NaN: it never wins
    blocks, s = combine(bs, cnt)
    assert (int(s["ipos"]), int(s["ila"]), float(s["v"])) == (2, 0, 2.5)
    assert (int(blocks[1]["ipos"]), float(blocks[1]["v"])) == (2, 2.5) and int(blocks[0]["ipos"]) == 2
    bs[:] = NAN
    blocks, s = combine(bs, cnt)
    assert int(s["ipos"]) == -1 and math.isnan(float(s["v"])) and math.isnan(float(s["se_pos"])) and int(s["g"]) == 3
    # one delete-one surface of NaN alone: its block has no estimate and no spread is reported
    bs, cnt = np.zeros((1, 2, 1)), np.ones((1, 2, 1), dtype=np.uint32)
    bs[0, 0, 0], bs[0, 1, 0] = 1.0, NAN
    blocks, s = combine(bs, cnt, pos=[10], la=[0.0])
    assert int(s["ipos"]) == -1 and int(blocks[1]["ipos"]) == 0 and float(blocks[1]["v"]) == 1.0 and int(blocks[0]["ipos"]) == -1


def test_combine_one_block_has_no_spread(built):
    bs, cnt = np.zeros((3, 4, 2)), np.zeros((3, 4, 2), dtype=np.uint32)
    bs[0, 2, 1], cnt[0, 2, 1] = 3.0, 1
    blocks, s = combine(bs, cnt)
    assert int(s["g"]) == 1 and (int(s["ipos"]), int(s["ila"])) == (0, 1)
    assert all(math.isnan(float(s[k])) for k in ("se_pos", "se_la", "se_clr", "bias_pos", "bias_la", "bias_clr"))


def test_combine_ties_first_wins(built):
    """Equal cells: the first in position order, then alpha order; deleting the only block leaves +0.0 everywhere."""
    bs, cnt = np.zeros((3, 2, 2)), np.ones((3, 2, 2), dtype=np.uint32)
    bs[1, 0, 1] = bs[2, 0, 0] = bs[1, 1, 0] = 7.0
    blocks, s = combine(bs, cnt)
    assert (int(s["ipos"]), int(s["ila"])) == (1, 0)          # V = 7 at (1, 0), (1, 1), (2, 0)
    assert (int(blocks[0]["ipos"]), int(blocks[0]["ila"])) == (1, 0) and (int(blocks[1]["ipos"]), int(blocks[1]["ila"])) == (1, 1)
    bs[:] = 0.0
    blocks, s = combine(bs, cnt)
    assert (int(s["ipos"]), int(s["ila"]), float(s["v"])) == (0, 0, 0.0) and float(s["se_pos"]) == 0.0


def test_combine_fold_order(built):
    """V_b is the fold over j != b in ascending j from +0.0: 1e16 + 1 + 1 - 1e16 is 0 in that order (not 2)."""
    bs, cnt = np.zeros((1, 5, 1)), np.ones((1, 5, 1), dtype=np.uint32)
    bs[0, :, 0] = [1e16, 1.0, 1.0, -1e16, 0.25]
    blocks, s = combine(bs, cnt, pos=[5], la=[0.0])
    assert float(s["v"]) == 0.25 and [float(b["v"]) for b in blocks] == [-9999999999999998.0, 0.25, 0.25, 1e16, 0.0]
    bs[0, 0, 0] = -0.0  # +0.0 + -0.0 is +0.0
    bs[0, 1:, 0] = -0.0
    blocks, s = combine(bs, cnt, pos=[5], la=[0.0])
    assert math.copysign(1.0, float(s["v"])) == 1.0


def test_combine_arguments(built):
    bs, cnt = peak()
    for bad in (dict(pos=POS[:2]), dict(la=LA[:1])):
        with pytest.raises(ValueError):
            fscl_amd.jackknife_combine(bs, cnt, **{**dict(pos=POS, la=LA), **bad})
    with pytest.raises(ValueError):
        fscl_amd.jackknife_combine(bs, cnt[:2], POS, LA)
    with pytest.raises(ValueError):
        fscl_amd.jackknife_combine(bs[:0], cnt[:0], [], LA)


# ------------------------------------------------------------------ the writer, requests without a device
@pytest.fixture(scope="module")
def scan(built):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    return fscl_amd.load_snp_input(GOLD / "g1.snp")


def make_blocks(bs, cnt, b0=1, block_bp=1000, la=(math.log(1e-4), math.log(1e-3))):
    hdr = np.zeros(1, dtype=fscl_amd.BLOCKS_DTYPE)[0]
    hdr["chr"], hdr["centre_pos"], hdr["n_la"], hdr["n_pos"], hdr["point"] = 0, 3000, bs.shape[2], bs.shape[0], 0
    hdr["nb"], hdr["b0"], hdr["block_bp"] = bs.shape[1], b0, block_bp
    hdr["la"][:len(la)] = la
    pts = np.zeros(bs.shape[0], dtype=fscl_amd._POINT_RAW)
    pts["sweep_pos"] = POS[:bs.shape[0]]
    return fscl_amd.Blocks(hdr, pts, bs, cnt)


def test_output_bytes(scan, tmp_path):
    name = scan.contents.chr_limits[0].name.decode()
    bk = make_blocks(*peak())
    fscl_amd.jackknife_output(tmp_path / "j.txt", scan, [bk], "L")
    want = "".join(f"L\t{name}\t3000\t{r}\n" for r in (
        "1000\t1999\t2\t3000\t1.000e-04\t22.00\t0\t0.0000\t-2.00",
        "2000\t2999\t5\t4000\t1.000e-04\t5.00\t1000\t0.0000\t-19.00",
        "3000\t3999\t1\t3000\t1.000e-04\t22.00\t0\t0.0000\t-2.00",
        "summary\t3\t2\t3\t3000\t1.000e-04\t24.00\t666.7\t0.0000\t11.33\t666.7\t0.0000\t2000\t2000\t1\t3"))
    assert (tmp_path / "j.txt").read_text() == want
    # a peak of NaN alone, and one whose single block leaves no spread; no label
    nan = make_blocks(np.full((1, 2, 1), NAN), np.ones((1, 2, 1), dtype=np.uint32), la=(0.0,))
    one = make_blocks(np.array([[[3.0]]]), np.ones((1, 1, 1), dtype=np.uint32), b0=7, block_bp=500, la=(0.0,))
    fscl_amd.jackknife_output(tmp_path / "n.txt", scan, [bk, nan, one])
    lines = (tmp_path / "n.txt").read_text().splitlines()
    assert len(lines) == 7 and lines[3] == want.splitlines()[3][2:]
    assert lines[4] == f"{name}\t3000\tsummary\t1\t1\t2\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\t0\t0"
    assert lines[5] == f"{name}\t3000\t3500\t3999\t1\t2000\t1.000e+00\t0.00\t0\t0.0000\t-6.00"
    assert lines[6] == f"{name}\t3000\tsummary\t1\t1\t1\t2000\t1.000e+00\t6.00\tNA\tNA\tNA\tNA\tNA\t3500\t3500\t1\t1"
    for ln in lines:
        assert len(ln.split("\t")) == (18 if "summary" in ln else 11)
    with pytest.raises(ValueError):
        fscl_amd.jackknife_output(tmp_path / "no-such-directory" / "x.txt", scan, [bk])
    fscl_amd.jackknife_output(tmp_path / "e.txt", scan, [])
    assert (tmp_path / "e.txt").read_bytes() == b""


def test_blocks_bound(scan):
    """The blocks of the widest windows a run's positions can have, from the sites alone."""
    s = scan.contents
    lim = s.chr_limits[0]
    a, n = int(lim.start_index), int(lim.n_snps)
    pos = np.array([s.snps[a + i].pos for i in range(n)], dtype=np.int64)
    mid = int(pos[n // 2])
    for er, bp, run in ((100, 5000, (0, mid - 3000, 1000, 7)), (10, 777, (0, int(pos[0]) - 50, 10, 3)),
                        (5, 1, (0, int(pos[-1]) + 9, 1, 1)), (81920, 50000, (0, mid, 1, 1))):
        first, last = run[1], run[1] + (run[3] - 1) * run[2]
        lo = max(int(np.searchsorted(pos, first, "left")) - 1, 0)
        hi = min(int(np.searchsorted(pos, last, "left")), n - 1)
        ws, we = max(min(lo - er, n - 1 - 2 * er), 0), min(max(hi + er, 2 * er), n - 1)
        assert fscl_amd.blocks_bound(scan, run, bp, er) == (int(pos[ws]) // bp, int(pos[we]) // bp - int(pos[ws]) // bp + 1)
    assert fscl_amd.blocks_bound(scan, (0, mid, 1000, 0), 5000) == (0, 1)
    for run, bp in (((0, mid, 0, 1), 100), ((-1, mid, 1, 1), 100), ((0, mid, 1, 1), 0)):
        with pytest.raises(ValueError):
            fscl_amd.blocks_bound(scan, run, bp)


def test_scan_blocks_refusals_before_any_device_call(scan, monkeypatch, capfd):
    """FSCLG_E_ARG (-1) with no tables set: too many blocks, a result above $FSCL_AMD_BLOCKS_CAP, bad requests."""
    L = fscl_amd.get_lib()
    res = fscl_amd.BlocksT()
    tab = C.cast(C.c_void_p(1), C.POINTER(fscl_amd.SmPtableT))  # (never dereferenced below)
    mid = int(scan.contents.chr_limits[0].bp_length) // 2
    req = fscl_amd._surface_requests([(0, mid, 2000, 1000, [0.0, 1.0])])
    assert L.fscl_amd_scan_blocks(None, tab, 81920, req.ctypes.data, 1, 1000, C.byref(res)) == -1
    assert L.fscl_amd_scan_blocks(scan, tab, 81920, req.ctypes.data, 1, 0, C.byref(res)) == -1      # block_bp < 1
    assert L.fscl_amd_scan_blocks(scan, tab, 81920, None, 1, 1000, C.byref(res)) == -1
    span = int(scan.contents.chr_limits[0].bp_length) - int(scan.contents.chr_limits[0].start_pos)
    assert span // 1025 > 100
    capfd.readouterr()
    assert L.fscl_amd_scan_blocks(scan, tab, 81920, req.ctypes.data, 1, span // 2000, C.byref(res)) == -1  # > 1024 blocks
    assert "--jackknife-block" in "".join(capfd.readouterr())
    assert fscl_amd.blocks_cap() == 2 ** 30
    monkeypatch.setenv("FSCL_AMD_BLOCKS_CAP", "1000")
    assert fscl_amd.blocks_cap() == 1000
    assert L.fscl_amd_scan_blocks(scan, tab, 81920, req.ctypes.data, 1, span // 20, C.byref(res)) == -1   # 5 x >= 10 x 2 x 12 B
    assert "FSCL_AMD_BLOCKS_CAP" in "".join(capfd.readouterr())
    monkeypatch.delenv("FSCL_AMD_BLOCKS_CAP")
    for la in ([0.0, 0.0], [1.0, 0.0], [-20.5, 0.0], [0.0, NAN]):
        bad = fscl_amd._surface_requests([(0, mid, 1000, 1000, la)])
        assert L.fscl_amd_scan_blocks(scan, tab, 81920, bad.ctypes.data, 1, 100000, C.byref(res)) == -1, la
        assert res.n == 0 and not res.hdr
    for args in ((-1, 1000, 1000, 50000), (3, 1000, 0, 50000), (3, -1, 1000, 50000), (3, 1000, 1000, 0)):
        top, hw, step, bp = args
        assert L.fscl_amd_scan_point_jackknife(scan, tab, 81920, top, hw, step, -20.0, 4.0, 33, bp, C.byref(res)) == -1, args


def test_host_check_under_sanitizers(built, tmp_path):
    """tools/jackknife_host_check.c: the block bound, the combination and the writer under ASan and UBSan, as a
    stand-alone program (no device library, nothing loaded into Python)."""
    run_host_check("jackknife_host_check", ["jackknife.c", "util.c"], tmp_path, [tmp_path])


# ------------------------------------------------------------------ the CLI's refusals
@pytest.mark.parametrize("args, msg", [
    (["--no-scan"], "--jackknife-file needs the scan"),
    (["--jackknife-top=-1"], "--jackknife-top must be >= 0"),
    (["--jackknife-block=0"], "--jackknife-block must be at least 1"),
    (["--jackknife-halfwidth=-5"], "--jackknife-halfwidth must be >= 0"),
    (["--jackknife-step=0"], "--jackknife-step must be at least 1"),
    (["--jackknife-alphas=-20:4:64"], "--jackknife-alphas must be LO:HI:N"),
    (["--jackknife-alphas=2:1:10"], "--jackknife-alphas must be LO:HI:N"),
])
def test_cli_refusals(built, tmp_path, args, msg):
    """Refused before the data is loaded: no device is touched and no file is written."""
    r = run_cli([f"--jackknife-file={tmp_path / 'j.txt'}"] + args, tmp_path, snp="g1.snp")
    assert r.returncode != 0 and msg in r.stderr + r.stdout, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "j.txt").exists() and not (tmp_path / "o.txt").exists()


def test_run_keyword_refusals(built):
    for kw in (dict(jackknife_top=-1), dict(jackknife_step=0), dict(jackknife_halfwidth=-1), dict(jackknife_block=0),
               dict(jackknife_alphas=(-20.0, 4.0, 64)), dict(surface_step=0)):
        with pytest.raises(ValueError):
            fscl_amd.run(GOLD / "g1.snp", None, jackknife_file="unused.txt", **kw)
