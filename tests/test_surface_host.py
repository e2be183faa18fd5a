"""The host-only side of the likelihood surfaces (--surface-file): the region summary, the writer, the
alpha list, a request's positions, the argument errors reached without a device and the CLI's refusals."""
from __future__ import annotations

import math

import numpy as np
import pytest

import fscl_amd
from util import GOLD, run_cli, run_host_check

NAN = math.nan


def region(a, drop=2.0):
    reg, mark = fscl_amd.surface_region(np.array(a, dtype=np.float64), drop)
    return {k: int(reg[k]) for k in reg.dtype.names if k not in ("max_v", "pad")}, float(reg["max_v"]), mark


# ------------------------------------------------------------------ surface_region
def test_region_single_ridge(built):
    a = [[0, 1, 2, 1, 0],
         [1, 4, 5, 4, 0],
         [0, 3.5, 9, 8, 1],
         [0, 1, 7.5, 6, 0],
         [0, 0, 1, 0, 0]]
    r, m, mark = region(a)
    assert (r["max_ipos"], r["max_ila"], m) == (2, 2, 9.0)
    assert mark.tolist() == [[0] * 5, [0] * 5, [0, 0, 2, 1, 0], [0, 0, 1, 0, 0], [0] * 5] and r["n_region"] == 3
    assert (r["ipos_lo"], r["ipos_hi"], r["ila_lo"], r["ila_hi"]) == (2, 3, 2, 3)
    assert not any(r[k] for k in ("open_pos_lo", "open_pos_hi", "open_la_lo", "open_la_hi"))
    assert region(a, 0.0)[0]["n_region"] == 1 and region(a, 100.0)[0]["n_region"] == 25


def test_region_first_maximum_wins_and_second_is_left_out(built):
    """Two equal maxima separated by a low column: the first in position order, then alpha order, is the
    argmax; the other lies within the drop but is not connected, so it is not in the region -- yet the alpha
    interval, a run of columns, is cut at the low column too."""
    a = [[9, 8, 0, 8.5, 9],
         [8, 7.5, 0, 7.5, 8]]
    r, m, mark = region(a)
    assert (r["max_ipos"], r["max_ila"]) == (0, 0) and m == 9.0
    assert mark.tolist() == [[2, 1, 0, 0, 0], [1, 1, 0, 0, 0]] and r["n_region"] == 4
    assert (r["ila_lo"], r["ila_hi"], r["open_la_lo"], r["open_la_hi"]) == (0, 1, 1, 0)
    assert (r["ipos_lo"], r["ipos_hi"], r["open_pos_lo"], r["open_pos_hi"]) == (0, 1, 1, 1)
    b = [[1, 9], [9, 1]]  # position order before alpha order
    assert region(b)[0]["max_ipos"] == 0 and region(b)[0]["max_ila"] == 1


@pytest.mark.parametrize("at, flag", [((0, 2), "open_pos_lo"), ((4, 2), "open_pos_hi"), ((2, 0), "open_la_lo"),
                                      ((2, 4), "open_la_hi")])
def test_region_open_flags(built, at, flag):
    a = np.zeros((5, 5))
    a[at] = 10.0
    r, _, _ = region(a)
    assert [k for k in ("open_pos_lo", "open_pos_hi", "open_la_lo", "open_la_hi") if r[k]] == [flag]


def test_region_nan(built):
    a = [[5, NAN, 5],
         [5, 9, NAN],
         [NAN, 8, 5]]
    r, m, mark = region(a, 100.0)  # every finite cell is above the cut
    assert m == 9.0 and mark.tolist() == [[1, 0, 0], [1, 2, 0], [0, 1, 1]] and r["n_region"] == 5
    r, m, mark = region([[NAN, NAN], [NAN, NAN]])
    assert math.isnan(m) and not mark.any() and r["n_region"] == 0
    assert all(r[k] == -1 for k in ("max_ipos", "max_ila", "ipos_lo", "ipos_hi", "ila_lo", "ila_hi"))
    assert not any(r[k] for k in ("open_pos_lo", "open_pos_hi", "open_la_lo", "open_la_hi"))
    r, m, mark = region([[3.5]])
    assert m == 3.5 and mark.tolist() == [[2]] and r["n_region"] == 1
    assert all(r[k] for k in ("open_pos_lo", "open_pos_hi", "open_la_lo", "open_la_hi"))


def test_region_null_sums_and_arguments(built):
    sm = np.array([[-100.0, -98.0], [-50.0, -49.5]])
    reg, mark = fscl_amd.surface_region(sm, 2.0, null_logl=[-101.0, -50.0])
    assert float(reg["max_v"]) == 3.0 and (int(reg["max_ipos"]), int(reg["max_ila"])) == (0, 1)
    assert mark.tolist() == [[1, 2], [0, 0]]
    for bad in (-1.0, NAN):
        with pytest.raises(ValueError):
            fscl_amd.surface_region(sm, bad)
    with pytest.raises(ValueError):
        fscl_amd.surface_region(np.zeros((0, 3)))
    with pytest.raises(ValueError):
        fscl_amd.surface_region(sm, 2.0, null_logl=[0.0])


# ------------------------------------------------------------------ the alpha list
def test_alpha_list_insertion(built):
    g = fscl_amd.surface_alphas()
    assert len(g) == 33 and g[0] == -20.0 and g[-1] == 4.0 and np.array_equal(np.diff(g), np.full(32, 0.75))
    assert np.array_equal(fscl_amd.surface_alphas(fitted=-20.0 + 0.75 * 11), g)      # equal to a grid value
    assert np.array_equal(fscl_amd.surface_alphas(fitted=-20.0), g) and np.array_equal(fscl_amd.surface_alphas(fitted=4.0), g)
    b = fscl_amd.surface_alphas(fitted=-3.3)                                          # between two values
    assert len(b) == 34 and list(b[22:25]) == [-3.5, -3.3, -2.75] and np.array_equal(np.delete(b, 23), g)
    lo = fscl_amd.surface_alphas(-10.0, 0.0, 5, -12.5)                                # at either end
    hi = fscl_amd.surface_alphas(-10.0, 0.0, 5, 1.5)
    assert list(lo) == [-12.5, -10.0, -7.5, -5.0, -2.5, 0.0] and list(hi) == [-10.0, -7.5, -5.0, -2.5, 0.0, 1.5]
    for f in (NAN, -20.5, 4.5, math.inf):                                             # nothing to insert
        assert np.array_equal(fscl_amd.surface_alphas(fitted=f), g)
    assert len(fscl_amd.surface_alphas(-20.0, 4.0, 63, 0.1)) == 64
    assert list(fscl_amd.surface_alphas(-3.0, -3.0, 1)) == [-3.0]
    for bad in ((-20.0, 4.0, 64), (-20.0, 4.0, 0), (-20.5, 4.0, 5), (-20.0, 4.5, 5), (1.0, 0.0, 5), (1.0, 1.0, 2),
                (NAN, 1.0, 2), (0.0, 1.0, 1)):
        with pytest.raises(ValueError):
            fscl_amd.surface_alphas(*bad)


# ------------------------------------------------------------------ requests, without a device
@pytest.fixture(scope="module")
def scan(built):
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    return fscl_amd.load_snp_input(GOLD / "g1.snp")


def test_request_positions(scan):
    lim = scan.contents.chr_limits[0]
    lo, hi = int(lim.start_pos), int(lim.bp_length)
    mid = (lo + hi) // 2
    assert fscl_amd.surface_run(scan, (0, mid, 2500, 1000, [0.0])) == (0, mid - 2000, 1000, 5)
    assert fscl_amd.surface_run(scan, (0, lo + 300, 2500, 1000, [0.0])) == (0, lo + 300, 1000, 3)   # clipped below
    assert fscl_amd.surface_run(scan, (0, hi - 300, 2500, 1000, [0.0])) == (0, hi - 2300, 1000, 3)  # clipped above
    assert fscl_amd.surface_run(scan, (0, hi, 0, 7, [0.0])) == (0, hi, 7, 1)
    assert fscl_amd.surface_run(scan, (0, hi + 5000, 1000, 1000, [0.0]))[3] == 0                   # nothing in the span
    for bad in ((0, mid, 1000, 0, [0.0]), (0, mid, -1, 1000, [0.0]), (-1, mid, 1000, 1000, [0.0]),
                (scan.contents.n_chromosomes, mid, 1000, 1000, [0.0])):
        with pytest.raises(ValueError):
            fscl_amd.surface_run(scan, bad)


def test_scan_surface_argument_errors(scan):
    """FSCLG_E_ARG (-1) before the first device call: no tables are needed to get there."""
    L = fscl_amd.get_lib()
    res = fscl_amd.SurfacesT()
    import ctypes as C
    tab = C.POINTER(fscl_amd.SmPtableT)()
    assert L.fscl_amd_scan_surface(None, tab, 81920, None, 0, C.byref(res)) == -1
    assert L.fscl_amd_scan_surface(scan, tab, 81920, None, 0, C.byref(res)) == -1          # no tables
    tab = C.cast(C.c_void_p(1), C.POINTER(fscl_amd.SmPtableT))                            # (never dereferenced below)
    assert L.fscl_amd_scan_surface(scan, tab, 81920, None, -1, C.byref(res)) == -1
    assert L.fscl_amd_scan_surface(scan, tab, 81920, None, 1, C.byref(res)) == -1
    mid = int(scan.contents.chr_limits[0].bp_length) // 2
    for la in ([0.0, 0.0], [1.0, 0.0], [-20.5, 0.0], [0.0, 4.5], [0.0, NAN]):
        req = fscl_amd._surface_requests([(0, mid, 1000, 1000, la)])
        assert L.fscl_amd_scan_surface(scan, tab, 81920, req.ctypes.data, 1, C.byref(res)) == -1, la
        assert res.n == 0 and not res.hdr
    for bad in ((0, mid, 1000, 0), (0, mid, -1, 1000), (-1, mid, 1000, 1000), (scan.contents.n_chromosomes, mid, 1000, 1000)):
        req = fscl_amd._surface_requests([bad + ([0.0, 1.0],)])
        assert L.fscl_amd_scan_surface(scan, tab, 81920, req.ctypes.data, 1, C.byref(res)) == -1, bad
    req = fscl_amd._surface_requests([(0, mid, 1000, 1000, [0.0])])
    req["n_la"] = 65
    assert L.fscl_amd_scan_surface(scan, tab, 81920, req.ctypes.data, 1, C.byref(res)) == -1
    with pytest.raises(ValueError):
        fscl_amd._surface_requests([(0, mid, 1000, 1000, [])])
    assert L.fscl_amd_scan_point_surfaces(scan, tab, 81920, -1, 1000, 1000, -20.0, 4.0, 33, C.byref(res)) == -1
    assert L.fscl_amd_scan_point_surfaces(scan, tab, 81920, 3, 1000, 0, -20.0, 4.0, 33, C.byref(res)) == -1
    assert L.fscl_amd_scan_point_surfaces(scan, tab, 81920, 3, -1, 1000, -20.0, 4.0, 33, C.byref(res)) == -1


# ------------------------------------------------------------------ the writer
def test_output_bytes(scan, tmp_path):
    name = scan.contents.chr_limits[0].name.decode()
    hdr = np.zeros(1, dtype=fscl_amd.SURFACE_DTYPE)[0]
    hdr["chr"], hdr["centre_pos"], hdr["n_la"], hdr["n_pos"], hdr["point"] = 0, 3000, 3, 2, 0
    hdr["la"][:3] = [math.log(1e-4), math.log(2e-3), 0.0]
    pts = np.zeros(2, dtype=fscl_amd._POINT_RAW)
    pts["sweep_pos"], pts["null_logl"] = [2500, 3001], [-10.0, -20.0]
    sf = fscl_amd.Surface(hdr, pts, np.array([[-10.0, -9.0, -8.5], [-15.0, -14.75, NAN]]))
    fscl_amd.surface_output(tmp_path / "s.txt", scan, [sf], 1.0, "L")
    want = "".join(f"L\t{name}\t3000\t{r}\n" for r in (
        "2500\t1.000e-04\t0.00\t-", "2500\t2.000e-03\t2.00\t-", "2500\t1.000e+00\t3.00\t-",
        "3001\t1.000e-04\t10.00\t+", "3001\t2.000e-03\t10.50\t*", "3001\t1.000e+00\tnan\t-",
        "summary\t2\t3\t3001\t2.000e-03\t10.50\t3001\t3001\t0\t1\t1.000e-04\t2.000e-03\t1\t0\t2"))
    assert (tmp_path / "s.txt").read_text().replace("-nan", "nan") == want
    sf2 = fscl_amd.Surface(hdr, pts, np.full((2, 3), NAN))
    fscl_amd.surface_output(tmp_path / "n.txt", scan, [sf, sf2], 1.0)
    lines = (tmp_path / "n.txt").read_text().splitlines()
    assert len(lines) == 14 and lines[6] == want.splitlines()[6][2:]
    assert lines[13] == f"{name}\t3000\tsummary\t2\t3\tNA\tNA\tNA\tNA\tNA\t0\t0\tNA\tNA\t0\t0\t0"
    with pytest.raises(ValueError):
        fscl_amd.surface_output(tmp_path / "x.txt", scan, [sf], -1.0)
    with pytest.raises(ValueError):
        fscl_amd.surface_output(tmp_path / "no-such-directory" / "x.txt", scan, [sf], 1.0)
    fscl_amd.surface_output(tmp_path / "e.txt", scan, [], 2.0)
    assert (tmp_path / "e.txt").read_bytes() == b""


def test_host_check_under_sanitizers(built, tmp_path):
    """tools/surface_host_check.c: the alpha list, the positions, the region and the writer under ASan and
    UBSan, as a stand-alone program (no device library, nothing loaded into Python)."""
    run_host_check("surface_host_check", ["surface.c", "util.c"], tmp_path, [tmp_path])


# ------------------------------------------------------------------ the CLI's refusals
@pytest.mark.parametrize("args, msg", [
    (["--no-scan"], "--surface-file needs the scan"),
    (["--surface-top=-1"], "--surface-top must be >= 0"),
    (["--surface-halfwidth=-5"], "--surface-halfwidth must be >= 0"),
    (["--surface-step=0"], "--surface-step must be at least 1"),
    (["--surface-drop=-0.5"], "--surface-drop must be >= 0"),
    (["--surface-alphas=-20:4:64"], "--surface-alphas must be LO:HI:N"),
    (["--surface-alphas=-21:4:10"], "--surface-alphas must be LO:HI:N"),
    (["--surface-alphas=0:5:10"], "--surface-alphas must be LO:HI:N"),
    (["--surface-alphas=2:1:10"], "--surface-alphas must be LO:HI:N"),
    (["--surface-alphas=1:1:2"], "--surface-alphas must be LO:HI:N"),
    (["--surface-alphas=-20:4"], "--surface-alphas must be LO:HI:N"),
    (["--surface-alphas=-20:4:10x"], "--surface-alphas must be LO:HI:N"),
    (["--surface-alphas=a:b:c"], "--surface-alphas must be LO:HI:N"),
])
def test_cli_refusals(built, tmp_path, args, msg):
    """Refused before the data is loaded: no device is touched and no file is written."""
    r = run_cli([f"--surface-file={tmp_path / 's.txt'}"] + args, tmp_path, snp="g1.snp")
    assert r.returncode != 0 and msg in r.stderr + r.stdout, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "s.txt").exists() and not (tmp_path / "o.txt").exists()


def test_run_keyword_refusals(built):
    for kw in (dict(surface_top=-1), dict(surface_step=0), dict(surface_halfwidth=-1), dict(surface_drop=-1.0),
               dict(surface_alphas=(-20.0, 4.0, 64)), dict(surface_alphas=(-21.0, 4.0, 5))):
        with pytest.raises(ValueError):
            fscl_amd.run(GOLD / "g1.snp", None, surface_file="unused.txt", **kw)
