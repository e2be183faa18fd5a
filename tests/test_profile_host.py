"""Host side of the fine-grid CLR profile (no GPU): the grid, the cell assignment, the cell
maxima, the output rows and the command line's checks."""
from __future__ import annotations

import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from util import CLI
import fscl_amd
from fscl_amd import synth


def py_grid(limits, g, G):
    """(chr, pos, cell) of every grid point: per chromosome from the first cell's start in steps
    of g to the last cell's clipped end, the end appended once when the step misses it; a
    boundary shared by two cells belongs to the lower one."""
    out, cell0 = [], 0
    for c, (start, end) in enumerate(limits):
        if start >= end:
            continue
        n_cells = -(-(end - start) // G)
        pos = list(range(start, end + 1, g))
        if pos[-1] != end:
            pos.append(end)
        for p in pos:
            out.append((c, p, cell0 + (0 if p == start else min((p - start - 1) // G, n_cells - 1))))
        cell0 += n_cells
    return out


@pytest.fixture(scope="module")
def scan4(built, tmp_path_factory):
    """Four chromosomes whose limits are then set by hand: a non-zero start, a clipped last
    cell, a length that is a multiple of g, a length shorter than g."""
    snp = tmp_path_factory.mktemp("host") / "h.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=4, chr_len=100_000, snps_per_chr=40, n=12, seed=7))
    fscl_amd.get_lib().configure_logmsg(1)
    scan = fscl_amd.load_snp_input(snp)
    limits = [(12_345, 250_000), (0, 130_500), (0, 60_000), (0, 700)]
    for c, (a, e) in enumerate(limits):
        scan.contents.chr_limits[c].start_pos = a
        scan.contents.chr_limits[c].bp_length = e
    return scan, limits


@pytest.mark.parametrize("g,G", [(1000, 20_000), (500, 50_000), (20_000, 20_000), (7, 700)])
def test_grid_matches_restatement(scan4, g, G):
    scan, limits = scan4
    ch, pos, cell = fscl_amd.profile_grid(scan, g, G)
    assert list(zip(ch.tolist(), pos.tolist(), cell.tolist())) == py_grid(limits, g, G)


def test_shared_boundaries_belong_to_the_lower_cell(scan4):
    scan, limits = scan4
    ch, pos, cell = fscl_amd.profile_grid(scan, 1000, 20_000)
    at = {(c, p): k for c, p, k in zip(ch.tolist(), pos.tolist(), cell.tolist())}
    assert at[(0, 12_345)] == 0 and at[(0, 32_345)] == 0 and at[(0, 33_345)] == 1 and at[(0, 52_345)] == 1
    assert at[(0, 250_000)] == 11  # the clipped last cell's end, appended
    assert at[(1, 0)] == 12 and at[(1, 20_000)] == 12 and at[(1, 130_500)] == 18
    assert at[(2, 60_000)] == 21 and at[(3, 0)] == 22 and at[(3, 700)] == 22
    with pytest.raises(ValueError):
        fscl_amd.profile_grid(scan, 3000, 20_000)
    with pytest.raises(ValueError):
        fscl_amd.profile_grid(scan, 0, 20_000)


def hand_profile(clrs, cells, chrs=None):
    pf = np.zeros(len(clrs), dtype=fscl_amd.PROFILE_DTYPE)
    pf["clr"] = clrs
    pf["cell"] = cells
    pf["chr"] = chrs if chrs is not None else 0
    pf["grid_pos"] = np.arange(len(clrs)) * 10
    pf["sweep_pos"] = pf["grid_pos"] + 1
    return pf


def hand_scan(clrs):
    pts = (fscl_amd.ScanPtT * len(clrs))()
    for i, v in enumerate(clrs):
        pts[i].clr = v
    s = fscl_amd.ScanT()
    s.n_scan_pts = len(clrs)
    s.scan_pts = C.cast(pts, C.POINTER(fscl_amd.ScanPtT))
    return C.pointer(s), pts


def test_cell_max_ties_single_points_and_no_scan(built):
    # cell 0: points 0-3 (a tie of 5.0: the first wins); cell 1: its own points 4-5 and the
    # boundary point 3 it shares with cell 0, which is its maximum; cell 2 (another chromosome):
    # one point, no shared boundary
    pf = hand_profile([1.0, 5.0, 5.0, 4.0, 3.0, 2.0, 9.0], [0, 0, 0, 0, 1, 1, 2], [0, 0, 0, 0, 0, 0, 1])
    scan, keep = hand_scan([5.0, 3.5, 9.5])
    got, missed = fscl_amd.profile_cell_max(pf, scan)
    assert got["sweep_pos"].tolist() == [11, 31, 61] and got["clr"].tolist() == [5.0, 4.0, 9.0]
    assert missed == 1  # cell 1: 4.0 > 3.5; an equal CLR (cell 0) is not a miss
    empty, _ = hand_scan([])
    with pytest.raises(ValueError):
        fscl_amd.profile_cell_max(pf, empty)


def test_profile_output_rows(scan4, tmp):
    scan, _ = scan4
    s = scan.contents
    pf = hand_profile([12.345, 0.0], [0, 0], [0, 1])
    pf["lalpha"] = [math.log(1e-4), 4.0]
    pf["n_snps"] = [40, 40]
    pf["window_start"] = [0, 40]
    pf["window_end"] = [39, 79]
    for label in (None, "run7"):
        fscl_amd.profile_output(tmp / "p.txt", scan, pf, label)
        want = "".join(("" if label is None else label + "\t") + "%s\t%d\t%1.2f\t%1.3e\t%d\t%d\t%d\n" % (
            s.chr_limits[int(p["chr"])].name.decode(), p["sweep_pos"], p["clr"], math.exp(p["lalpha"]), p["n_snps"],
            s.snps[int(p["window_start"])].pos, s.snps[int(p["window_end"])].pos) for p in pf)
        assert (tmp / "p.txt").read_text() == want


def test_cli_rejects_profile_without_scan_and_bad_spacing(built, tmp):
    snp = tmp / "c.snp"
    synth.write_snp_file(str(snp), synth.generate(n_chr=1, chr_len=100_000, snps_per_chr=40, n=12, seed=8))
    base = [str(CLI), "-f", str(snp), "-o", str(tmp / "o.txt")]
    r = subprocess.run(base + ["--no-scan", f"--profile-file={tmp / 'p.txt'}"], capture_output=True, text=True)
    assert r.returncode != 0 and "--profile-file" in r.stderr + r.stdout
    r = subprocess.run(base + ["--no-scan", "-g", "3000", "-G", "100000"], capture_output=True, text=True)
    assert r.returncode != 0 and "evenly divide" in r.stderr + r.stdout
    # with --output-bs the spacing is checked only for the profile's sake
    bs = ["--no-scan", f"--output-bs={tmp / 'bs.txt'}", "-g", "3000", "-G", "100000"]
    r = subprocess.run(base + bs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(base + bs + [f"--profile-file={tmp / 'p.txt'}"], capture_output=True, text=True)
    assert r.returncode != 0 and "evenly divide" in r.stderr + r.stdout
    assert not (tmp / "p.txt").exists()


def test_fsclg_profile_rejects_points_without_an_output(built):
    """The synchronous entry checks `out` before it submits anything (no context needed)."""
    L = fscl_amd.get_lib()
    L.fsclg_profile.restype = C.c_int
    L.fsclg_profile.argtypes = [C.c_void_p, C.POINTER(fscl_amd.RunT), C.c_int, C.c_int, C.c_void_p]
    runs = (fscl_amd.RunT * 1)(fscl_amd.RunT(0, 100, 10, 5))
    assert L.fsclg_profile(None, runs, 1, 100, None) == -1  # FSCLG_E_ARG
    assert L.fsclg_profile(None, runs, 1, 100, C.c_void_p(8)) == -1  # (no context: the submit's own check)
