"""Measure the grid-maximum mode on one GPU (HISTORY.md, "grid-maximum permutation test").

    python tools/grid_measure.py [--config C2] [--repeats 5] [-g 1000] [--n-permute 100]

On the bench genome of the config (bench.py's: seed 1, two sweeps per chromosome), in one process:
  * `repeats` all-cells launches of the cell-maximum kernel (scan_chromosome_grid, one launch
    over every cell) and `repeats` profiles of the same grid (scan_profile), alternating; each
    one's own kernel time (HIP events: cellmax_last_ms, profile_last_ms);
  * the whole grid job (scan_chromosome_grid + scan_permute_grid, n_permute trials): wall time,
    trials run, grid-point evaluations; and the default mode's job beside it.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import fscl_amd  # noqa: E402
from fscl_amd import synth  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("-g", "--small-grid-sp", type=int, default=1000)
    ap.add_argument("-G", "--large-grid-sp", type=int, default=100000)
    ap.add_argument("--n-permute", type=int, default=None)
    a = ap.parse_args()
    cfg = dict(synth.CONFIGS[a.config])
    n_perm = cfg.pop("n_permute")
    if a.n_permute is not None:
        n_perm = a.n_permute
    snp = Path(tempfile.mkdtemp(prefix="fscl_grid_")) / f"{a.config}.snp"
    synth.write_snp_file(str(snp), synth.generate(seed=55 if a.config == "C5" else 1, sweeps_per_chr=2, **cfg))
    fscl_amd.set_device(0)
    fscl_amd.get_lib().configure_logmsg(1)
    fscl_amd.init_log_table()
    scan = fscl_amd.load_snp_input(snp)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp)
    fscl_amd.compute_snp_null_model(scan, fsp)
    g, G = a.small_grid_sp, a.large_grid_sp
    fscl_amd.scan_chromosome_grid(scan, tab, small_grid_sp=g, large_grid_sp=G)  # warm-up: uploads, LDS plan
    n_cells = scan.contents.n_scan_pts
    cm, pr = [], []
    n_pts = 0
    for _ in range(a.repeats):
        fscl_amd.scan_chromosome_grid(scan, tab, small_grid_sp=g, large_grid_sp=G)
        cm.append(fscl_amd.cellmax_last_ms())
        n_pts = len(fscl_amd.scan_profile(scan, tab, small_grid_sp=g, large_grid_sp=G))
        pr.append(fscl_amd.profile_last_ms())
    out = {"config": a.config, "g": g, "G": G, "cells": n_cells, "profile_points": n_pts,
           "cellmax_kernel_ms": cm, "profile_kernel_ms": pr}
    jobs = {}
    for mode in ("grid", "bisection", "grid", "bisection"):
        fscl_amd.reset_stats()
        fscl_amd.srand()
        fscl_amd.set_permute_mode("parity")
        t0 = time.time()
        if mode == "grid":
            fscl_amd.scan_chromosome_grid(scan, tab, small_grid_sp=g, large_grid_sp=G)
            fscl_amd.scan_permute_grid(scan, tab, n_perm, small_grid_sp=g, large_grid_sp=G)
        else:
            fscl_amd.scan_chromosome(scan, tab, large_grid_sp=G)
            fscl_amd.scan_permute(scan, tab, n_perm, large_grid_sp=G)
        wall = time.time() - t0
        st = fscl_amd.get_stats()
        pts = fscl_amd.points(scan)
        jobs.setdefault(mode, []).append({
            "wall_s": wall, "trials": st["trials"], "gp_evals": st["gp_evals"], "kernel_ms": st["kernel_ms"],
            "n_maxalpha": st["n_maxalpha"], "sum_permute_n": int(pts["permute_n"].sum()),
            "finished": int(pts["permute_finished"].sum())})
    out["n_permute"] = n_perm
    out["jobs"] = jobs
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
