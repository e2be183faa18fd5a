"""fscl_amd -- MI355X-native drop-in for slowkoni/fscl's CLR sweep scan and
block-permutation test.

The product is the C-ABI library ``fscl_amd/_build/libfscl_amd.so`` (host C +
gfx950 HIP kernels, see include/fscl_amd.h and include/fsclg.h) and the
``fscl_amd/_build/fscl`` command line.  This module is the Python mirror of the
reference's entry points (fscl.h:86-128) over ctypes: same names, same argument
meaning, same fatal-error behaviour (the library prints and exits, as
logmsg(MSG_FATAL) does in the reference).

There is no CPU fallback: importing works without a GPU (so the library's
exports can be inspected), but every scan entry point needs the HIP device and
fails loudly without it.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from pathlib import Path

import numpy as np

__all__ = [
    "lib", "LIB_PATH", "CLI_PATH", "SnpT", "ScanPtT", "ScanT", "ChrLimitsT", "SplineT", "SmPtableT", "Stats",
    "load_snp_input", "load_ms_input", "background_fsp", "compute_sweep_model_tables", "compute_snp_null_model",
    "init_log_table", "scan_chromosome", "scan_permute", "scan_output", "output_background_fs", "points",
    "get_stats", "reset_stats", "set_device", "set_devices", "set_ranks", "set_ranks_shm", "srand", "shutdown", "run",
    "device_count", "set_dump_output", "ProfileT", "RunT", "PointT", "scan_profile", "profile_cell_max", "profile_grid",
    "profile_runs", "profile_output", "profile_last_ms", "profile_chunk",
    "scan_chromosome_grid", "scan_permute_grid", "cellmax_runs", "cellmax_last_ms", "site_rows",
    "scan_curves", "scan_point_curves", "curve_runs", "curve_support", "curve_output", "curve_last_ms",
    "curve_forced", "CURVE_DTYPE",
    "scan_sites", "scan_point_sites", "sites_summary", "sites_output", "sites_last_ms", "sites_cap", "SitesT",
    "SITES_DTYPE", "SITE_REQ_DTYPE", "SITES_SUMMARY_DTYPE",
    "scan_expect", "scan_point_expect", "expect_output", "expect_last_ms", "expect_runs", "ExpectT", "EXPECT_DTYPE",
    "EXPECT_SITE_DTYPE",
    "simulate", "simulate_scan", "simulate_output", "simulate_last_ms", "scan_free", "bootstrap", "bootstrap_output",
    "bootstrap_times", "parse_sweep", "nearest_sweep", "SWEEP_DTYPE", "BOOT_DTYPE",
    "tail_fit", "tail_runs", "tail_output", "tail_last_ms", "tail_summary", "tail_records", "TAIL_DTYPE", "TAIL_FLAGS",
    "familywise", "familywise_runs", "familywise_combine", "familywise_output", "familywise_null_output",
    "familywise_last_ms", "familywise_order", "familywise_threshold", "familywise_chunk", "FamilywiseT",
    "MAXT_WG", "MAXT_TILE", "MAXT_MAX_GROUPS",
]

ROOT = Path(__file__).resolve().parent
LIB_PATH = (Path(os.environ["FSCL_AMD_LIBDIR"]) if os.environ.get("FSCL_AMD_LIBDIR") else
            ROOT / ("_build_trace" if os.environ.get("FSCL_AMD_TRACE") else "_build")) / "libfscl_amd.so"
CLI_PATH = ROOT / "_build" / "fscl"


class SnpT(C.Structure):  # fscl.h:7-14
    _fields_ = [("chr", C.c_int), ("pos", C.c_int), ("null_logl", C.c_double), ("obs_freq", C.c_int),
                ("depth_p", C.c_int), ("folded", C.c_int)]


class ChrLimitsT(C.Structure):  # fscl.h:26-33
    _fields_ = [("chr", C.c_int), ("name", C.c_char_p), ("start_index", C.c_int), ("n_snps", C.c_int),
                ("start_pos", C.c_int), ("bp_length", C.c_int)]


class ScanPtT(C.Structure):  # fscl.h:35-51
    _fields_ = [("chr", C.c_int), ("nearest_snp", C.c_int), ("sweep_pos", C.c_int), ("n_snps", C.c_int),
                ("window_start", C.c_int), ("window_end", C.c_int), ("lalpha", C.c_double),
                ("null_logl", C.c_double), ("sm_logl", C.c_double), ("clr", C.c_double),
                ("permute_n", C.c_int), ("permute_p", C.c_int), ("permute_finished", C.c_int),
                ("scan_running", C.c_int), ("permute_clr", C.POINTER(C.c_float))]


class ScanT(C.Structure):  # fscl.h:53-62
    _fields_ = [("n_snps", C.c_int), ("snps", C.POINTER(SnpT)), ("n_depths", C.c_int),
                ("sample_depths", C.POINTER(C.c_int)), ("n_scan_pts", C.c_int),
                ("scan_pts", C.POINTER(ScanPtT)), ("chr_limits", C.POINTER(ChrLimitsT)),
                ("n_chromosomes", C.c_int)]


class SplineT(C.Structure):  # fscl.h:64-68
    _fields_ = [("n", C.c_int), ("knot_points", C.POINTER(C.c_double)),
                ("coef", C.POINTER(C.POINTER(C.c_double)))]


class SmPtableT(C.Structure):  # fscl.h:70-76
    _fields_ = [("spline_func", C.POINTER(C.POINTER(SplineT))), ("fspline_func", C.POINTER(C.POINTER(SplineT))),
                ("sample_size", C.c_int), ("pbk", C.POINTER(C.POINTER(C.c_double))),
                ("fsp", C.POINTER(C.c_double))]


class Stats(C.Structure):  # fscl_amd_stats_t
    _fields_ = [("scan_s", C.c_double), ("permute_s", C.c_double), ("host_perm_s", C.c_double),
                ("kernel_ms", C.c_double), ("gp_evals", C.c_ulonglong), ("n_terms", C.c_ulonglong),
                ("n_null", C.c_ulonglong), ("n_walks", C.c_ulonglong), ("n_maxalpha", C.c_ulonglong),
                ("n_unsafe", C.c_ulonglong), ("n_slow", C.c_ulonglong), ("n_ties", C.c_ulonglong),
                ("n_launches", C.c_ulonglong), ("negj", C.c_ulonglong), ("trials", C.c_int),
                ("cache_iv0", C.c_int), ("cache_n_iv", C.c_int), ("cache_n_rows", C.c_int),
                ("cache_cover", C.c_double), ("window_ms", C.c_double), ("host_null_s", C.c_double),
                ("host_upload_s", C.c_double), ("search_s", C.c_double), ("prune_s", C.c_double),
                ("n_dup_cells", C.c_ulonglong), ("n_ep_saved", C.c_ulonglong), ("busy_ms", C.c_double),
                ("wait_s", C.c_double), ("n_crit", C.c_ulonglong), ("n_drain", C.c_ulonglong),
                ("n_devices", C.c_int), ("spec_threads", C.c_int), ("spec_posted", C.c_ulonglong),
                ("spec_hits", C.c_ulonglong), ("spec_cands", C.c_ulonglong), ("spec_wait_s", C.c_double),
                ("spec_done", C.c_ulonglong), ("spec_gen_s", C.c_double),
                ("n_split_retry", C.c_ulonglong), ("spec_claimed", C.c_ulonglong), ("n_merged", C.c_ulonglong),
                ("perm_leader", C.c_int), ("plan_mode", C.c_int), ("plan_fallback", C.c_ulonglong),
                ("spec_rank", C.c_ulonglong * 8), ("prestaged", C.c_ulonglong), ("prestage_hits", C.c_ulonglong)]

    def as_dict(self) -> dict:
        return {k: (list(v) if isinstance(v, C.Array) else v) for k, v in ((k, getattr(self, k)) for k, _ in self._fields_)}


class ProfileT(C.Structure):  # fscl_amd_profile_t
    _fields_ = [("n_pts", C.c_int), ("pts", C.POINTER(ScanPtT)), ("grid_pos", C.POINTER(C.c_int)),
                ("cell", C.POINTER(C.c_int))]


class RunT(C.Structure):  # fsclg_run_t
    _fields_ = [("chr", C.c_int32), ("start_pos", C.c_int32), ("step", C.c_int32), ("count", C.c_int32)]


class ExpectT(C.Structure):  # fscl_amd_expect_t
    _fields_ = [("n", C.c_int), ("n_tasks", C.c_int), ("n_bins", C.c_int), ("req", C.c_void_p), ("first", C.c_void_p),
                ("own", C.c_void_p), ("la", C.c_void_p), ("hdr", C.c_void_p), ("tot", C.c_void_p), ("point", C.c_void_p),
                ("kernel_ms", C.c_double)]


class SitesT(C.Structure):  # fscl_amd_sites_t
    _fields_ = [("n", C.c_int), ("point", C.POINTER(C.c_int)), ("hdr", C.c_void_p), ("terms", C.POINTER(C.c_double)),
                ("n_terms", C.c_size_t)]


class TailT(C.Structure):  # fscl_amd_tail_t
    _fields_ = [("n", C.c_int), ("df", C.c_int), ("min_n", C.c_int), ("pt", C.c_void_p), ("n_fit", C.c_int),
                ("n_central", C.c_int), ("n_nofit", C.c_int), ("n_calibration", C.c_int), ("calibration", C.c_double),
                ("kernel_ms", C.c_double), ("wall_s", C.c_double)]


class FamilywiseT(C.Structure):  # fscl_amd_familywise_t
    _fields_ = [("n", C.c_int), ("n_groups", C.c_int), ("trials", C.c_int), ("seed", C.c_ulonglong),
                ("order", C.POINTER(C.c_int32)), ("c_single", C.POINTER(C.c_int32)), ("c_chr", C.POINTER(C.c_int32)),
                ("c_step", C.POINTER(C.c_int32)), ("gmax", C.POINTER(C.c_double)), ("garg", C.POINTER(C.c_int32)),
                ("chr_max", C.POINTER(C.c_double)), ("chr_arg", C.POINTER(C.c_int32)), ("matrix", C.POINTER(C.c_double)),
                ("kernel_ms", C.c_double), ("wall_s", C.c_double)]


class SurfacesT(C.Structure):  # fscl_amd_surfaces_t
    _fields_ = [("n", C.c_int), ("hdr", C.c_void_p), ("pts", C.c_void_p), ("sm", C.c_void_p), ("n_pos", C.c_size_t),
                ("n_cells", C.c_size_t), ("n_terms", C.c_ulonglong)]


class ConditionalT(C.Structure):  # fscl_amd_conditional_t
    _fields_ = [("n_blocks", C.c_int), ("blk", C.c_void_p), ("rows", C.c_void_p), ("given", C.c_void_p),
                ("n_rows", C.c_size_t), ("n_given", C.c_size_t), ("n_terms", C.c_ulonglong), ("fold_s", C.c_double)]


class BlocksT(C.Structure):  # fscl_amd_blocks_t
    _fields_ = [("n", C.c_int), ("hdr", C.c_void_p), ("pts", C.c_void_p), ("bs", C.c_void_p), ("cnt", C.c_void_p),
                ("n_pos", C.c_size_t), ("n_cells", C.c_size_t), ("n_terms", C.c_ulonglong)]


class PointT(C.Structure):  # fsclg_point_t
    _fields_ = [("chr", C.c_int32), ("nearest_snp", C.c_int32), ("sweep_pos", C.c_int32), ("n_snps", C.c_int32),
                ("window_start", C.c_int32), ("window_end", C.c_int32), ("flags", C.c_int32), ("cost", C.c_uint32),
                ("lalpha", C.c_double), ("null_logl", C.c_double), ("sm_logl", C.c_double), ("clr", C.c_double)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_longlong), C.c_int, C.c_void_p)
TOP_ACCEPT_FN = C.CFUNCTYPE(C.c_int, C.POINTER(ScanPtT))

# exported symbols of include/fscl_amd.h and include/fsclg.h (checked by tests)
EXPORTS = [
    "load_snp_input", "background_fsp", "output_background_fs", "lchoose", "compute_sweep_model_tables",
    "spline_interpolate", "init_log_table", "search_maxalpha", "compute_snp_null_model", "scan_chromosome",
    "scan_permute", "scan_output", "ascbias_adjust_background", "ascbias_adjust_expect", "configure_logmsg",
    "logmsg", "cr_logmsg", "fscl_amd_load_ms_input", "fscl_amd_set_device", "fscl_amd_set_ranks",
    "fscl_amd_get_stats", "fscl_amd_reset_stats", "fscl_amd_shutdown", "fscl_amd_partition",
    "fscl_amd_set_devices", "fscl_amd_n_devices", "fscl_amd_set_ranks_shm", "fscl_amd_srand",
    "fscl_amd_set_dump_output", "fsclg_host_alloc", "fsclg_host_free", "fsclg_slot_wait",
    "fsclg_slot_set_rows_host", "fsclg_slot_set_rows_packed",
    "fsclg_open", "fsclg_close", "fsclg_last_error", "fsclg_device_count", "fsclg_upload_tables",
    "fsclg_upload_snps", "fsclg_set_rows", "fsclg_set_chr_null", "fsclg_set_alpha_grid", "fsclg_search_maxpos",
    "fsclg_search_points", "fsclg_get_stats", "fsclg_reset_stats", "fsclg_interval_thresholds",
    "fsclg_row_buffer", "fsclg_slot_row_buffer", "fsclg_slot_set_rows", "fsclg_search_submit", "fsclg_search_wait",
    "fsclg_slot_windows", "ms_openfile", "ms_background", "ms_next_block",
    "fscl_amd_set_permute_mode",
    "fsclg_profile", "fsclg_profile_submit", "fsclg_profile_wait", "fsclg_profile_chunk", "fsclg_profile_last_ms",
    "fscl_amd_scan_profile", "fscl_amd_profile_cell_max", "fscl_amd_profile_output", "fscl_amd_profile_free",
    "fscl_amd_profile_grid", "fscl_amd_profile_runs", "fscl_amd_profile_last_ms",
    "fsclg_cellmax_submit", "fsclg_cellmax_wait", "fsclg_cellmax_last_ms",
    "fscl_amd_scan_chromosome_grid", "fscl_amd_scan_permute_grid", "fscl_amd_cellmax_runs",
    "fscl_amd_cellmax_last_ms", "fscl_amd_site_rows",
    "fsclg_curve_submit", "fsclg_curve_wait", "fsclg_curve_last_ms", "fsclg_curve_forced",
    "fscl_amd_scan_curves", "fscl_amd_scan_point_curves", "fscl_amd_curve_support", "fscl_amd_curve_output",
    "fscl_amd_curve_runs", "fscl_amd_curve_last_ms", "fscl_amd_curve_forced",
    "fsclg_sites_submit", "fsclg_sites_wait", "fsclg_sites_last_ms", "fsclg_sites_cap",
    "fscl_amd_scan_sites", "fscl_amd_scan_point_sites", "fscl_amd_sites_free", "fscl_amd_sites_summary",
    "fscl_amd_sites_output", "fscl_amd_sites_last_ms",
    "fsclg_sample_tables", "fsclg_sample_submit", "fsclg_sample_wait", "fsclg_sample_last_ms",
    "fscl_amd_simulate", "fscl_amd_simulate_scan", "fscl_amd_scan_free", "fscl_amd_simulate_output",
    "fscl_amd_simulate_last_ms", "fscl_amd_bootstrap", "fscl_amd_bootstrap_times", "fscl_amd_bootstrap_output",
    "fscl_amd_parse_sweep", "fscl_amd_nearest_sweep", "fscl_amd_sample_tables_build",
    "fsclg_tail_submit", "fsclg_tail_wait", "fsclg_tail_last_ms",
    "fscl_amd_tail_fit", "fscl_amd_tail_runs", "fscl_amd_tail_last_ms", "fscl_amd_tail_free", "fscl_amd_tail_count",
    "fscl_amd_tail_chunk", "fscl_amd_tail_pack", "fscl_amd_tail_log10p", "fscl_amd_tail_summary", "fscl_amd_tail_output",
    "fsclg_surface_submit", "fsclg_surface_wait", "fsclg_surface_last_ms",
    "fscl_amd_surface_alphas", "fscl_amd_surface_run", "fscl_amd_scan_surface", "fscl_amd_scan_point_surfaces",
    "fscl_amd_top_points", "fscl_amd_surfaces_free", "fscl_amd_surface_region", "fscl_amd_surface_output", "fscl_amd_surface_runs",
    "fscl_amd_surface_last_ms",
    "fsclg_blocks_submit", "fsclg_blocks_wait", "fsclg_blocks_last_ms",
    "fscl_amd_scan_blocks", "fscl_amd_scan_point_jackknife", "fscl_amd_blocks_free", "fscl_amd_blocks_cap",
    "fscl_amd_blocks_bound", "fscl_amd_jackknife_combine", "fscl_amd_jackknife_output", "fscl_amd_blocks_runs",
    "fscl_amd_blocks_last_ms",
    "fsclg_cond_submit", "fsclg_cond_wait", "fsclg_cond_last_ms",
    "fscl_amd_cond_clip", "fscl_amd_cond_given_terms", "fscl_amd_cond_base", "fscl_amd_conditional_cap",
    "fscl_amd_conditional_error", "fscl_amd_conditional_check", "fscl_amd_scan_conditional", "fscl_amd_conditional_output", "fscl_amd_conditional_free",
    "fscl_amd_conditional_last_ms", "fscl_amd_cond_runs",
    "fsclg_expect_tables", "fsclg_expect_submit", "fsclg_expect_count", "fsclg_expect_wait", "fsclg_expect_last_ms",
    "fscl_amd_scan_expect", "fscl_amd_scan_point_expect", "fscl_amd_expect_runs", "fscl_amd_expect_check",
    "fscl_amd_expect_error", "fscl_amd_expect_cap", "fscl_amd_expect_bin", "fscl_amd_expect_tables_build",
    "fscl_amd_expect_output", "fscl_amd_expect_free", "fscl_amd_expect_last_ms",
    "fsclg_maxt_submit", "fsclg_maxt_wait", "fsclg_maxt_last_ms",
    "fscl_amd_familywise", "fscl_amd_familywise_runs", "fscl_amd_familywise_last_ms", "fscl_amd_familywise_error",
    "fscl_amd_familywise_cap", "fscl_amd_familywise_check", "fscl_amd_familywise_free", "fscl_amd_familywise_order",
    "fscl_amd_familywise_chunk", "fscl_amd_familywise_combine", "fscl_amd_familywise_threshold",
    "fscl_amd_familywise_output", "fscl_amd_familywise_null_output",
]


def _load() -> C.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(f"fscl_amd native library missing at {LIB_PATH}; run `python -m fscl_amd.build`")
    L = C.CDLL(str(LIB_PATH))
    P = C.POINTER
    sigs = {
        "load_snp_input": (P(ScanT), [C.c_char_p, C.c_int, C.c_int]),
        "fscl_amd_load_ms_input": (P(ScanT), [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]),
        "ms_openfile": (None, [C.c_char_p]),
        "fscl_amd_set_permute_mode": (C.c_int, [C.c_int, C.c_ulonglong]),
        "ms_background": (P(ScanT), [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]),
        "ms_next_block": (P(ScanT), [C.c_int, C.c_int, C.c_int, C.c_int]),
        "background_fsp": (P(P(C.c_double)), [P(ScanT), C.c_int, C.c_char_p, C.c_int]),
        "output_background_fs": (None, [C.c_char_p, P(ScanT), P(P(C.c_double))]),
        "lchoose": (C.c_double, [C.c_int, C.c_int]),
        "compute_sweep_model_tables": (P(SmPtableT), [P(ScanT), P(P(C.c_double)), C.c_int, C.c_int, C.c_int,
                                                      C.c_int]),
        "spline_interpolate": (C.c_double, [P(SplineT), C.c_double]),
        "init_log_table": (None, []),
        "search_maxalpha": (None, [P(ScanPtT), P(SnpT), P(SmPtableT)]),
        "compute_snp_null_model": (None, [P(ScanT), P(P(C.c_double))]),
        "scan_chromosome": (None, [P(ScanT), P(SmPtableT), C.c_int, C.c_int, C.c_int, C.c_int]),
        "scan_permute": (None, [P(ScanT), P(SmPtableT), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_double]),
        "scan_output": (None, [C.c_char_p, P(ScanT), C.c_int, C.c_int, C.c_char_p]),
        "ascbias_adjust_background": (P(C.c_double), [P(C.c_double), C.c_int, C.c_int, C.c_int]),
        "ascbias_adjust_expect": (None, [P(C.c_double), C.c_int, C.c_int, C.c_int]),
        "configure_logmsg": (None, [C.c_int]),
        "fscl_amd_set_device": (C.c_int, [C.c_int]),
        "fscl_amd_set_devices": (C.c_int, [P(C.c_int), C.c_int]),
        "fscl_amd_n_devices": (C.c_int, []),
        "fscl_amd_set_ranks_shm": (C.c_int, [C.c_int, C.c_int, C.c_char_p]),
        "fscl_amd_srand": (None, [C.c_uint]),
        "fscl_amd_set_dump_output": (None, [C.c_char_p, C.c_char_p]),
        "fscl_amd_set_ranks": (C.c_int, [C.c_int, C.c_int, EXCHANGE_FN, C.c_void_p]),
        "fscl_amd_get_stats": (None, [P(Stats)]),
        "fscl_amd_partition": (None, [P(C.c_double), C.c_int, C.c_int, C.c_int, P(C.c_int), P(C.c_int)]),
        "fh_srand": (None, [C.c_void_p, C.c_uint]),
        "fh_rand": (C.c_int, [C.c_void_p]),
        "fscl_amd_reset_stats": (None, []),
        "fscl_amd_shutdown": (None, []),
        "fsclg_device_count": (C.c_int, []),
        "fsclg_last_error": (C.c_char_p, []),
        "fsclg_interval_thresholds": (C.c_int, [C.c_double, C.c_int, P(C.c_double)]),
        "fsclg_profile_chunk": (C.c_int, []),
        "fscl_amd_scan_profile": (P(ProfileT), [P(ScanT), P(SmPtableT), C.c_int, C.c_int, C.c_int]),
        "fscl_amd_profile_cell_max": (C.c_int, [P(ProfileT), P(ScanT), P(ScanPtT), P(C.c_int)]),
        "fscl_amd_profile_output": (None, [C.c_char_p, P(ScanT), P(ProfileT), C.c_char_p]),
        "fscl_amd_profile_free": (None, [P(ProfileT)]),
        "fscl_amd_profile_grid": (C.c_int, [P(ScanT), C.c_int, C.c_int, P(P(C.c_int)), P(P(C.c_int)), P(P(C.c_int))]),
        "fscl_amd_profile_runs": (C.c_int, [P(ScanT), P(SmPtableT), P(RunT), C.c_int, C.c_int, P(PointT)]),
        "fscl_amd_profile_last_ms": (C.c_double, []),
        "fscl_amd_scan_chromosome_grid": (None, [P(ScanT), P(SmPtableT), C.c_int, C.c_int, C.c_int]),
        "fscl_amd_scan_permute_grid": (None, [P(ScanT), P(SmPtableT), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                              C.c_double]),
        "fscl_amd_cellmax_runs": (C.c_int, [P(ScanT), P(SmPtableT), P(RunT), C.c_int, C.c_int, C.c_void_p, P(PointT)]),
        "fscl_amd_cellmax_last_ms": (C.c_double, []),
        "fscl_amd_site_rows": (C.c_int, [P(ScanT), P(SmPtableT), C.c_void_p]),
        "fscl_amd_scan_curves": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "fscl_amd_scan_point_curves": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_void_p]),
        "fscl_amd_curve_support": (C.c_int, [C.c_void_p, C.c_double, P(C.c_double), P(C.c_double), P(C.c_int),
                                             P(C.c_int)]),
        "fscl_amd_curve_output": (None, [C.c_char_p, P(ScanT), C.c_void_p, C.c_int, C.c_double, C.c_char_p]),
        "fscl_amd_curve_runs": (C.c_int, [P(ScanT), P(SmPtableT), P(RunT), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
        "fscl_amd_curve_last_ms": (C.c_double, []),
        "fscl_amd_curve_forced": (C.c_ulonglong, []),
        "fscl_amd_scan_sites": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_void_p, C.c_int, P(SitesT)]),
        "fscl_amd_scan_point_sites": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_int, P(SitesT)]),
        "fscl_amd_sites_free": (None, [P(SitesT)]),
        "fscl_amd_sites_summary": (None, [P(ScanT), P(SitesT), C.c_void_p]),
        "fscl_amd_sites_output": (None, [C.c_char_p, P(ScanT), P(SitesT), C.c_char_p]),
        "fscl_amd_sites_last_ms": (C.c_double, []),
        "fsclg_sites_cap": (C.c_size_t, []),
        "fscl_amd_parse_sweep": (C.c_int, [P(ScanT), C.c_char_p, C.c_void_p]),
        "fscl_amd_nearest_sweep": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
        "fscl_amd_simulate": (C.c_int, [P(ScanT), P(SmPtableT), C.c_void_p, C.c_int, C.c_ulonglong, C.c_int, C.c_void_p,
                                        P(C.c_ulonglong)]),
        "fscl_amd_simulate_scan": (P(ScanT), [P(ScanT), C.c_void_p]),
        "fscl_amd_scan_free": (None, [P(ScanT)]),
        "fscl_amd_simulate_output": (C.c_int, [C.c_char_p, P(ScanT)]),
        "fscl_amd_simulate_last_ms": (C.c_double, []),
        "fscl_amd_bootstrap": (C.c_int, [P(ScanT), P(SmPtableT), P(P(C.c_double)), C.c_void_p, C.c_int, C.c_int,
                                         C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
        "fscl_amd_bootstrap_times": (None, [P(C.c_double)]),
        "fscl_amd_bootstrap_output": (None, [C.c_char_p, P(ScanT), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p]),
        "fscl_amd_tail_fit": (C.c_int, [P(ScanT), C.c_int, C.c_int, P(TailT)]),
        "fscl_amd_tail_runs": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p]),
        "fscl_amd_tail_last_ms": (C.c_double, []),
        "fscl_amd_tail_free": (None, [P(TailT)]),
        "fscl_amd_tail_summary": (None, [P(ScanT), P(TailT)]),
        "fscl_amd_tail_output": (C.c_int, [C.c_char_p, P(ScanT), P(TailT), C.c_char_p]),
        "fscl_amd_surface_alphas": (C.c_int, [C.c_double, C.c_double, C.c_int, C.c_double, C.c_void_p]),
        "fscl_amd_surface_run": (C.c_int, [P(ScanT), C.c_void_p, P(RunT)]),
        "fscl_amd_top_points": (C.c_int, [P(ScanT), C.c_int, C.c_int, TOP_ACCEPT_FN, C.c_void_p]),
        "fscl_amd_scan_surface": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_void_p, C.c_int, P(SurfacesT)]),
        "fscl_amd_scan_point_surfaces": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                                   C.c_double, C.c_int, P(SurfacesT)]),
        "fscl_amd_surfaces_free": (None, [P(SurfacesT)]),
        "fscl_amd_surface_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
        "fscl_amd_surface_output": (C.c_int, [C.c_char_p, P(ScanT), P(SurfacesT), C.c_double, C.c_char_p]),
        "fscl_amd_surface_runs": (C.c_int, [P(ScanT), P(SmPtableT), P(RunT), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
        "fscl_amd_surface_last_ms": (C.c_double, []),
        "fscl_amd_scan_blocks": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_void_p, C.c_int, C.c_int, P(BlocksT)]),
        "fscl_amd_scan_point_jackknife": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                                    C.c_double, C.c_int, C.c_int, P(BlocksT)]),
        "fscl_amd_blocks_free": (None, [P(BlocksT)]),
        "fscl_amd_blocks_cap": (C.c_size_t, []),
        "fscl_amd_blocks_bound": (C.c_int, [P(ScanT), P(RunT), C.c_int, C.c_int, P(C.c_int), P(C.c_int)]),
        "fscl_amd_jackknife_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
        "fscl_amd_jackknife_output": (C.c_int, [C.c_char_p, P(ScanT), P(BlocksT), C.c_char_p]),
        "fscl_amd_blocks_runs": (C.c_int, [P(ScanT), P(SmPtableT), P(RunT), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
        "fscl_amd_blocks_last_ms": (C.c_double, []),
        "fscl_amd_cond_clip": (C.c_int, [P(ScanT), C.c_void_p, C.c_int, C.c_int, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int)]),
        "fscl_amd_cond_base": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_int)]),
        "fscl_amd_conditional_cap": (C.c_size_t, []),
        "fscl_amd_conditional_error": (C.c_char_p, []),
        "fscl_amd_scan_conditional": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_int, C.c_int, C.c_double, P(ConditionalT)]),
        "fscl_amd_conditional_output": (C.c_int, [C.c_char_p, P(ScanT), P(ConditionalT), C.c_char_p]),
        "fscl_amd_conditional_free": (None, [P(ConditionalT)]),
        "fscl_amd_conditional_last_ms": (C.c_double, []),
        "fscl_amd_cond_runs": (C.c_int, [P(ScanT), P(SmPtableT), P(RunT), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
        "fscl_amd_scan_expect": (C.c_int, [P(ScanT), P(SmPtableT), P(P(C.c_double)), C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_int, C.c_int, P(ExpectT)]),
        "fscl_amd_scan_point_expect": (C.c_int, [P(ScanT), P(SmPtableT), P(P(C.c_double)), C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_int, C.c_int, P(ExpectT)]),
        "fscl_amd_expect_runs": (C.c_int, [P(ScanT), P(SmPtableT), P(P(C.c_double)), C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, P(C.c_void_p), P(C.c_size_t)]),
        "fscl_amd_expect_check": (C.c_int, [P(ScanT), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
        "fscl_amd_expect_error": (C.c_char_p, []),
        "fscl_amd_expect_cap": (C.c_size_t, []),
        "fscl_amd_expect_bin": (C.c_int, [C.c_double, C.c_int]),
        "fscl_amd_expect_output": (C.c_int, [C.c_char_p, P(ScanT), P(ExpectT), C.c_char_p]),
        "fscl_amd_expect_free": (None, [P(ExpectT)]),
        "fscl_amd_expect_last_ms": (C.c_double, []),
        "fscl_amd_familywise": (C.c_int, [P(ScanT), P(SmPtableT), C.c_int, C.c_ulonglong, C.c_double, C.c_int, C.c_int, C.c_int,
                                          C.c_double, C.c_int, P(FamilywiseT)]),
        "fscl_amd_familywise_runs": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
        "fscl_amd_familywise_last_ms": (C.c_double, []),
        "fscl_amd_familywise_error": (C.c_char_p, []),
        "fscl_amd_familywise_cap": (C.c_size_t, []),
        "fscl_amd_familywise_check": (C.c_int, [P(ScanT), C.c_int, C.c_int]),
        "fscl_amd_familywise_free": (None, [P(FamilywiseT)]),
        "fscl_amd_familywise_order": (None, [C.c_void_p, C.c_int, C.c_void_p]),
        "fscl_amd_familywise_chunk": (C.c_int, [C.c_int, C.c_int, C.c_size_t]),
        "fscl_amd_familywise_combine": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
        "fscl_amd_familywise_threshold": (C.c_int, [C.c_void_p, C.c_int, C.c_double, P(C.c_double)]),
        "fscl_amd_familywise_output": (C.c_int, [C.c_char_p, P(ScanT), P(FamilywiseT), C.c_char_p]),
        "fscl_amd_familywise_null_output": (C.c_int, [C.c_char_p, P(ScanT), P(FamilywiseT), C.c_char_p]),
    }
    for name, (res, args) in sigs.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return L


_lib = None
_keep = []  # ctypes callbacks and buffers that must outlive their C users


def get_lib() -> C.CDLL:
    """The loaded native library (loaded on first use, so `python -m fscl_amd.build` works without it)."""
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def __getattr__(name):  # PEP 562: fscl_amd.lib
    if name == "lib":
        return get_lib()
    raise AttributeError(name)


def _b(s):
    return None if s is None else os.fsencode(str(s))


def device_count() -> int:
    return int(get_lib().fsclg_device_count())


def init_log_table() -> None:
    get_lib().init_log_table()


def load_snp_input(path, include_invariant: bool = False, minimum_depth: int = 5):
    return get_lib().load_snp_input(_b(path), int(include_invariant), max(5, int(minimum_depth)))


def load_ms_input(path, segment_length: int, folded: bool = False, sample_first: int = 0, sample_size: int = 0):
    return get_lib().fscl_amd_load_ms_input(_b(path), int(segment_length), int(folded), int(sample_first),
                                      int(sample_size))


def ms_blocks(path, segment_length: int, folded: bool = False, sample_first: int = 0, sample_size: int = 0):
    """The reference's block loop (fscl.c:296-313): ms_openfile, then one
    scan_t per ms_next_block until it returns NULL."""
    L = get_lib()
    L.ms_openfile(_b(path))
    while True:
        s = L.ms_next_block(int(segment_length), int(folded), int(sample_first), int(sample_size))
        if not s:
            return
        yield s


PERMUTE_MODES = {"parity": 0, "throughput": 1}


def set_permute_mode(mode: str = "parity", seed: int = 0xFD821A6) -> None:
    """scan_permute's mode (include/fscl_amd.h): "parity" (the reference's rand() stream) or
    "throughput" (counter-based random numbers from `seed`, labelled non-parity)."""
    if get_lib().fscl_amd_set_permute_mode(PERMUTE_MODES[mode], int(seed)) != 0:
        raise ValueError(mode)


def background_fsp(scan, force_neutral: bool = False, bs_file=None, include_invariant: bool = False):
    return get_lib().background_fsp(scan, int(force_neutral), _b(bs_file), int(include_invariant))


def output_background_fs(path, scan, fsp) -> None:
    get_lib().output_background_fs(_b(path), scan, fsp)


def compute_sweep_model_tables(scan, fsp, asc_depth: int = 0, asc_min_freq: int = 1,
                               ascbias_background_only: bool = False, include_invariant: bool = False):
    return get_lib().compute_sweep_model_tables(scan, fsp, int(asc_depth), int(asc_min_freq),
                                          int(ascbias_background_only), int(include_invariant))


def compute_snp_null_model(scan, fsp) -> None:
    get_lib().compute_snp_null_model(scan, fsp)


def scan_chromosome(scan, tables, eval_range: int = 81920, bp_resl: int = 128, large_grid_sp: int = 100000,
                    n_threads: int = 1) -> None:
    get_lib().scan_chromosome(scan, tables, eval_range, bp_resl, large_grid_sp, n_threads)


def scan_permute(scan, tables, n_permute: int, permute_nbp: float = 0.1, alpha_factor: float = 1.0,
                 n_threads: int = 1, eval_range: int = 81920, bp_resl: int = 128, large_grid_sp: int = 100000,
                 scan_width_mb: float = 1.0) -> None:
    get_lib().scan_permute(scan, tables, int(n_permute), float(permute_nbp), float(alpha_factor), int(n_threads),
                     int(eval_range), int(bp_resl), int(large_grid_sp), float(scan_width_mb))


def scan_output(path, scan, max_only: bool = False, n_permute: int = 0, label=None) -> None:
    get_lib().scan_output(_b(path), scan, int(max_only), int(n_permute), _b(label))


POINT_DTYPE = np.dtype([("chr", "i4"), ("sweep_pos", "i4"), ("clr", "f8"), ("lalpha", "f8"), ("sm_logl", "f8"),
                        ("null_logl", "f8"), ("nearest_snp", "i4"), ("window_start", "i4"), ("window_end", "i4"),
                        ("n_snps", "i4"), ("permute_p", "i4"), ("permute_n", "i4"), ("permute_finished", "i4")])


def points(scan) -> np.ndarray:
    """The scan points of a scan_t as a numpy structured array."""
    s = scan.contents
    out = np.zeros(s.n_scan_pts, dtype=POINT_DTYPE)
    for i in range(s.n_scan_pts):
        p = s.scan_pts[i]
        out[i] = (p.chr, p.sweep_pos, p.clr, p.lalpha, p.sm_logl, p.null_logl, p.nearest_snp, p.window_start,
                  p.window_end, p.n_snps, p.permute_p, p.permute_n, p.permute_finished)
    return out


PROFILE_DTYPE = np.dtype(POINT_DTYPE.descr + [("grid_pos", "i4"), ("cell", "i4")])


# the C layouts of scan_pt_t and fsclg_point_t (the pointer as an integer)
_SCANPT_RAW = np.dtype([("chr", "i4"), ("nearest_snp", "i4"), ("sweep_pos", "i4"), ("n_snps", "i4"),
                        ("window_start", "i4"), ("window_end", "i4"), ("lalpha", "f8"), ("null_logl", "f8"),
                        ("sm_logl", "f8"), ("clr", "f8"), ("permute_n", "i4"), ("permute_p", "i4"),
                        ("permute_finished", "i4"), ("scan_running", "i4"), ("permute_clr", "u8")])
_POINT_RAW = np.dtype([("chr", "i4"), ("nearest_snp", "i4"), ("sweep_pos", "i4"), ("n_snps", "i4"),
                       ("window_start", "i4"), ("window_end", "i4"), ("flags", "i4"), ("cost", "u4"),
                       ("lalpha", "f8"), ("null_logl", "f8"), ("sm_logl", "f8"), ("clr", "f8")])
assert _SCANPT_RAW.itemsize == C.sizeof(ScanPtT) and _POINT_RAW.itemsize == C.sizeof(PointT)


def _pts_array(pts, n, dtype=POINT_DTYPE) -> np.ndarray:
    """n structs (ScanPtT or PointT) at `pts` as a structured array of `dtype`'s point fields."""
    out = np.zeros(n, dtype=dtype)
    if n:
        ct = pts._type_
        raw = np.frombuffer((ct * n).from_address(C.addressof(pts.contents) if hasattr(pts, "contents")
                                                  else C.addressof(pts)),
                            dtype=_SCANPT_RAW if ct is ScanPtT else _POINT_RAW)
        have = set(raw.dtype.names)
        for k in POINT_DTYPE.names:
            if k in have:
                out[k] = raw[k]
    return out


def _libc_free(*ptrs) -> None:
    free = C.CDLL(None).free
    free.argtypes = [C.c_void_p]
    for p in ptrs:
        free(C.cast(p, C.c_void_p))


def profile_chunk() -> int:
    """Positions per workgroup of the profile kernel ($FSCLG_PROFILE_CHUNK, read per call)."""
    return int(get_lib().fsclg_profile_chunk())


def profile_last_ms() -> float:
    return float(get_lib().fscl_amd_profile_last_ms())


def profile_grid(scan, small_grid_sp: int = 1000, large_grid_sp: int = 100000):
    """The fine grid alone (no GPU): (chr, grid_pos, cell) int32 arrays."""
    pc, pp, pe = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_int)()
    n = get_lib().fscl_amd_profile_grid(scan, int(small_grid_sp), int(large_grid_sp), C.byref(pc), C.byref(pp),
                                        C.byref(pe))
    if n < 0:
        raise ValueError("small_grid_sp must be positive and divide large_grid_sp")
    out = tuple(np.array(a[:n], dtype=np.int32) for a in (pc, pp, pe))
    _libc_free(pc, pp, pe)
    return out


def profile_runs(scan, tables, runs, eval_range: int = 81920) -> np.ndarray:
    """init_scan_result + search_maxalpha at start + k * step, k < count, for each
    (chr, start, step, count) of ``runs``: a POINT_DTYPE array in run order."""
    arr = (RunT * max(len(runs), 1))(*[RunT(*[int(v) for v in r]) for r in runs])
    n = sum(max(int(r[3]), 0) for r in runs)
    out = (PointT * max(n, 1))()
    r = get_lib().fscl_amd_profile_runs(scan, tables, arr, len(runs), int(eval_range), out)
    if r != 0:
        raise RuntimeError(f"fscl_amd_profile_runs: code {r}: {get_lib().fsclg_last_error().decode()}")
    return _pts_array(out, n)


def scan_profile(scan, tables, eval_range: int = 81920, small_grid_sp: int = 1000,
                 large_grid_sp: int = 100000) -> np.ndarray:
    """CLR and alpha at every small_grid_sp-spaced position (include/fscl_amd.h): points()'s
    fields plus grid_pos (the requested position) and cell (its coarse cell)."""
    pf = get_lib().fscl_amd_scan_profile(scan, tables, int(eval_range), int(small_grid_sp), int(large_grid_sp))
    if not pf:
        return np.zeros(0, dtype=PROFILE_DTYPE)
    n = pf.contents.n_pts
    out = _pts_array(pf.contents.pts, n, PROFILE_DTYPE)
    out["grid_pos"] = np.array(pf.contents.grid_pos[:n], dtype=np.int32)
    out["cell"] = np.array(pf.contents.cell[:n], dtype=np.int32)
    get_lib().fscl_amd_profile_free(pf)
    return out


def _profile_struct(profile: np.ndarray):
    n = len(profile)
    pts = np.zeros(max(n, 1), dtype=_SCANPT_RAW)
    for k in POINT_DTYPE.names:
        pts[k][:n] = profile[k]
    gp = np.ascontiguousarray(np.resize(profile["grid_pos"], max(n, 1)) if n else np.zeros(1), dtype=np.int32)
    ce = np.ascontiguousarray(np.resize(profile["cell"], max(n, 1)) if n else np.zeros(1), dtype=np.int32)
    pf = ProfileT(n, pts.ctypes.data_as(C.POINTER(ScanPtT)), gp.ctypes.data_as(C.POINTER(C.c_int)),
                  ce.ctypes.data_as(C.POINTER(C.c_int)))
    return pf, (pts, gp, ce)


def profile_cell_max(profile: np.ndarray, scan):
    """Per coarse cell the first grid point of strictly greatest CLR, and the number of cells
    whose grid maximum exceeds the scan's (bisection's) point: (POINT_DTYPE array, n_missed).
    Needs scan_chromosome to have run (ValueError otherwise)."""
    pf, keep = _profile_struct(profile)
    n_cells = scan.contents.n_scan_pts
    out = (ScanPtT * max(n_cells, 1))()
    missed = C.c_int(0)
    r = get_lib().fscl_amd_profile_cell_max(C.byref(pf), scan, out, C.byref(missed))
    del keep
    if r < 0:
        raise ValueError("profile_cell_max needs scan_chromosome's points")
    return _pts_array(out, r), missed.value


def profile_output(path, scan, profile: np.ndarray, label=None) -> None:
    pf, keep = _profile_struct(profile)
    get_lib().fscl_amd_profile_output(_b(path), scan, C.byref(pf), _b(label))
    del keep


def scan_chromosome_grid(scan, tables, eval_range: int = 81920, small_grid_sp: int = 1000,
                         large_grid_sp: int = 100000) -> None:
    """scan_chromosome's grid counterpart (include/fscl_amd.h): each cell's point is the first of
    strictly greatest CLR among its small_grid_sp-spaced positions, in cell order."""
    get_lib().fscl_amd_scan_chromosome_grid(scan, tables, int(eval_range), int(small_grid_sp), int(large_grid_sp))


def scan_permute_grid(scan, tables, n_permute: int, permute_nbp: float = 0.1, eval_range: int = 81920,
                      small_grid_sp: int = 1000, large_grid_sp: int = 100000, scan_width_mb: float = 1.0) -> None:
    """scan_permute's grid counterpart on scan_chromosome_grid's points: every trial takes each
    active point's own cell's grid maximum on the permuted rows (one process, parity stream)."""
    get_lib().fscl_amd_scan_permute_grid(scan, tables, int(n_permute), float(permute_nbp), int(eval_range),
                                         int(small_grid_sp), int(large_grid_sp), float(scan_width_mb))


def site_rows(scan, tables) -> np.ndarray:
    """The device row of every site as uploaded (uint32): what a permutation of the sites rearranges."""
    out = np.zeros(max(scan.contents.n_snps, 1), dtype=np.uint32)
    n = get_lib().fscl_amd_site_rows(scan, tables, out.ctypes.data)
    if n < 0:
        raise RuntimeError("fscl_amd_site_rows failed")
    return out[:n]


def _runs_rows(scan, runs, rows):
    """What the *_runs handles share: the RunT array of ``runs`` (chr, start, step, count) and the pointer to
    ``rows`` as uint32, one per site, or None (the pointer keeps its array alive)."""
    arr = (RunT * max(len(runs), 1))(*[RunT(*[int(v) for v in r]) for r in runs])
    if rows is None:
        return arr, None
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    if len(rows) != scan.contents.n_snps:
        raise ValueError("rows must hold one row per site")
    return arr, rows.ctypes.data_as(C.c_void_p)


def _run_alphas(runs, alphas):
    """(la [len(runs)][n_la], sum(count), n_la) of one alpha list per run, all of one length."""
    la = np.ascontiguousarray(alphas, dtype=np.float64).reshape(len(runs), -1) if len(runs) else np.zeros((0, 1))
    return la, sum(max(int(r[3]), 0) for r in runs), la.shape[1]


def cellmax_runs(scan, tables, runs, eval_range: int = 81920, rows=None) -> np.ndarray:
    """Per (chr, start, step, count) of ``runs`` the first position of strictly greatest CLR, through
    fsclg_cellmax_submit / fsclg_cellmax_wait on the scan's context: one POINT_DTYPE row per run (a
    zero-count run: a zeroed row).  ``rows``: a uint32 array of n_snps device rows (a rearrangement of
    site_rows) set into the slot first; None: the uploaded rows."""
    out = (PointT * max(len(runs), 1))()
    arr, rp = _runs_rows(scan, runs, rows)
    r = get_lib().fscl_amd_cellmax_runs(scan, tables, arr, len(runs), int(eval_range), rp, out)
    if r != 0:
        raise RuntimeError(f"fscl_amd_cellmax_runs: code {r}: {get_lib().fsclg_last_error().decode()}")
    return _pts_array(out, len(runs))


def cellmax_last_ms() -> float:
    return float(get_lib().fscl_amd_cellmax_last_ms())


CURVE_MAX = 27  # FSCLG_CURVE_MAX: 11 coarse + 16 refine candidates at most
# fsclg_curve_t (= fscl_amd_curve_t): the position's point, then the alpha search's candidates in the
# reference's evaluation order -- la[k] the log alpha, sm[k] its sm_likelihood value, k < n_coarse + n_refine
CURVE_DTYPE = np.dtype([("pt", _POINT_RAW), ("n_coarse", "i4"), ("n_refine", "i4"), ("la", "f8", (CURVE_MAX,)),
                        ("sm", "f8", (CURVE_MAX,))])
assert CURVE_DTYPE.itemsize == _POINT_RAW.itemsize + 8 + 16 * CURVE_MAX


def _curve_check(r: int, what: str) -> None:
    if r != 0:
        raise RuntimeError(f"{what}: code {r}: {get_lib().fsclg_last_error().decode()}")


def scan_curves(scan, tables, chr_pos, eval_range: int = 81920) -> np.ndarray:
    """The alpha likelihood curve at each (chromosome index, position) of ``chr_pos``, on the data as
    loaded (include/fscl_amd.h): a CURVE_DTYPE array in the given order."""
    cp = np.ascontiguousarray(np.asarray(chr_pos, dtype=np.int32).reshape(-1, 2).T)  # [chr..., pos...]
    n = cp.shape[1]
    out = np.zeros(max(n, 1), dtype=CURVE_DTYPE)
    _curve_check(get_lib().fscl_amd_scan_curves(scan, tables, int(eval_range), cp[0].ctypes.data, cp[1].ctypes.data, n,
                                                out.ctypes.data), "fscl_amd_scan_curves")
    return out[:n]


def scan_point_curves(scan, tables, eval_range: int = 81920) -> np.ndarray:
    """The curve of every scan point at its own sweep_pos (after scan_chromosome or
    scan_chromosome_grid): a CURVE_DTYPE array in points() order."""
    n = scan.contents.n_scan_pts
    out = np.zeros(max(n, 1), dtype=CURVE_DTYPE)
    _curve_check(get_lib().fscl_amd_scan_point_curves(scan, tables, int(eval_range), out.ctypes.data),
                 "fscl_amd_scan_point_curves")
    return out[:n]


def curve_runs(scan, tables, runs, eval_range: int = 81920, rows=None, out=None) -> np.ndarray:
    """The curves at start + k * step, k < count, for each (chr, start, step, count) of ``runs``, through
    fsclg_curve_submit / fsclg_curve_wait on the scan's first device (the shim-level handle, next to
    cellmax_runs): a CURVE_DTYPE array in run order.  ``rows`` as for cellmax_runs; ``out``: a
    CURVE_DTYPE array to fill (tests pre-fill it)."""
    n = sum(max(int(r[3]), 0) for r in runs)
    if out is None:
        out = np.zeros(max(n, 1), dtype=CURVE_DTYPE)
    if out.dtype != CURVE_DTYPE or len(out) < n or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous CURVE_DTYPE array of sum(count) records")
    arr, rp = _runs_rows(scan, runs, rows)
    _curve_check(get_lib().fscl_amd_curve_runs(scan, tables, arr, len(runs), int(eval_range), rp, out.ctypes.data),
                 "fscl_amd_curve_runs")
    return out[:n]


def curve_support(curve, drop: float = 2.0):
    """(la_lo, la_hi, open_lo, open_hi) of one CURVE_DTYPE record: the log alphas bounding the
    connected run around the argmax whose sm >= sm_max - drop, and whether it reaches the lowest /
    highest evaluated alpha; None if no value beat the initial state (all NaN).  Host only.  The
    likelihood is composite: the interval describes the curve, it is not a calibrated confidence interval."""
    rec = np.ascontiguousarray(np.asarray(curve, dtype=CURVE_DTYPE).reshape(1))
    lo, hi, ol, oh = C.c_double(), C.c_double(), C.c_int(), C.c_int()
    r = get_lib().fscl_amd_curve_support(rec.ctypes.data, float(drop), C.byref(lo), C.byref(hi), C.byref(ol), C.byref(oh))
    if r < 0:
        raise ValueError("drop must be >= 0")
    return (lo.value, hi.value, bool(ol.value), bool(oh.value)) if r == 1 else None


def curve_output(path, scan, curves: np.ndarray, drop: float = 2.0, label=None) -> None:
    """The --alpha-file format (include/fscl_amd.h, README): one row per point and alpha, one
    summary row per point."""
    cv = np.ascontiguousarray(curves, dtype=CURVE_DTYPE)
    get_lib().fscl_amd_curve_output(_b(path), scan, cv.ctypes.data if len(cv) else None, len(cv), float(drop), _b(label))


def curve_last_ms() -> float:
    return float(get_lib().fscl_amd_curve_last_ms())


def curve_forced() -> int:
    """Walks summed sequentially only because a curve wants every value exact (since reset_stats)."""
    return int(get_lib().fscl_amd_curve_forced())


# fsclg_site_req_t: one walk of sm_likelihood -- chromosome index, position, log alpha
SITE_REQ_DTYPE = np.dtype([("chr", "i4"), ("pos", "i4"), ("lalpha", "f8")])
# fsclg_site_hdr_t: the walk's point (lalpha the request's, sm_logl the sequential sum of null_logl and
# the terms), the terms left / right of the nearest SNP, len = 0 or 1 + nl + nr, and where the walk's
# terms start in the flat terms array; term k belongs to site nearest_snp (k = 0), nearest_snp - k
# (k <= nl) or nearest_snp + k - nl
SITES_DTYPE = np.dtype([("pt", _POINT_RAW), ("nl", "i4"), ("nr", "i4"), ("len", "i4"), ("pad", "i4"), ("off", "u8")])
assert SITES_DTYPE.itemsize == _POINT_RAW.itemsize + 24
# fscl_amd_sites_summary_t (include/fscl_amd.h); top_term / top_share NaN where the file prints NA
SITES_SUMMARY_DTYPE = np.dtype([("n_sites", "i4"), ("first_pos", "i4"), ("last_pos", "i4"), ("n_pos", "i4"),
                                ("n_neg", "i4"), ("top_pos", "i4"), ("n_half", "i4"), ("pad", "i4"),
                                ("top_term", "f8"), ("top_share", "f8")])


def _sites_take(res: SitesT):
    """(headers, terms) copied out of a native result, which is released."""
    n, nt = int(res.n), int(res.n_terms)
    hdr = np.zeros(n, dtype=SITES_DTYPE)
    terms = np.zeros(nt, dtype=np.float64)
    if n:
        C.memmove(hdr.ctypes.data, res.hdr, n * SITES_DTYPE.itemsize)
    if nt:
        C.memmove(terms.ctypes.data, res.terms, nt * 8)
    get_lib().fscl_amd_sites_free(C.byref(res))
    return hdr, terms


def scan_sites(scan, tables, requests, eval_range: int = 81920):
    """The per-site likelihood terms of one sm_likelihood walk per (chromosome index, position, log alpha)
    of ``requests``, on the data as loaded (include/fscl_amd.h): (headers, terms) -- a SITES_DTYPE array
    in the given order and the flat float64 array its ``off`` / ``len`` index, in walk order."""
    req = np.zeros(len(requests), dtype=SITE_REQ_DTYPE)
    for q, r in zip(req, requests):
        q["chr"], q["pos"], q["lalpha"] = int(r[0]), int(r[1]), float(r[2])
    res = SitesT()
    _curve_check(get_lib().fscl_amd_scan_sites(scan, tables, int(eval_range), req.ctypes.data if len(req) else None,
                                               len(req), C.byref(res)), "fscl_amd_scan_sites")
    return _sites_take(res)


def scan_point_sites(scan, tables, top: int = 10, eval_range: int = 81920):
    """The walks of the scan points at their own sweep_pos and lalpha (after scan_chromosome or
    scan_chromosome_grid): the ``top`` points of greatest CLR (0: every point), in points() order."""
    res = SitesT()
    _curve_check(get_lib().fscl_amd_scan_point_sites(scan, tables, int(eval_range), int(top), C.byref(res)),
                 "fscl_amd_scan_point_sites")
    return _sites_take(res)


# fsclg_expect_site_t: one site of a walk -- its index, 1 if degenerate, x = logt(|d|) + log alpha, the observed
# term, the first two moments of the term under the sweep and under neutrality, the probability lost to
# unusable classes (include/fsclg.h)
EXPECT_SITE_DTYPE = np.dtype([("site", "i4"), ("degenerate", "i2"), ("bin", "i2"), ("x", "f8"), ("obs", "f8"), ("m1_s", "f8"),
                              ("m2_s", "f8"), ("m1_0", "f8"), ("m2_0", "f8"), ("lost_s", "f8"), ("lost_0", "f8")])
# fsclg_expect_tot_t: the totals of a walk's sites in one bin (or in all): sums of log-likelihood terms
EXPECT_DTYPE = np.dtype([("n_sites", "u4"), ("n_degenerate", "u4"), ("obs", "f8"), ("e_s", "f8"), ("v_s", "f8"),
                         ("e_0", "f8"), ("v_0", "f8"), ("max_lost_s", "f8"), ("max_lost_0", "f8")])
assert EXPECT_SITE_DTYPE.itemsize == 72 and EXPECT_DTYPE.itemsize == 64


def _expect_check(r: int, what: str) -> None:
    if r != 0:
        msg = get_lib().fscl_amd_expect_error() or get_lib().fsclg_last_error() or b""
        raise ValueError(f"{what} failed (code {r}): {msg.decode()}") if r == -1 else RuntimeError(
            f"{what} failed (code {r}): {msg.decode()}")


def _expect_take(res: ExpectT) -> dict:
    n, nt, nb = int(res.n), int(res.n_tasks), int(res.n_bins)
    out = {"n_bins": nb, "kernel_ms": float(res.kernel_ms), "evaluated": bool(res.hdr),
           "req": np.zeros(n, dtype=SITE_REQ_DTYPE), "first": np.zeros(n + 1, dtype=np.int32),
           "own": np.zeros(n, dtype=np.int32), "la": np.zeros(nt, dtype=np.float64),
           "hdr": np.zeros(nt, dtype=SITES_DTYPE), "tot": np.zeros((nt, nb + 1), dtype=EXPECT_DTYPE),
           "point": None}
    if res.hdr:
        for key, ptr in (("req", res.req), ("first", res.first), ("own", res.own), ("la", res.la), ("hdr", res.hdr),
                         ("tot", res.tot)):
            if out[key].nbytes:
                C.memmove(out[key].ctypes.data, ptr, out[key].nbytes)
        if res.point:
            out["point"] = np.zeros(n, dtype=np.int32)
            if n:
                C.memmove(out["point"].ctypes.data, res.point, 4 * n)
    return out


def _expect_res(d: dict):
    res = ExpectT()
    keep = {k: np.ascontiguousarray(d[k]) for k in ("req", "first", "own", "la", "hdr", "tot")}
    res.n, res.n_tasks, res.n_bins = len(keep["req"]), len(keep["la"]), int(d["n_bins"])
    for k, a in keep.items():
        setattr(res, k, a.ctypes.data)
    return res, keep


def scan_expect(scan, tables, fsp, requests, alphas, n_bins: int = 24, eval_range: int = 81920) -> dict:
    """The expected terms under the model (include/fscl_amd.h, --expect-file) of one sweep per (chromosome
    index, position, log alpha) of ``requests``: each at the ascending log alphas ``alphas`` with its own inserted
    in order.  A dict: ``first`` / ``own`` index the tasks of a request, ``la`` their log alphas, ``hdr`` their
    walks (SITES_DTYPE), ``tot[task, b]`` (EXPECT_DTYPE) the totals of bin b, ``tot[task, n_bins]`` of the walk."""
    req = np.zeros(len(requests), dtype=SITE_REQ_DTYPE)
    for q, r in zip(req, requests):
        q["chr"], q["pos"], q["lalpha"] = int(r[0]), int(r[1]), float(r[2])
    la = np.ascontiguousarray(alphas, dtype=np.float64)
    res = ExpectT()
    _expect_check(get_lib().fscl_amd_scan_expect(scan, tables, fsp, int(eval_range), req.ctypes.data if len(req) else None,
                                                 len(req), la.ctypes.data if len(la) else None, len(la), int(n_bins),
                                                 C.byref(res)), "fscl_amd_scan_expect")
    out = _expect_take(res)
    get_lib().fscl_amd_expect_free(C.byref(res))
    return out


def scan_point_expect(scan, tables, fsp, alphas, top: int = 3, spacing: int = 100000, n_bins: int = 24,
                      eval_range: int = 81920) -> dict:
    """scan_expect at the ``top`` scan points of greatest CLR at their fitted alpha, none within ``spacing`` bp of
    one already taken; ``point`` holds each request's scan point."""
    la = np.ascontiguousarray(alphas, dtype=np.float64)
    res = ExpectT()
    _expect_check(get_lib().fscl_amd_scan_point_expect(scan, tables, fsp, int(eval_range), int(top), int(spacing),
                                                       la.ctypes.data if len(la) else None, len(la), int(n_bins),
                                                       C.byref(res)), "fscl_amd_scan_point_expect")
    out = _expect_take(res)
    get_lib().fscl_amd_expect_free(C.byref(res))
    return out


def expect_output(path, scan, result: dict, label=None) -> None:
    """The --expect-file format (include/fscl_amd.h, README) of a scan_expect result."""
    res, keep = _expect_res(result)
    if get_lib().fscl_amd_expect_output(_b(path), scan, C.byref(res), _b(label)) != 0:
        raise OSError(f"cannot write {path}")
    del keep


def expect_last_ms() -> float:
    return float(get_lib().fscl_amd_expect_last_ms())


def expect_runs(scan, tables, fsp, requests, alphas, n_bins: int = 24, eval_range: int = 81920, batch: int = 0):
    """The raw handle of fsclg_expect_submit / fsclg_expect_wait on the first device: ``alphas`` is one list of log
    alphas per request, all of one length.  (totals [task, n_bins + 1], headers [task], site records), the tasks
    request-major, the site records task after task (hdr["off"], hdr["len"])."""
    req = np.zeros(len(requests), dtype=SITE_REQ_DTYPE)
    for q, r in zip(req, requests):
        q["chr"], q["pos"], q["lalpha"] = int(r[0]), int(r[1]), float(r[2])
    la = np.ascontiguousarray(alphas, dtype=np.float64).reshape(len(req), -1)
    n_la = la.shape[1]
    nt = len(req) * n_la
    tot = np.zeros((nt, int(n_bins) + 1), dtype=EXPECT_DTYPE)
    hdr = np.zeros(nt, dtype=SITES_DTYPE)
    ptr, ns = C.c_void_p(), C.c_size_t()
    r = get_lib().fscl_amd_expect_runs(scan, tables, fsp, req.ctypes.data if len(req) else None, len(req),
                                       la.ctypes.data if la.size else None, n_la, int(n_bins), int(eval_range), int(batch),
                                       tot.ctypes.data, hdr.ctypes.data, C.byref(ptr), C.byref(ns))
    if r != 0:
        raise (ValueError if r == -1 else RuntimeError)(
            f"fscl_amd_expect_runs failed (code {r}): {(get_lib().fsclg_last_error() or b'').decode()}")
    sites = np.zeros(ns.value, dtype=EXPECT_SITE_DTYPE)
    if ns.value:
        C.memmove(sites.ctypes.data, ptr, sites.nbytes)
    _libc_free(ptr)
    return tot, hdr, sites


def _sites_view(hdr, terms):
    h = np.ascontiguousarray(hdr, dtype=SITES_DTYPE)
    t = np.ascontiguousarray(terms, dtype=np.float64)
    if len(h) and int((h["off"] + h["len"].astype(np.uint64)).max()) > len(t):
        raise ValueError("a header's terms lie past the terms array")
    res = SitesT(len(h), None, h.ctypes.data if len(h) else None,
                 t.ctypes.data_as(C.POINTER(C.c_double)) if len(t) else None, len(t))
    return res, (h, t)  # (the arrays stay alive with the view)


def sites_summary(scan, hdr, terms) -> np.ndarray:
    """The footprint summary of each walk (include/fscl_amd.h): a SITES_SUMMARY_DTYPE array.  Host only."""
    res, keep = _sites_view(hdr, terms)
    out = np.zeros(max(res.n, 1), dtype=SITES_SUMMARY_DTYPE)
    get_lib().fscl_amd_sites_summary(scan, C.byref(res), out.ctypes.data)
    return out[:res.n]


def sites_output(path, scan, hdr, terms, label=None) -> None:
    """The --sites-file format (include/fscl_amd.h, README): per walk one row per site in ascending
    position, then one summary row.  Host only."""
    res, keep = _sites_view(hdr, terms)
    get_lib().fscl_amd_sites_output(_b(path), scan, C.byref(res), _b(label))


def sites_last_ms() -> float:
    return float(get_lib().fscl_amd_sites_last_ms())


def sites_cap() -> int:
    """Terms per launch of the term kernel ($FSCLG_SITES_CAP)."""
    return int(get_lib().fsclg_sites_cap())


SURFACE_MAX_LA = 64  # FSCL_AMD_SURFACE_MAX_LA: alphas per list at most
LOG_AD_MIN, LOG_AD_MAX = -20.0, 4.0
# fscl_amd_surface_req_t: chromosome index, centre position, half-width and step in bp, the list's length,
# the scan point the request is centred on (-1: none), the ascending log alphas
SURFACE_REQ_DTYPE = np.dtype([("chr", "i4"), ("centre_pos", "i4"), ("halfwidth", "i4"), ("step", "i4"), ("n_la", "i4"),
                              ("point", "i4"), ("la", "f8", (SURFACE_MAX_LA,))])
# fscl_amd_surface_hdr_t: the request, the run evaluated (start_pos + p * step, p < n_pos) and where the
# surface's points and values start in the result's flat arrays
SURFACE_DTYPE = np.dtype([("chr", "i4"), ("centre_pos", "i4"), ("halfwidth", "i4"), ("step", "i4"), ("n_la", "i4"),
                          ("point", "i4"), ("start_pos", "i4"), ("n_pos", "i4"), ("pos_off", "u8"), ("cell_off", "u8"),
                          ("la", "f8", (SURFACE_MAX_LA,))])
assert SURFACE_REQ_DTYPE.itemsize == 24 + 8 * SURFACE_MAX_LA and SURFACE_DTYPE.itemsize == 48 + 8 * SURFACE_MAX_LA
# fscl_amd_surface_region_t: indices into the surface's positions and alphas (-1: every cell NaN)
SURFACE_REGION_DTYPE = np.dtype([(k, "i4") for k in ("n_pos", "n_la", "max_ipos", "max_ila", "ipos_lo", "ipos_hi", "ila_lo",
                                                      "ila_hi", "open_pos_lo", "open_pos_hi", "open_la_lo", "open_la_hi",
                                                      "n_region", "pad")] + [("max_v", "f8")])


class Surface:
    """One position-by-alpha surface: ``hdr`` (a SURFACE_DTYPE record), ``la`` (the n_la log alphas),
    ``pts`` (the n_pos points, fsclg_point_t fields) and ``sm`` (float64 [n_pos][n_la], what
    sm_likelihood returns at each position and alpha)."""

    def __init__(self, hdr, pts, sm):
        self.hdr, self.pts, self.sm = hdr, pts, sm
        self.la = np.array(hdr["la"][:int(hdr["n_la"])], dtype=np.float64)

    @property
    def null_logl(self):
        return np.ascontiguousarray(self.pts["null_logl"], dtype=np.float64)


def surface_alphas(lo: float = LOG_AD_MIN, hi: float = LOG_AD_MAX, n: int = 33, fitted: float = float("nan")) -> np.ndarray:
    """The grid lo + i (hi - lo) / (n - 1), i < n, with ``fitted`` inserted in order (not when it equals a
    grid value, is NaN or lies outside [-20, 4]).  Host only."""
    out = np.zeros(SURFACE_MAX_LA, dtype=np.float64)
    m = get_lib().fscl_amd_surface_alphas(float(lo), float(hi), int(n), float(fitted), out.ctypes.data)
    if m < 1:
        raise ValueError("surface alphas: -20 <= lo <= hi <= 4, 1 <= n <= 63, lo < hi unless n is 1")
    return out[:m].copy()


_surface_grid = surface_alphas  # (run() has a keyword of that name)


def _surface_requests(requests) -> np.ndarray:
    req = np.zeros(len(requests), dtype=SURFACE_REQ_DTYPE)
    for q, r in zip(req, requests):
        la = np.asarray(r[4], dtype=np.float64).reshape(-1)
        if not 1 <= len(la) <= SURFACE_MAX_LA:
            raise ValueError("a surface takes 1 to 64 alphas")
        q["chr"], q["centre_pos"], q["halfwidth"], q["step"] = (int(v) for v in r[:4])
        q["n_la"], q["point"] = len(la), int(r[5]) if len(r) > 5 else -1
        q["la"][:len(la)] = la
    return req


def surface_run(scan, request):
    """(chr, start_pos, step, count): the positions of one request (chr, centre, halfwidth, step, alphas)
    clipped to the chromosome's span.  Host only."""
    req = _surface_requests([request])
    run = RunT()
    if get_lib().fscl_amd_surface_run(scan, req.ctypes.data, C.byref(run)) != 0:
        raise ValueError("surface request: a chromosome of the scan, step >= 1, halfwidth >= 0")
    return int(run.chr), int(run.start_pos), int(run.step), int(run.count)


def _surfaces_take(res: SurfacesT) -> list:
    """The surfaces copied out of a native result, which is released."""
    n, npos, nc = int(res.n), int(res.n_pos), int(res.n_cells)
    hdr = np.zeros(n, dtype=SURFACE_DTYPE)
    pts = np.zeros(npos, dtype=_POINT_RAW)
    sm = np.zeros(nc, dtype=np.float64)
    if n:
        C.memmove(hdr.ctypes.data, res.hdr, n * SURFACE_DTYPE.itemsize)
    if npos:
        C.memmove(pts.ctypes.data, res.pts, npos * _POINT_RAW.itemsize)
    if nc:
        C.memmove(sm.ctypes.data, res.sm, nc * 8)
    terms = int(res.n_terms)
    get_lib().fscl_amd_surfaces_free(C.byref(res))
    out = []
    for h in hdr:
        p0, c0, m, k = int(h["pos_off"]), int(h["cell_off"]), int(h["n_pos"]), int(h["n_la"])
        out.append(Surface(h, pts[p0:p0 + m].copy(), sm[c0:c0 + m * k].reshape(m, k).copy()))
    _surface_terms[0] = terms
    return out


_surface_terms = [0]


def surface_last_terms() -> int:
    """The terms of the walks of the last scan_surface / scan_point_surfaces call."""
    return _surface_terms[0]


def scan_surface(scan, tables, requests, eval_range: int = 81920) -> list:
    """The likelihood surface of each request (chromosome index, centre position, half-width bp, step bp,
    ascending log alphas[, scan point index]), on the data as loaded (include/fscl_amd.h): a list of
    Surface in the given order."""
    req = _surface_requests(requests)
    res = SurfacesT()
    _curve_check(get_lib().fscl_amd_scan_surface(scan, tables, int(eval_range), req.ctypes.data if len(req) else None,
                                                 len(req), C.byref(res)), "fscl_amd_scan_surface")
    return _surfaces_take(res)


def scan_point_surfaces(scan, tables, top: int = 3, halfwidth: int = 100000, step: int = 1000, alphas=(LOG_AD_MIN, LOG_AD_MAX, 33),
                        eval_range: int = 81920) -> list:
    """The surfaces around the ``top`` scan points of greatest CLR (none within ``halfwidth`` of one already
    chosen), each centred on its sweep_pos, on the grid ``alphas`` = (lo, hi, n) with the point's fitted
    lalpha inserted: a list of Surface in descending CLR order."""
    res = SurfacesT()
    _curve_check(get_lib().fscl_amd_scan_point_surfaces(scan, tables, int(eval_range), int(top), int(halfwidth), int(step),
                                                        float(alphas[0]), float(alphas[1]), int(alphas[2]), C.byref(res)),
                 "fscl_amd_scan_point_surfaces")
    return _surfaces_take(res)


def top_points(scan, top: int, spacing: int, accept=None) -> np.ndarray:
    """The indices of at most ``top`` scan points by descending CLR (ties in scan order, a NaN never), none
    within ``spacing`` bp of one already chosen on its chromosome; ``accept(ScanPtT) -> bool`` rejects points
    without blocking their neighbours.  Host only."""
    idx = np.zeros(max(int(top), 1), dtype=np.int32)
    fn = TOP_ACCEPT_FN(lambda p: int(bool(accept(p.contents)))) if accept else TOP_ACCEPT_FN()
    n = get_lib().fscl_amd_top_points(scan, int(top), int(spacing), fn, idx.ctypes.data)
    if n < 0:
        raise ValueError("fscl_amd_top_points: no scan")
    return idx[:n].copy()


def _sampler_takes_alpha(p) -> bool:
    """The ``accept`` rule of the bootstrap's peak selection (the CLI's sampler_takes_alpha): the point's
    alpha = exp(lalpha) is positive and finite, else the sampler refuses it."""
    with np.errstate(over="ignore"):
        return bool(0.0 < float(np.exp(p.lalpha)) < np.inf)


def surface_runs(scan, tables, runs, alphas, eval_range: int = 81920, rows=None, batch: int = 0, pts=None, sm=None):
    """fsclg_surface_submit / fsclg_surface_wait on the scan's first device (the shim-level handle, next to
    curve_runs): ``alphas`` holds one ascending list per run, all of one length.  Returns (points
    [sum(count)], values [sum(count)][n_la]); ``pts`` / ``sm``: arrays to fill (tests pre-fill them)."""
    la, n, k = _run_alphas(runs, alphas)
    if pts is None:
        pts = np.zeros(max(n, 1), dtype=_POINT_RAW)
    if sm is None:
        sm = np.zeros(max(n, 1) * k, dtype=np.float64)
    if pts.dtype != _POINT_RAW or len(pts) < n or sm.dtype != np.float64 or sm.size < n * k or \
            not (pts.flags.c_contiguous and sm.flags.c_contiguous):
        raise ValueError("pts / sm must be contiguous arrays of sum(count) points and sum(count) * n_la values")
    arr, rp = _runs_rows(scan, runs, rows)
    _curve_check(get_lib().fscl_amd_surface_runs(scan, tables, arr, len(runs), la.ctypes.data, k, int(eval_range), rp,
                                                 int(batch), pts.ctypes.data, sm.ctypes.data), "fscl_amd_surface_runs")
    return pts[:n], sm.reshape(-1)[:n * k].reshape(n, k)


def surface_region(surface, drop: float = 2.0, null_logl=None):
    """The region summary of a Surface, or of a float64 [n_pos][n_la] array with the positions' null sums
    ``null_logl`` (default 0): (SURFACE_REGION_DTYPE record, uint8 marks [n_pos][n_la]: 2 the argmax, 1 the
    joint region, 0 elsewhere), or (record, marks) with indices -1 when every cell is NaN.  Host only.  The
    likelihood is composite: the region describes the surface, it is not a calibrated confidence region."""
    if isinstance(surface, Surface):
        sm, nul = surface.sm, surface.null_logl
    else:
        sm = np.asarray(surface, dtype=np.float64)
        nul = np.zeros(sm.shape[0]) if null_logl is None else np.asarray(null_logl, dtype=np.float64)
    sm = np.ascontiguousarray(sm, dtype=np.float64)
    nul = np.ascontiguousarray(nul, dtype=np.float64)
    if sm.ndim != 2 or sm.shape[0] < 1 or sm.shape[1] < 1 or nul.shape != (sm.shape[0],):
        raise ValueError("a surface is a non-empty [n_pos][n_la] array with one null sum per position")
    out = np.zeros(1, dtype=SURFACE_REGION_DTYPE)
    mark = np.zeros(sm.shape, dtype=np.uint8)
    r = get_lib().fscl_amd_surface_region(sm.ctypes.data, nul.ctypes.data, sm.shape[0], sm.shape[1], float(drop),
                                          out.ctypes.data, mark.ctypes.data)
    if r < 0:
        raise ValueError("drop must be >= 0")
    return out[0], mark


def surface_output(path, scan, surfaces, drop: float = 2.0, label=None) -> None:
    """The --surface-file format (include/fscl_amd.h, README): per surface one row per cell,
    position-major, then one summary row.  Host only."""
    n = len(surfaces)
    hdr = np.zeros(max(n, 1), dtype=SURFACE_DTYPE)
    po = co = 0
    for i, sf in enumerate(surfaces):
        hdr[i] = sf.hdr
        if sf.sm.shape != (len(sf.pts), int(sf.hdr["n_la"])):
            raise ValueError("a surface's values must be [n_pos][n_la]")
        hdr["n_pos"][i], hdr["pos_off"][i], hdr["cell_off"][i] = len(sf.pts), po, co
        po += len(sf.pts)
        co += sf.sm.size
    pts = np.concatenate([np.ascontiguousarray(sf.pts, dtype=_POINT_RAW) for sf in surfaces]) if n else np.zeros(0, _POINT_RAW)
    sm = np.concatenate([np.ascontiguousarray(sf.sm, dtype=np.float64).reshape(-1) for sf in surfaces]) if n else np.zeros(0)
    res = SurfacesT(n, hdr.ctypes.data, pts.ctypes.data if len(pts) else None, sm.ctypes.data if len(sm) else None,
                    len(pts), len(sm), 0)
    if get_lib().fscl_amd_surface_output(_b(path), scan, C.byref(res), float(drop), _b(label)) != 0:
        raise ValueError(f"surface_output: drop must be >= 0 and {path} writable")


def surface_last_ms() -> float:
    return float(get_lib().fscl_amd_surface_last_ms())


BLOCKS_MAX_NB = 1024  # FSCL_AMD_BLOCKS_MAX_NB: blocks per peak at most
# fscl_amd_blocks_hdr_t: the request, the run evaluated, the blocks (block j holds the sites with
# b0 + j == pos // block_bp; the edge blocks also what lies beyond) and where the peak's points and cells start
BLOCKS_DTYPE = np.dtype([("chr", "i4"), ("centre_pos", "i4"), ("halfwidth", "i4"), ("step", "i4"), ("n_la", "i4"),
                         ("point", "i4"), ("start_pos", "i4"), ("n_pos", "i4"), ("block_bp", "i4"), ("b0", "i4"), ("nb", "i4"),
                         ("pad", "i4"), ("pos_off", "u8"), ("cell_off", "u8"), ("la", "f8", (SURFACE_MAX_LA,))])
# fsclg_blocks_t: one run's blocks
BLOCKSPEC_DTYPE = np.dtype([("block_bp", "i4"), ("b0", "i4"), ("nb", "i4"), ("pad", "i4")])
# fscl_amd_jack_block_t / fscl_amd_jack_summary_t (fscl_amd_jackknife_combine)
JACK_BLOCK_DTYPE = np.dtype([("block", "i4"), ("has_terms", "i4"), ("ipos", "i4"), ("ila", "i4"), ("n_terms", "u4"),
                             ("pad", "i4"), ("v", "f8")])
JACK_SUMMARY_DTYPE = np.dtype([(k, "i4") for k in ("n_pos", "n_la", "nb", "g", "ipos", "ila", "top_shift", "top_loss",
                                                    "n_edge_pos", "n_edge_la")] +
                              [(k, "f8") for k in ("v", "se_pos", "se_la", "se_clr", "bias_pos", "bias_la", "bias_clr")])
assert BLOCKS_DTYPE.itemsize == 64 + 8 * SURFACE_MAX_LA and JACK_BLOCK_DTYPE.itemsize == 32 and JACK_SUMMARY_DTYPE.itemsize == 96


class Blocks:
    """The block sums of one peak: ``hdr`` (a BLOCKS_DTYPE record), ``la`` (the n_la log alphas), ``pts``
    (the n_pos points), ``bs`` (float64 [n_pos][nb][n_la]: the surface's terms summed per block) and
    ``cnt`` (uint32, the same shape: their counts)."""

    def __init__(self, hdr, pts, bs, cnt):
        self.hdr, self.pts, self.bs, self.cnt = hdr, pts, bs, cnt
        self.la = np.array(hdr["la"][:int(hdr["n_la"])], dtype=np.float64)

    @property
    def sweep_pos(self):
        return np.ascontiguousarray(self.pts["sweep_pos"], dtype=np.int32)


def _blocks_take(res: BlocksT) -> list:
    """The peaks copied out of a native result, which is released."""
    n, npos, nc = int(res.n), int(res.n_pos), int(res.n_cells)
    hdr = np.zeros(n, dtype=BLOCKS_DTYPE)
    pts = np.zeros(npos, dtype=_POINT_RAW)
    bs = np.zeros(nc, dtype=np.float64)
    cnt = np.zeros(nc, dtype=np.uint32)
    if n:
        C.memmove(hdr.ctypes.data, res.hdr, n * BLOCKS_DTYPE.itemsize)
    if npos:
        C.memmove(pts.ctypes.data, res.pts, npos * _POINT_RAW.itemsize)
    if nc:
        C.memmove(bs.ctypes.data, res.bs, nc * 8)
        C.memmove(cnt.ctypes.data, res.cnt, nc * 4)
    get_lib().fscl_amd_blocks_free(C.byref(res))
    out = []
    for h in hdr:
        p0, c0, m, b, k = int(h["pos_off"]), int(h["cell_off"]), int(h["n_pos"]), int(h["nb"]), int(h["n_la"])
        out.append(Blocks(h, pts[p0:p0 + m].copy(), bs[c0:c0 + m * b * k].reshape(m, b, k).copy(),
                          cnt[c0:c0 + m * b * k].reshape(m, b, k).copy()))
    return out


def blocks_cap() -> int:
    """$FSCL_AMD_BLOCKS_CAP: the bytes of block sums and counts one scan_blocks call may return (default 2^30)."""
    return int(get_lib().fscl_amd_blocks_cap())


def blocks_bound(scan, run, block_bp: int, eval_range: int = 81920):
    """(b0, nb): the blocks of the widest windows the positions of ``run`` = (chr, start_pos, step, count) can
    have.  Host only."""
    b0, nb = C.c_int(0), C.c_int(0)
    if get_lib().fscl_amd_blocks_bound(scan, C.byref(RunT(*[int(v) for v in run])), int(eval_range), int(block_bp),
                                       C.byref(b0), C.byref(nb)) != 0:
        raise ValueError("blocks_bound: a chromosome of the scan, step >= 1, block_bp >= 1")
    return b0.value, nb.value


def scan_blocks(scan, tables, requests, block_bp: int, eval_range: int = 81920) -> list:
    """The block sums of each surface request (chromosome index, centre position, half-width bp, step bp,
    ascending log alphas[, scan point index]) in blocks of ``block_bp``, on the data as loaded
    (include/fscl_amd.h): a list of Blocks in the given order."""
    req = _surface_requests(requests)
    res = BlocksT()
    _curve_check(get_lib().fscl_amd_scan_blocks(scan, tables, int(eval_range), req.ctypes.data if len(req) else None, len(req),
                                                int(block_bp), C.byref(res)), "fscl_amd_scan_blocks")
    return _blocks_take(res)


def scan_point_jackknife(scan, tables, top: int = 3, halfwidth: int = 100000, step: int = 1000,
                         alphas=(LOG_AD_MIN, LOG_AD_MAX, 33), block_bp: int = 50000, eval_range: int = 81920) -> list:
    """The block sums around the ``top`` scan points of greatest CLR, chosen and centred as scan_point_surfaces
    does: a list of Blocks in descending CLR order (jackknife_combine gives each one's delete-one estimates)."""
    res = BlocksT()
    _curve_check(get_lib().fscl_amd_scan_point_jackknife(scan, tables, int(eval_range), int(top), int(halfwidth), int(step),
                                                         float(alphas[0]), float(alphas[1]), int(alphas[2]), int(block_bp),
                                                         C.byref(res)), "fscl_amd_scan_point_jackknife")
    return _blocks_take(res)


def blocks_runs(scan, tables, runs, alphas, blocks, eval_range: int = 81920, rows=None, batch: int = 0, pts=None, bs=None,
                cnt=None):
    """fsclg_blocks_submit / fsclg_blocks_wait on the scan's first device (the shim-level handle, next to
    surface_runs): ``alphas`` holds one ascending list per run, all of one length, ``blocks`` one
    (block_bp, b0, nb) per run.  Returns (points [sum(count)], sums, counts), the latter two flat,
    position-major, then block, then alpha; ``pts`` / ``bs`` / ``cnt``: arrays to fill (tests pre-fill them)."""
    la, n, k = _run_alphas(runs, alphas)
    blk = np.zeros(max(len(runs), 1), dtype=BLOCKSPEC_DTYPE)
    for q, b in zip(blk, blocks):
        q["block_bp"], q["b0"], q["nb"] = (int(v) for v in b)
    nc = sum(max(int(r[3]), 0) * max(int(b[2]), 0) for r, b in zip(runs, blocks)) * k
    if pts is None:
        pts = np.zeros(max(n, 1), dtype=_POINT_RAW)
    if bs is None:
        bs = np.zeros(max(nc, 1), dtype=np.float64)
    if cnt is None:
        cnt = np.zeros(max(nc, 1), dtype=np.uint32)
    if pts.dtype != _POINT_RAW or len(pts) < n or bs.dtype != np.float64 or bs.size < nc or cnt.dtype != np.uint32 or \
            cnt.size < nc or not (pts.flags.c_contiguous and bs.flags.c_contiguous and cnt.flags.c_contiguous):
        raise ValueError("pts / bs / cnt must be contiguous arrays of sum(count) points and sum(count * nb) * n_la cells")
    arr, rp = _runs_rows(scan, runs, rows)
    _curve_check(get_lib().fscl_amd_blocks_runs(scan, tables, arr, len(runs), la.ctypes.data, k, blk.ctypes.data, int(eval_range),
                                                rp, int(batch), pts.ctypes.data, bs.ctypes.data, cnt.ctypes.data),
                 "fscl_amd_blocks_runs")
    return pts[:n], bs.reshape(-1)[:nc], cnt.reshape(-1)[:nc]


def jackknife_combine(bs, cnt, pos, la):
    """The delete-one-block estimates of one peak from its block sums ``bs`` / counts ``cnt`` [n_pos][nb][n_la],
    the positions' sweep_pos and the log alphas (or ``jackknife_combine(blocks)`` for a Blocks): (JACK_BLOCK_DTYPE
    records [nb], a JACK_SUMMARY_DTYPE record); the summary's ipos is -1 when every cell is NaN.  Host only.
    The estimator is an argmax on a grid: an SE of 0 means that no block moves it by one step."""
    bs = np.ascontiguousarray(bs, dtype=np.float64)
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    la = np.ascontiguousarray(la, dtype=np.float64)
    if bs.ndim != 3 or bs.shape != cnt.shape or min(bs.shape) < 1 or pos.shape != (bs.shape[0],) or la.shape != (bs.shape[2],):
        raise ValueError("bs and cnt are non-empty [n_pos][nb][n_la] arrays, with n_pos positions and n_la alphas")
    blocks = np.zeros(bs.shape[1], dtype=JACK_BLOCK_DTYPE)
    out = np.zeros(1, dtype=JACK_SUMMARY_DTYPE)
    if get_lib().fscl_amd_jackknife_combine(bs.ctypes.data, cnt.ctypes.data, bs.shape[0], bs.shape[1], bs.shape[2],
                                            pos.ctypes.data, la.ctypes.data, blocks.ctypes.data, out.ctypes.data) < 0:
        raise ValueError("jackknife_combine: bad arrays")
    return blocks, out[0]


def jackknife_output(path, scan, blocks, label=None) -> None:
    """The --jackknife-file format (include/fscl_amd.h, README): per peak one row per block with terms, then one
    summary row.  Host only."""
    n = len(blocks)
    hdr = np.zeros(max(n, 1), dtype=BLOCKS_DTYPE)
    po = co = 0
    for i, b in enumerate(blocks):
        hdr[i] = b.hdr
        if b.bs.shape != (len(b.pts), int(b.hdr["nb"]), int(b.hdr["n_la"])) or b.cnt.shape != b.bs.shape:
            raise ValueError("a peak's sums and counts must be [n_pos][nb][n_la]")
        hdr["n_pos"][i], hdr["pos_off"][i], hdr["cell_off"][i] = len(b.pts), po, co
        po += len(b.pts)
        co += b.bs.size
    pts = np.concatenate([np.ascontiguousarray(b.pts, dtype=_POINT_RAW) for b in blocks]) if n else np.zeros(0, _POINT_RAW)
    bs = np.concatenate([np.ascontiguousarray(b.bs, dtype=np.float64).reshape(-1) for b in blocks]) if n else np.zeros(0)
    cnt = np.concatenate([np.ascontiguousarray(b.cnt, dtype=np.uint32).reshape(-1) for b in blocks]) if n else np.zeros(0, np.uint32)
    res = BlocksT(n, hdr.ctypes.data, pts.ctypes.data if len(pts) else None, bs.ctypes.data if len(bs) else None,
                  cnt.ctypes.data if len(cnt) else None, len(pts), len(bs), 0)
    if get_lib().fscl_amd_jackknife_output(_b(path), scan, C.byref(res), _b(label)) != 0:
        raise ValueError(f"jackknife_output: the peaks must fit their arrays and {path} be writable")


def blocks_last_ms() -> float:
    return float(get_lib().fscl_amd_blocks_last_ms())


# fscl_amd_sweep_t: chromosome index, position, alpha (> 0)
SWEEP_DTYPE = np.dtype([("chr", "i4"), ("pos", "i4"), ("alpha", "f8")])
# fscl_amd_boot_t: one planted sweep in one replicate; est_pos -1 (and NaN est_lalpha / clr) when the
# replicate's scan has no point within the window
BOOT_DTYPE = np.dtype([("sweep", "i4"), ("rep", "i4"), ("chr", "i4"), ("planted_pos", "i4"), ("planted_alpha", "f8"),
                       ("est_pos", "i4"), ("pad", "i4"), ("est_lalpha", "f8"), ("clr", "f8")])
assert SWEEP_DTYPE.itemsize == 16 and BOOT_DTYPE.itemsize == 48


def _sweeps(sweeps) -> np.ndarray:
    a = np.zeros(len(sweeps), dtype=SWEEP_DTYPE)
    for q, r in zip(a, sweeps):
        q["chr"], q["pos"], q["alpha"] = int(r[0]), int(r[1]), float(r[2])
    return a


def parse_sweep(scan, text: str):
    """"name:pos:alpha" (the chromosome name as in the input) -> (chromosome index, pos, alpha)."""
    a = np.zeros(1, dtype=SWEEP_DTYPE)
    r = get_lib().fscl_amd_parse_sweep(scan, _b(text), a.ctypes.data)
    if r != 0:
        raise ValueError({-2: "unknown chromosome name", -3: "alpha must be positive"}.get(r, "expected chr:pos:alpha")
                         + f": {text!r}")
    return int(a[0]["chr"]), int(a[0]["pos"]), float(a[0]["alpha"])


def nearest_sweep(sweeps, chrom: int, pos: int) -> int:
    """Index of the sweep governing a site at (chromosome index, pos), -1 if its chromosome has none."""
    a = _sweeps(sweeps)
    return int(get_lib().fscl_amd_nearest_sweep(a.ctypes.data if len(a) else None, len(a), int(chrom), int(pos)))


# fscl_amd_cond_row_t: one candidate position of a conditional scan -- its sweep_pos, the global site interval it
# owns (lo > hi: none), the sites of it inside the window, the kernel point's log alpha, cond_clr, the base A,
# V at that alpha and the window null sum N
COND_ROW_DTYPE = np.dtype([("pos", "i4"), ("lo", "i4"), ("hi", "i4"), ("n_terms", "i4"), ("lalpha", "f8"), ("cond_clr", "f8"),
                           ("base", "f8"), ("v", "f8"), ("null_logl", "f8")])
# fscl_amd_cond_block_t: one (round, chromosome) -- its rows and given sweeps in the flat arrays, the row of
# greatest cond_clr (-1: none) and whether it joined the given sweeps
COND_BLOCK_DTYPE = np.dtype([("chr", "i4"), ("round", "i4"), ("n_pos", "i4"), ("n_given", "i4"), ("row_off", "u8"),
                             ("given_off", "u8"), ("max_row", "i4"), ("added", "i4")])
assert COND_ROW_DTYPE.itemsize == 56 and COND_BLOCK_DTYPE.itemsize == 40
COND_MAX_GIVEN, COND_MAX_ROUNDS = 64, 8


class CondBlock:
    """One round and chromosome of a conditional scan: ``hdr`` (a COND_BLOCK_DTYPE record), ``rows`` (COND_ROW_DTYPE, one
    per position) and ``given`` (SWEEP_DTYPE: the sweeps held fixed in this round, on this chromosome)."""

    def __init__(self, hdr, rows, given):
        self.hdr, self.rows, self.given = hdr, rows, given


def cond_clip(scan, given, chrom: int, pos: int):
    """(sweep_pos, lo, hi): the de-collided position of a candidate at ``pos`` and the global site interval it owns
    against the ``given`` sweeps (chromosome index, pos, alpha) of its chromosome; lo > hi: none.  Host only."""
    a = _sweeps(given)
    sp, lo, hi = C.c_int(), C.c_int(), C.c_int()
    if get_lib().fscl_amd_cond_clip(scan, a.ctypes.data if len(a) else None, len(a), int(chrom), int(pos), C.byref(sp),
                                    C.byref(lo), C.byref(hi)) != 0:
        raise ValueError("cond_clip: a chromosome of the scan")
    return sp.value, lo.value, hi.value


def cond_base(g, chr_start_index: int, lo: int, hi: int, window_start: int, window_end: int):
    """(A, n): the sequential sum from +0.0 of g[i - chr_start_index] over the sites i of [lo, hi] inside the window, in
    ascending order, and their count.  Host only."""
    g = np.ascontiguousarray(g, dtype=np.float64)
    a, b = max(int(lo), int(window_start)), min(int(hi), int(window_end))
    if a <= b and not (0 <= a - int(chr_start_index) and b - int(chr_start_index) < len(g)):
        raise ValueError("cond_base: the interval leaves g")
    n = C.c_int()
    v = get_lib().fscl_amd_cond_base(g.ctypes.data, int(chr_start_index), int(lo), int(hi), int(window_start), int(window_end),
                                     C.byref(n))
    return float(v), n.value


def conditional_cap() -> int:
    return int(get_lib().fscl_amd_conditional_cap())


_cond_last = {"n_terms": 0, "fold_s": 0.0}


def conditional_last_terms() -> int:
    """The device's walk terms of the last scan_conditional call."""
    return _cond_last["n_terms"]


def conditional_last_fold_s() -> float:
    """Host seconds of the base folds of the last scan_conditional call."""
    return _cond_last["fold_s"]


def scan_conditional(scan, tables, given, halfwidth: int = 0, step: int = 1000, alphas=None, rounds: int = 1,
                     min_clr: float = 0.0, eval_range: int = 81920) -> list:
    """The conditional sweep scan (include/fscl_amd.h): the likelihood ratio of one more sweep at every position
    chromosome start + k * step (within ``halfwidth`` of a given sweep when it is > 0), given the sweeps ``given``
    (chromosome index, pos, alpha) held fixed; ``alphas``: ascending log alphas (default surface_alphas()).  Returns
    a list of CondBlock, per round the chromosomes that hold a given sweep.  The given sweeps stay fixed, ownership
    goes by distance alone and the likelihood is composite: the ratio describes, it is not a calibrated test."""
    g = _sweeps(given)
    la = np.ascontiguousarray(surface_alphas() if alphas is None else alphas, dtype=np.float64).reshape(-1)
    res = ConditionalT()
    r = get_lib().fscl_amd_scan_conditional(scan, tables, int(eval_range), g.ctypes.data if len(g) else None, len(g), int(halfwidth),
                                            int(step), la.ctypes.data if len(la) else None, len(la), int(rounds), float(min_clr),
                                            C.byref(res))
    if r == -1:
        raise ValueError("scan_conditional: " + (get_lib().fscl_amd_conditional_error() or b"bad argument").decode())
    _curve_check(r, "fscl_amd_scan_conditional")
    nb, nr, ng = int(res.n_blocks), int(res.n_rows), int(res.n_given)
    blk, rows, gv = np.zeros(nb, dtype=COND_BLOCK_DTYPE), np.zeros(nr, dtype=COND_ROW_DTYPE), np.zeros(ng, dtype=SWEEP_DTYPE)
    for a, ptr, n in ((blk, res.blk, nb), (rows, res.rows, nr), (gv, res.given, ng)):
        if n:
            C.memmove(a.ctypes.data, ptr, n * a.dtype.itemsize)
    _cond_last["n_terms"], _cond_last["fold_s"] = int(res.n_terms), float(res.fold_s)
    get_lib().fscl_amd_conditional_free(C.byref(res))
    return [CondBlock(h, rows[int(h["row_off"]):int(h["row_off"]) + int(h["n_pos"])].copy(),
                      gv[int(h["given_off"]):int(h["given_off"]) + int(h["n_given"])].copy()) for h in blk]


def conditional_output(path, scan, blocks, label=None) -> None:
    """The --conditional-file format (include/fscl_amd.h, README): per block one row per position, then one summary
    row.  Host only."""
    n = len(blocks)
    blk = np.zeros(max(n, 1), dtype=COND_BLOCK_DTYPE)
    ro = go = 0
    for i, b in enumerate(blocks):
        blk[i] = b.hdr
        blk["n_pos"][i], blk["n_given"][i], blk["row_off"][i], blk["given_off"][i] = len(b.rows), len(b.given), ro, go
        ro += len(b.rows)
        go += len(b.given)
    rows = np.concatenate([np.ascontiguousarray(b.rows, dtype=COND_ROW_DTYPE) for b in blocks]) if n else np.zeros(0, COND_ROW_DTYPE)
    gv = np.concatenate([np.ascontiguousarray(b.given, dtype=SWEEP_DTYPE) for b in blocks]) if n else np.zeros(0, SWEEP_DTYPE)
    res = ConditionalT(n, blk.ctypes.data, rows.ctypes.data if len(rows) else None, gv.ctypes.data if len(gv) else None,
                       len(rows), len(gv), 0, 0.0)
    if get_lib().fscl_amd_conditional_output(_b(path), scan, C.byref(res), _b(label)) != 0:
        raise ValueError(f"conditional_output: blocks inside their arrays and {path} writable")


def cond_runs(scan, tables, runs, alphas, clip, eval_range: int = 81920, rows=None, batch: int = 0, pts=None, sm=None):
    """fsclg_cond_submit / fsclg_cond_wait on the scan's first device (the shim-level handle, as surface_runs):
    ``clip`` holds one global site-index pair (lo, hi) per position.  Returns (points [sum(count)], values
    [sum(count)][n_la])."""
    la, n, k = _run_alphas(runs, alphas)
    cl = np.ascontiguousarray(clip, dtype=np.int32).reshape(-1)
    if cl.size != 2 * n:
        raise ValueError("clip must hold one (lo, hi) pair per position")
    if pts is None:
        pts = np.zeros(max(n, 1), dtype=_POINT_RAW)
    if sm is None:
        sm = np.zeros(max(n, 1) * k, dtype=np.float64)
    if pts.dtype != _POINT_RAW or len(pts) < n or sm.dtype != np.float64 or sm.size < n * k or \
            not (pts.flags.c_contiguous and sm.flags.c_contiguous):
        raise ValueError("pts / sm must be contiguous arrays of sum(count) points and sum(count) * n_la values")
    arr, rp = _runs_rows(scan, runs, rows)
    _curve_check(get_lib().fscl_amd_cond_runs(scan, tables, arr, len(runs), la.ctypes.data, k, cl.ctypes.data if n else None,
                                              int(eval_range), rp, int(batch), pts.ctypes.data, sm.ctypes.data), "fscl_amd_cond_runs")
    return pts[:n], sm.reshape(-1)[:n * k].reshape(n, k)


def conditional_last_ms() -> float:
    return float(get_lib().fscl_amd_conditional_last_ms())


def simulate(scan, tables, sweeps=(), seed: int = 0xFD821A6, rep: int = 0):
    """One replicate under the sweep model at the scan's own sites (include/fscl_amd.h): the int32 array
    of drawn derived counts and the number of degenerate sites (which keep their observed count).
    ``sweeps``: (chromosome index, pos, alpha) each; none: a neutral replicate."""
    a = _sweeps(sweeps)
    out = np.zeros(max(scan.contents.n_snps, 1), dtype=np.int32)
    deg = C.c_ulonglong(0)
    _curve_check(get_lib().fscl_amd_simulate(scan, tables, a.ctypes.data if len(a) else None, len(a), int(seed), int(rep),
                                             out.ctypes.data, C.byref(deg)), "fscl_amd_simulate")
    return out[:scan.contents.n_snps], int(deg.value)


def simulate_scan(scan, freq):
    """A new scan_t with the scan's sites and ``freq`` as derived counts (folded at folded sites);
    scan_free releases it."""
    f = np.ascontiguousarray(freq, dtype=np.int32)
    if len(f) != scan.contents.n_snps:
        raise ValueError("one count per site")
    return get_lib().fscl_amd_simulate_scan(scan, f.ctypes.data)


def scan_free(scan) -> None:
    get_lib().fscl_amd_scan_free(scan)


def simulate_output(path, scan) -> None:
    """The scan's sites in the SNP input format (load_snp_input reads them back)."""
    if get_lib().fscl_amd_simulate_output(_b(path), scan) != 0:
        raise OSError(f"cannot write {path}")


def simulate_last_ms() -> float:
    return float(get_lib().fscl_amd_simulate_last_ms())


def bootstrap(scan, tables, fsp, sweeps, reps: int = 100, seed: int = 0xFD821A6, window_bp: int = 100000,
              eval_range: int = 81920, bp_resl: int = 128, large_grid_sp: int = 100000) -> np.ndarray:
    """The parametric bootstrap of planted sweeps (include/fscl_amd.h): a BOOT_DTYPE array of
    len(sweeps) * reps rows, row sweep * reps + rep."""
    a = _sweeps(sweeps)
    out = np.zeros(max(len(a) * int(reps), 1), dtype=BOOT_DTYPE)
    _curve_check(get_lib().fscl_amd_bootstrap(scan, tables, fsp, a.ctypes.data if len(a) else None, len(a), int(reps),
                                              int(seed), int(window_bp), int(eval_range), int(bp_resl), int(large_grid_sp),
                                              out.ctypes.data), "fscl_amd_bootstrap")
    return out[:len(a) * int(reps)]


def bootstrap_times() -> dict:
    t = (C.c_double * 5)()
    get_lib().fscl_amd_bootstrap_times(t)
    return dict(zip(("total_s", "simulate_s", "null_s", "upload_s", "scan_s"), t))


def bootstrap_output(path, scan, sweeps, reps: int, rows, label=None) -> None:
    """The --bootstrap-file format (include/fscl_amd.h): per sweep one row per replicate, then a
    quantile summary row.  Host only."""
    a = _sweeps(sweeps)
    b = np.ascontiguousarray(rows, dtype=BOOT_DTYPE)
    if len(b) != len(a) * int(reps):
        raise ValueError("rows must hold len(sweeps) * reps entries")
    get_lib().fscl_amd_bootstrap_output(_b(path), scan, a.ctypes.data if len(a) else None, len(a), int(reps),
                                        b.ctypes.data if len(b) else None, _b(label))


# fsclg_tail_t: one point's noncentral chi-square fit; flag 0 fit, 1 central (lambda = 0), 2 nofit (NaN lambda, logl,
# log10_q)
TAIL_DTYPE = np.dtype([("m", "i4"), ("m_pos", "i4"), ("mean", "f8"), ("variance", "f8"), ("lambda", "f8"), ("logl", "f8"),
                       ("log10_q", "f8"), ("flag", "i4"), ("pad", "i4")])
TAIL_FLAGS = ("fit", "central", "nofit")
TAIL_SAVE = 10000  # FSCL_AMD_TAIL_SAVE: the null CLRs a point keeps
assert TAIL_DTYPE.itemsize == 56


def _tail_df(df) -> int:
    if int(df) != df or int(df) < 2 or int(df) % 2:
        raise ValueError("df must be an even integer >= 2")
    return int(df)


def tail_records(scan) -> list:
    """The used prefix of every scan point's saved null CLRs (float32 copies, in the record's own order)."""
    s = scan.contents
    out = []
    for i in range(s.n_scan_pts):
        q = s.scan_pts[i]
        m = min(q.permute_n, TAIL_SAVE) if q.permute_clr and q.permute_n > 0 else 0
        out.append(np.ctypeslib.as_array(q.permute_clr, shape=(m,)).copy() if m else np.zeros(0, dtype=np.float32))
    return out


def tail_runs(samples, offsets, x0, df: int = 2, min_n: int = 20, counts=None) -> np.ndarray:
    """The projected-tail fit of raw records (include/fscl_amd.h): point p holds the floats
    samples[offsets[p]:offsets[p + 1]] (``offsets`` has one entry more than there are points; or give
    ``counts``) and the observed value x0[p].  Needs no scan.  A TAIL_DTYPE array."""
    df = _tail_df(df)
    smp = np.ascontiguousarray(samples, dtype=np.float32)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    x = np.ascontiguousarray(x0, dtype=np.float64)
    if counts is None:
        if len(off) != len(x) + 1:
            raise ValueError("offsets must hold one entry more than x0")
        cnt = np.ascontiguousarray(np.diff(off.astype(np.int64)), dtype=np.int32)
        off = np.ascontiguousarray(off[:-1])
    else:
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
    if len(cnt) != len(x) or len(off) != len(x):
        raise ValueError("one offset, count and x0 per point")
    out = np.zeros(max(len(x), 1), dtype=TAIL_DTYPE)
    _curve_check(get_lib().fscl_amd_tail_runs(smp.ctypes.data if len(smp) else None, len(smp), off.ctypes.data, cnt.ctypes.data,
                                              x.ctypes.data, len(x), df, int(min_n), out.ctypes.data), "fscl_amd_tail_runs")
    return out[:len(x)]


def tail_fit(scan, df: int = 2, min_n: int = 20) -> np.ndarray:
    """The projected-tail fit of every scan point after scan_permute / scan_permute_grid: a TAIL_DTYPE array
    in scan-point order."""
    df = _tail_df(df)
    t = TailT()
    _curve_check(get_lib().fscl_amd_tail_fit(scan, df, int(min_n), C.byref(t)), "fscl_amd_tail_fit")
    out = np.zeros(t.n, dtype=TAIL_DTYPE)
    if t.n:
        C.memmove(out.ctypes.data, t.pt, t.n * TAIL_DTYPE.itemsize)
    get_lib().fscl_amd_tail_free(C.byref(t))
    return out


def _tail_struct(rows, df, min_n):
    r = np.ascontiguousarray(rows, dtype=TAIL_DTYPE)
    t = TailT()
    t.n, t.df, t.min_n, t.pt = len(r), _tail_df(df), int(min_n), r.ctypes.data if len(r) else None
    return t, r


def tail_summary(scan, rows, df: int = 2, min_n: int = 20) -> dict:
    """Counts of fit / central / nofit rows and the calibration figure (median of log10 p_tail - log10
    p_empirical over the fitted points with permute_p >= 5).  Host only."""
    if len(rows) != scan.contents.n_scan_pts:
        raise ValueError("one row per scan point")
    t, keep = _tail_struct(rows, df, min_n)
    get_lib().fscl_amd_tail_summary(scan, C.byref(t))
    return {"n_fit": t.n_fit, "n_central": t.n_central, "n_nofit": t.n_nofit, "n_calibration": t.n_calibration,
            "calibration": t.calibration}


def tail_output(path, scan, rows, df: int = 2, label=None) -> None:
    """The --tail-file format (include/fscl_amd.h), one row per scan point.  Host only."""
    if len(rows) != scan.contents.n_scan_pts:
        raise ValueError("one row per scan point")
    t, keep = _tail_struct(rows, df, 0)
    if get_lib().fscl_amd_tail_output(_b(path), scan, C.byref(t), _b(label)) != 0:
        raise OSError(f"cannot write {path}")


def tail_last_ms() -> float:
    return float(get_lib().fscl_amd_tail_last_ms())


# family-wise adjusted p-values from unpruned permutation maxima (include/fscl_amd.h; maxt_kernel, include/fsclg.h)
MAXT_WG = 256            # FSCLG_MAXT_WG: threads of a trial's workgroup
MAXT_TILE = 1024         # FSCLG_MAXT_TILE: ranks of one tile of the suffix-maximum scan
MAXT_MAX_GROUPS = 4096   # FSCLG_MAXT_MAX_GROUPS


def _familywise_check(r: int, what: str) -> None:
    if r != 0:
        msg = (get_lib().fscl_amd_familywise_error() or b"").decode()
        raise (ValueError if r == -1 else RuntimeError)(f"{what} failed (code {r}): {msg}")


def familywise_order(obs) -> np.ndarray:
    """The points by observed CLR descending, ties by index ascending, a NaN last (int32).  Host only."""
    x = np.ascontiguousarray(obs, dtype=np.float64)
    out = np.zeros(len(x), dtype=np.int32)
    if len(x):
        get_lib().fscl_amd_familywise_order(x.ctypes.data, len(x), out.ctypes.data)
    return out


def familywise_chunk(n: int, trials: int, cap_bytes: int | None = None) -> int:
    """The trials of one chunk: the most whose trials * n doubles fit in cap_bytes ($FSCL_AMD_FWER_CAP, default
    2^28), at most ``trials``; 0 when one trial does not fit.  Host only."""
    L = get_lib()
    return int(L.fscl_amd_familywise_chunk(int(n), int(trials), int(L.fscl_amd_familywise_cap() if cap_bytes is None else cap_bytes)))


def familywise_runs(clr, obs, group, n_groups: int | None = None, order=None) -> dict:
    """maxt_kernel on caller arrays (fsclg_maxt_submit, in chunks under $FSCL_AMD_FWER_CAP, counts added): ``clr`` is
    [n_trials][m], ``obs`` [m], ``group`` [m] in [0, n_groups); ``order`` defaults to familywise_order(obs).  Needs
    no scan.  A dict of gmax, garg [n_trials], chr_max, chr_arg [n_trials][n_groups], c_single, c_chr, c_step [m]."""
    T = np.ascontiguousarray(clr, dtype=np.float64)
    x = np.ascontiguousarray(obs, dtype=np.float64)
    g = np.ascontiguousarray(group, dtype=np.int32)
    if T.ndim != 2 or T.shape[1] != len(x) or len(g) != len(x):
        raise ValueError("clr must be [n_trials][m], with one obs and one group per point")
    o = familywise_order(x) if order is None else np.ascontiguousarray(order, dtype=np.int32)
    if len(o) != len(x):
        raise ValueError("one rank per point")
    nt, m = T.shape
    G = int((g.max() + 1 if len(g) else 0) if n_groups is None else n_groups)
    res = {"order": o, "gmax": np.zeros(nt), "garg": np.zeros(nt, np.int32), "chr_max": np.zeros((nt, G)),
           "chr_arg": np.zeros((nt, G), np.int32), "c_single": np.zeros(m, np.int32), "c_chr": np.zeros(m, np.int32),
           "c_step": np.zeros(m, np.int32), "trials": nt}
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    _familywise_check(get_lib().fscl_amd_familywise_runs(ptr(T), nt, m, ptr(x), ptr(o), ptr(g), G, ptr(res["gmax"]), ptr(res["garg"]),
                                                         ptr(res["chr_max"]), ptr(res["chr_arg"]), ptr(res["c_single"]),
                                                         ptr(res["c_chr"]), ptr(res["c_step"])), "fscl_amd_familywise_runs")
    return res


def familywise(scan, tables, trials: int = 1000, seed: int = 0xFD821A6, permute_nbp: float = 0.1, eval_range: int = 81920,
               bp_resl: int = 128, large_grid_sp: int = 100000, scan_width_mb: float = 1.0, matrix: bool = False) -> dict:
    """The unpruned pass after scan_chromosome (include/fscl_amd.h): trial t is the throughput mode's trial t under
    ``seed``, every scan point evaluated in every trial.  A dict of order, the counts c_single, c_chr, c_step [n], the
    maxima gmax, garg [trials], chr_max, chr_arg [trials][chromosomes], trials, seed, kernel_ms, wall_s and, with
    ``matrix``, familywise_matrix: T itself, [trials][n] doubles."""
    f = FamilywiseT()
    _familywise_check(get_lib().fscl_amd_familywise(scan, tables, int(trials), int(seed), float(permute_nbp), int(eval_range),
                                                    int(bp_resl), int(large_grid_sp), float(scan_width_mb), int(bool(matrix)),
                                                    C.byref(f)), "fscl_amd_familywise")
    take = lambda p, shape, dt: (np.ctypeslib.as_array(p, shape=shape).astype(dt, copy=True)  # noqa: E731
                                 if int(np.prod(shape)) else np.zeros(shape, dt))
    n, G, M = f.n, f.n_groups, f.trials
    res = {"order": take(f.order, (n,), np.int32), "c_single": take(f.c_single, (n,), np.int32),
           "c_chr": take(f.c_chr, (n,), np.int32), "c_step": take(f.c_step, (n,), np.int32),
           "gmax": take(f.gmax, (M,), np.float64), "garg": take(f.garg, (M,), np.int32),
           "chr_max": take(f.chr_max, (M, G), np.float64), "chr_arg": take(f.chr_arg, (M, G), np.int32),
           "trials": M, "seed": int(f.seed), "kernel_ms": f.kernel_ms, "wall_s": f.wall_s}
    if matrix:
        res["familywise_matrix"] = take(f.matrix, (M, n), np.float64)
    get_lib().fscl_amd_familywise_free(C.byref(f))
    return res


def familywise_combine(c_single, c_chr, c_step, order, trials: int) -> dict:
    """rank (from 1), p_single, p_chr and the step-down p_step of every point, from the counts.  Host only."""
    cs, cc, ct = (np.ascontiguousarray(a, dtype=np.int32) for a in (c_single, c_chr, c_step))
    o = np.ascontiguousarray(order, dtype=np.int32)
    n = len(o)
    if not (len(cs) == len(cc) == len(ct) == n) or int(trials) < 1 or sorted(o.tolist()) != list(range(n)):
        raise ValueError("one count of each kind per point, order a permutation, trials >= 1")
    res = {"rank": np.zeros(n, np.int32), "p_single": np.zeros(n), "p_chr": np.zeros(n), "p_step": np.zeros(n)}
    if n:
        get_lib().fscl_amd_familywise_combine(cs.ctypes.data, cc.ctypes.data, ct.ctypes.data, o.ctypes.data, n, int(trials),
                                              res["rank"].ctypes.data, res["p_single"].ctypes.data, res["p_chr"].ctypes.data,
                                              res["p_step"].ctypes.data)
    return res


def familywise_threshold(maxima, level: float):
    """(k, threshold): k = floor(level (M + 1)) and the k-th largest of the M maxima; (0, None) when k = 0.  Host only."""
    x = np.ascontiguousarray(maxima, dtype=np.float64)
    thr = C.c_double()
    k = int(get_lib().fscl_amd_familywise_threshold(x.ctypes.data if len(x) else None, len(x), float(level), C.byref(thr)))
    return k, (thr.value if k > 0 else None)


def _familywise_struct(scan, result: dict):
    n, G = scan.contents.n_scan_pts, scan.contents.n_chromosomes
    M = int(result["trials"])
    a = {k: np.ascontiguousarray(result[k], dtype=np.int32) for k in ("order", "c_single", "c_chr", "c_step", "garg", "chr_arg")}
    a.update({k: np.ascontiguousarray(result[k], dtype=np.float64) for k in ("gmax", "chr_max")})
    if M < 1 or any(len(a[k]) != n for k in ("order", "c_single", "c_chr", "c_step")) or len(a["gmax"]) != M or \
            len(a["garg"]) != M or a["chr_max"].size != M * G or a["chr_arg"].size != M * G:
        raise ValueError("one count per scan point, one maximum per trial, one per trial and chromosome")
    f = FamilywiseT()
    f.n, f.n_groups, f.trials, f.seed = n, G, M, int(result.get("seed", 0))
    p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    for k in ("order", "c_single", "c_chr", "c_step", "garg", "chr_arg"):
        setattr(f, k, a[k].ctypes.data_as(p32))
    f.gmax, f.chr_max = a["gmax"].ctypes.data_as(p64), a["chr_max"].ctypes.data_as(p64)
    return f, a


def familywise_output(path, scan, result: dict, label=None) -> None:
    """The --familywise-file format (include/fscl_amd.h): a row per scan point, then the summary rows.  Host only."""
    f, keep = _familywise_struct(scan, result)
    if get_lib().fscl_amd_familywise_output(_b(path), scan, C.byref(f), _b(label)) != 0:
        raise OSError(f"cannot write {path}")


def familywise_null_output(path, scan, result: dict, label=None) -> None:
    """The --familywise-null-file format: a row per trial.  Host only."""
    f, keep = _familywise_struct(scan, result)
    if get_lib().fscl_amd_familywise_null_output(_b(path), scan, C.byref(f), _b(label)) != 0:
        raise OSError(f"cannot write {path}")


def familywise_last_ms() -> float:
    return float(get_lib().fscl_amd_familywise_last_ms())


def get_stats() -> dict:
    st = Stats()
    get_lib().fscl_amd_get_stats(C.byref(st))
    return st.as_dict()


def reset_stats() -> None:
    get_lib().fscl_amd_reset_stats()


def set_device(device: int) -> None:
    get_lib().fscl_amd_set_device(int(device))


def set_devices(devices=None, n: int | None = None) -> None:
    """This process drives several GPUs: ``devices`` (a list of ids) or the first ``n``;
    ``n=0`` (or nothing given): every visible GPU."""
    if devices is not None:
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        r = get_lib().fscl_amd_set_devices(arr, len(devices))
    else:
        r = get_lib().fscl_amd_set_devices(None, int(n or 0))
    if r != 0:
        raise ValueError("bad device list")


def srand(seed: int = 0xFD821A6) -> None:
    """Restart the process-wide permutation rand() stream (srand, fscl.c:135)."""
    get_lib().fscl_amd_srand(int(seed))


_dump_names = []


def set_dump_output(path=None, label=None) -> None:
    """What a SIGINT during scan_permute writes (the reference reads fscl.c's globals)."""
    b = (_b(path), _b(label))
    _dump_names.append(b)  # the C side keeps the pointers
    get_lib().fscl_amd_set_dump_output(*b)


def set_ranks_shm(rank: int, world: int, name: str) -> None:
    """Multi-process parity mode with the library's own shared-memory exchange (one node)."""
    if get_lib().fscl_amd_set_ranks_shm(int(rank), int(world), name.encode()) != 0:
        raise RuntimeError(f"fscl_amd_set_ranks_shm({rank}, {world}, {name!r}) failed")


def set_ranks(rank: int, world: int, allreduce_sum_int64=None) -> None:
    """Multi-process parity mode.  ``allreduce_sum_int64(np.ndarray[int64]) -> None``
    must sum the array in place across ranks (torch.distributed over RCCL in
    bench.py, gloo in the CPU tests)."""
    if world == 1:
        cb = EXCHANGE_FN()
    else:
        def _cb(buf, n, _ctx):
            try:
                arr = np.ctypeslib.as_array(buf, shape=(n,))
                allreduce_sum_int64(arr)
                return 0
            except Exception as e:  # noqa: BLE001 -- a failed exchange must not unwind through C
                import sys
                print(f"fscl_amd exchange failed: {e!r}", file=sys.stderr)
                return 1
        cb = EXCHANGE_FN(_cb)
    _keep.append(cb)
    if get_lib().fscl_amd_set_ranks(int(rank), int(world), cb, None) != 0:
        raise ValueError("bad rank/world")


def partition(cost, rank: int, world: int) -> tuple[int, int]:
    c = np.ascontiguousarray(cost, dtype=np.float64)
    lo, hi = C.c_int(), C.c_int()
    get_lib().fscl_amd_partition(c.ctypes.data_as(C.POINTER(C.c_double)), len(c), rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def shutdown() -> None:
    get_lib().fscl_amd_shutdown()


def run(snp_file=None, output=None, *, ms_file=None, ms_segment_length=0, ms_folded=False, n_permute=0,
        permute_nbp=0.1, asc_depth=0, asc_min_freq=1, ascbias_background_only=False, include_invariant=False,
        force_neutral=False, minimum_depth=5, large_grid_sp=100000, scan_width_mb=1.0, max_only=False,
        label=None, eval_range=81920, bp_resl=128, verbosity=1, permute_mode="parity", permute_seed=0xFD821A6,
        profile_file=None, small_grid_sp=1000, scan_mode="bisection", alpha_file=None, alpha_drop=2.0,
        sites_file=None, sites_top=10, simulate_file=None, simulate_sweeps=(), simulate_seed=0xFD821A6, simulate_rep=0,
        bootstrap_file=None, bootstrap_reps=100, bootstrap_window=None, bootstrap_sweeps=(), bootstrap_top=3,
        tail_file=None, tail_df=2, tail_min_n=20, surface_file=None, surface_top=3, surface_halfwidth=None,
        surface_step=None, surface_alphas=(LOG_AD_MIN, LOG_AD_MAX, 33), surface_drop=2.0,
        jackknife_file=None, jackknife_top=3, jackknife_block=None, jackknife_halfwidth=None, jackknife_step=None,
        jackknife_alphas=None, conditional_file=None, given_sweeps=(), conditional_halfwidth=0, conditional_step=None,
        conditional_alphas=None, conditional_rounds=1, conditional_min_clr=0.0,
        expect_file=None, expect_top=3, expect_sweeps=(), expect_alphas=None, expect_bins=24,
        familywise_file=None, familywise_trials=None, familywise_seed=None, familywise_null_file=None):
    """The fscl main() pipeline (fscl.c:316-337) in-process; returns the scan_t
    pointer (points(scan) reads the results).  permute_mode "throughput": the
    counter-based permutation test (set_permute_mode).  scan_mode "grid": the CLI's
    --scan-mode=grid (scan_chromosome_grid and scan_permute_grid at small_grid_sp)."""
    if scan_mode not in ("bisection", "grid"):
        raise ValueError("scan_mode must be bisection or grid")
    if scan_mode == "grid" and permute_mode != "parity":
        raise ValueError("scan_mode grid runs on the parity stream only")
    if int(sites_top) < 0:
        raise ValueError("sites_top must be >= 0")
    if expect_file is None and (expect_sweeps or expect_alphas is not None or expect_top != 3 or expect_bins != 24):
        raise ValueError("expect_sweeps, expect_top, expect_alphas and expect_bins need expect_file")
    # the defaults that follow other options (the CLI's check pass): the -G and -g spacings, then the surface's values
    bootstrap_window = int(large_grid_sp if bootstrap_window is None else bootstrap_window)
    surface_halfwidth = int(large_grid_sp if surface_halfwidth is None else surface_halfwidth)
    surface_step = int(small_grid_sp if surface_step is None else surface_step)
    jackknife_halfwidth = surface_halfwidth if jackknife_halfwidth is None else int(jackknife_halfwidth)
    jackknife_step = surface_step if jackknife_step is None else int(jackknife_step)
    jackknife_block = max(int(large_grid_sp) // 2, 1) if jackknife_block is None else int(jackknife_block)
    conditional_step = int(small_grid_sp if conditional_step is None else conditional_step)
    jackknife_alphas, conditional_alphas, expect_alphas = (surface_alphas if a is None else a
                                                           for a in (jackknife_alphas, conditional_alphas, expect_alphas))
    if bootstrap_file is not None and scan_mode == "grid":
        raise ValueError("the bootstrap rescans by bisection (not with scan_mode grid)")
    if bootstrap_file is not None and (int(bootstrap_reps) < 0 or int(bootstrap_top) < 0):
        raise ValueError("bootstrap_reps and bootstrap_top must be >= 0")
    if surface_file is not None:
        if int(surface_top) < 0 or not float(surface_drop) >= 0.0:
            raise ValueError("surface_top and surface_drop must be >= 0")
        if surface_step < 1:
            raise ValueError("surface_step must be at least 1")
        if surface_halfwidth < 0:
            raise ValueError("surface_halfwidth must be >= 0")
        _surface_grid(*surface_alphas)  # (raises ValueError)
    if jackknife_file is not None:
        if int(jackknife_top) < 0 or jackknife_halfwidth < 0:
            raise ValueError("jackknife_top and jackknife_halfwidth must be >= 0")
        if jackknife_step < 1 or jackknife_block < 1:
            raise ValueError("jackknife_step and jackknife_block must be at least 1")
        _surface_grid(*jackknife_alphas)  # (raises ValueError)
    if conditional_file is not None:
        if conditional_step < 1:
            raise ValueError("conditional_step must be at least 1")
        if int(conditional_halfwidth) < 0 or not 1 <= int(conditional_rounds) <= COND_MAX_ROUNDS:
            raise ValueError("conditional_halfwidth must be >= 0 and conditional_rounds 1 .. 8")
        _surface_grid(*conditional_alphas)  # (raises ValueError)
    if expect_file is not None:
        if int(expect_top) < 0 or not 1 <= int(expect_bins) <= 64:
            raise ValueError("expect_top must be >= 0 and expect_bins 1 .. 64")
        _surface_grid(*expect_alphas)  # (raises ValueError)
    if tail_file is not None:
        _tail_df(tail_df)
        if int(n_permute) <= 0:
            raise ValueError("tail_file needs the permutation test (n_permute > 0)")
        if int(tail_min_n) < 1:
            raise ValueError("tail_min_n must be >= 1")
    if familywise_file is None and (familywise_trials is not None or familywise_seed is not None or
                                    familywise_null_file is not None):
        raise ValueError("familywise_trials, familywise_seed and familywise_null_file need familywise_file")
    if familywise_file is not None:
        familywise_trials = 1000 if familywise_trials is None else int(familywise_trials)
        familywise_seed = 0xFD821A6 if familywise_seed is None else int(familywise_seed)
        if familywise_trials < 1:
            raise ValueError("familywise_trials must be at least 1")
        if scan_mode == "grid":
            raise ValueError("familywise_file evaluates the bisection scan's cells (not with scan_mode grid)")
    get_lib().configure_logmsg(int(verbosity))
    set_permute_mode(permute_mode, permute_seed)
    init_log_table()
    srand()  # init_options (fscl.c:135): a fresh process's stream
    set_dump_output(output, label)
    scan = (load_ms_input(ms_file, ms_segment_length, ms_folded) if ms_file else
            load_snp_input(snp_file, include_invariant, minimum_depth))
    fsp = background_fsp(scan, force_neutral, None, include_invariant)
    tab = compute_sweep_model_tables(scan, fsp, asc_depth, asc_min_freq, ascbias_background_only,
                                     include_invariant)
    compute_snp_null_model(scan, fsp)
    as_sweep = lambda w: parse_sweep(scan, w) if isinstance(w, str) else w  # noqa: E731 -- "name:pos:alpha" or a tuple
    sim_sw, boot_sw = [as_sweep(w) for w in simulate_sweeps], [as_sweep(w) for w in bootstrap_sweeps]
    if simulate_file is not None:  # the CLI's --simulate-file: one replicate under the model
        rep_scan = simulate_scan(scan, simulate(scan, tab, sim_sw, simulate_seed, simulate_rep)[0])
        simulate_output(simulate_file, rep_scan)
        scan_free(rep_scan)
    if scan_mode == "grid":
        scan_chromosome_grid(scan, tab, eval_range, small_grid_sp, large_grid_sp)
    else:
        scan_chromosome(scan, tab, eval_range, bp_resl, large_grid_sp)
    if profile_file is not None:  # the CLI's --profile-file: the -g spaced likelihood profile
        profile_output(profile_file, scan, scan_profile(scan, tab, eval_range, small_grid_sp, large_grid_sp), label)
    if alpha_file is not None:  # the CLI's --alpha-file: the scan points' alpha likelihood curves
        curve_output(alpha_file, scan, scan_point_curves(scan, tab, eval_range), alpha_drop, label)
    if sites_file is not None:  # the CLI's --sites-file: the per-site terms of the scan points' walks
        sites_output(sites_file, scan, *scan_point_sites(scan, tab, sites_top, eval_range), label)
    if surface_file is not None:  # the CLI's --surface-file: the surfaces around the points of greatest CLR
        surface_output(surface_file, scan,
                       scan_point_surfaces(scan, tab, surface_top, surface_halfwidth, surface_step, surface_alphas, eval_range),
                       surface_drop, label)
    if jackknife_file is not None:  # the CLI's --jackknife-file: the delete-one-block jackknife of the same points
        jackknife_output(jackknife_file, scan,
                         scan_point_jackknife(scan, tab, jackknife_top, jackknife_halfwidth, jackknife_step, jackknife_alphas,
                                              jackknife_block, eval_range), label)
    if conditional_file is not None:  # the CLI's --conditional-file: one more sweep given the fixed ones
        given = [as_sweep(w) for w in given_sweeps]
        if not given:  # the scan point of greatest CLR (the first on a tie, never a NaN) at its fitted alpha
            p = points(scan)
            given = [(int(p["chr"][i]), int(p["sweep_pos"][i]), math.exp(float(p["lalpha"][i]))) for i in top_points(scan, 1, 0)]
        conditional_output(conditional_file, scan,
                           scan_conditional(scan, tab, given, conditional_halfwidth, conditional_step,
                                            _surface_grid(*conditional_alphas), conditional_rounds, conditional_min_clr,
                                            eval_range), label)
    if expect_file is not None:  # the CLI's --expect-file: what the model expects at the sweeps
        grid = _surface_grid(*expect_alphas)
        sw = [as_sweep(w) for w in expect_sweeps]
        res = (scan_expect(scan, tab, fsp, [(c, q, math.log(a)) for c, q, a in sw], grid, expect_bins, eval_range) if sw else
               scan_point_expect(scan, tab, fsp, grid, expect_top, large_grid_sp, expect_bins, eval_range))
        expect_output(expect_file, scan, res, label)
    if n_permute > 0 and scan_mode == "grid":
        scan_permute_grid(scan, tab, n_permute, permute_nbp, eval_range, small_grid_sp, large_grid_sp, scan_width_mb)
    elif n_permute > 0:
        scan_permute(scan, tab, n_permute, permute_nbp, 1.0, 1, eval_range, bp_resl, large_grid_sp, scan_width_mb)
    if output is not None:
        scan_output(output, scan, max_only, n_permute, label)
    if tail_file is not None:  # the CLI's --tail-file: after the permutation test and the output
        tail_output(tail_file, scan, tail_fit(scan, tail_df, tail_min_n), tail_df, label)
    if familywise_file is not None:  # the CLI's --familywise-file: unpruned trials of its own, after the output
        fw = familywise(scan, tab, familywise_trials, familywise_seed, permute_nbp, eval_range, bp_resl, large_grid_sp,
                        scan_width_mb)
        familywise_output(familywise_file, scan, fw, label)
        if familywise_null_file is not None:
            familywise_null_output(familywise_null_file, scan, fw, label)
    if bootstrap_file is not None:  # the CLI's --bootstrap-file, last
        if not boot_sw:  # the scan points of greatest CLR, none within the window of one already chosen
            p = points(scan)
            boot_sw = [(int(p["chr"][i]), int(p["sweep_pos"][i]), float(np.exp(p["lalpha"][i])))
                       for i in top_points(scan, bootstrap_top, bootstrap_window, accept=_sampler_takes_alpha)]
        rows = bootstrap(scan, tab, fsp, boot_sw, bootstrap_reps, simulate_seed, bootstrap_window, eval_range, bp_resl,
                         large_grid_sp)
        bootstrap_output(bootstrap_file, scan, boot_sw, bootstrap_reps, rows, label)
    return scan
