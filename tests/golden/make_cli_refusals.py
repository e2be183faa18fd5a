#!/usr/bin/env python3
"""What the `fscl` command line answers to arguments it refuses (test infrastructure).

For each case below -- an argument vector and, for the WORLD_SIZE / RANK and *_CAP cases, an
environment -- run fscl_amd/_build/fscl and store in cli_refusals.json the exit code and, in order,
the output lines that tests/test_cli_refusals_host.py compares (cli_answer() in tests/util.py: the lines that begin
Error:, Warning:, fscl:, Fatal, Specify, Unrecognized, Option or the usage title; the temporary and
golden directories replaced by @TMP@ and @GOLD@).  None of the cases reaches a device call.

    python tests/golden/make_cli_refusals.py

The cases cover every `stop = 1` of the command line's option checks as of the commit that first
recorded the fixture (63 sites, numbered S1 .. S63 in the case names' comments), the refusals after
the data is loaded and before the device is opened (parse_sweeps, fscl_amd_conditional_check,
fscl_amd_expect_check, fscl_amd_familywise_check), several bad options at once (the order of the
lines), the lenient side of the option parsing, --help, a missing value and an unrecognised option.
Run it only to add cases: the stored answers are the contract, not what a later binary gives.
"""
from __future__ import annotations

import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from util import cli_answer as observe  # noqa: E402

T, G1 = "@TMP@", "@GOLD@/g1.snp"
BASE = ["-f", G1, "-o", f"{T}/o.txt"]
RANKS = {"WORLD_SIZE": "2", "RANK": "1"}
GRID_BAD = "-20:4:64"


def f(opt: str, name: str) -> str:
    return f"--{opt}={T}/{name}"


SUR, JK, CD, EX = f("surface-file", "s.txt"), f("jackknife-file", "j.txt"), f("conditional-file", "c.txt"), f("expect-file", "e.txt")
BOOT, SIM, TAIL, FW = f("bootstrap-file", "b.txt"), f("simulate-file", "m.txt"), f("tail-file", "t.txt"), f("familywise-file", "w.txt")

# (name, arguments after BASE -- or the whole vector where `bare` --, environment, bare)
CASES: list[tuple] = [
    # ---- the reference's checks and the scan options
    ("splines_low", ["--splines=100"], None, False),                                     # S1
    ("splines_warning_then_error", ["--splines=501", "--n-gpus=-1"], None, False),       # (warning) S16
    ("no_input", ["-o", f"{T}/o.txt"], None, True),                                      # S2
    ("both_inputs", ["-m", G1], None, False),                                            # S3
    ("no_output", ["-f", G1], None, True),                                               # S4
    ("ms_segment_length_warning", ["--ms-segment-length=1000", "--n-gpus=-1"], None, False),
    ("asc_depth_one", ["--asc-depth=1"], None, False),                                   # S5
    ("asc_depth_negative", ["-d", "-3"], None, False),                                   # S5
    ("asc_min_freq", ["-d", "4", "--asc-minimum-freq=9"], None, False),                  # S6
    ("fine_grid_zero", ["-g", "0"], None, False),                                        # S7
    ("grids_do_not_divide", ["-g", "3000", "-G", "100000"], None, False),                # S8
    ("profile_no_scan", [f("profile-file", "p.txt"), "--no-scan"], None, False),         # S9
    ("profile_fine_grid_zero", [f("profile-file", "p.txt"), "-g", "0", f("output-bs", "bs.txt")], None, False),  # S10
    ("alpha_no_scan", [f("alpha-file", "a.txt"), "--no-scan"], None, False),             # S11
    ("sites_no_scan", [f("sites-file", "i.txt"), "--no-scan"], None, False),             # S12
    ("sites_top_negative", ["--sites-top=-1"], None, False),                             # S13
    ("alpha_drop_negative", ["--alpha-drop=-1"], None, False),                           # S14
    ("alpha_drop_nan", ["--alpha-drop=nan"], None, False),                               # S14
    ("coarse_grid_zero", ["-G", "0"], None, False),                                      # S15
    ("n_gpus_negative", ["--n-gpus=-1"], None, False),                                   # S16
    ("permute_mode_unknown", ["--permute-mode=fast"], None, False),                      # S17
    ("scan_mode_unknown", ["--scan-mode=band"], None, False),                            # S18
    ("grid_with_throughput", ["--scan-mode=grid", "--permute-mode=throughput"], None, False),  # S19
    ("grid_several_ranks", ["--scan-mode=grid"], RANKS, False),                          # S20
    ("grid_fine_grid_zero", ["--scan-mode=grid", "-g", "0", f("output-bs", "bs.txt")], None, False),  # S21
    ("grid_fine_grid_zero_no_bs", ["--scan-mode=grid", "-g", "0"], None, False),         # S7 S21
    ("permute_seed_warning", ["--permute-seed=5", "--n-gpus=-1"], None, False),
    ("verbosity_zero", ["-v", "0", "--n-gpus=-1"], None, False),                         # (the Fatal line alone)
    ("verbosity_negative", ["--verbosity=-3", "--n-gpus=-1"], None, False),
    ("verbosity_one", ["-v", "1", "--n-gpus=-1", "--permute-seed=5"], None, False),      # (errors, no warnings)
    # ---- simulation and bootstrap
    ("bootstrap_no_scan", [BOOT, "--no-scan"], None, False),                             # S22
    ("bootstrap_grid", [BOOT, "--scan-mode=grid"], None, False),                         # S23
    ("bootstrap_several_ranks", [BOOT], RANKS, False),                                   # S24
    ("bootstrap_reps_negative", [BOOT, "--bootstrap-reps=-1"], None, False),             # S25
    ("bootstrap_top_negative", [BOOT, "--bootstrap-top=-1"], None, False),               # S26
    ("bootstrap_sweep_alpha_zero", [BOOT, "--bootstrap-sweep=anything:5000:0"], None, False),        # S27
    ("simulate_sweep_alpha_negative", [SIM, "--simulate-sweep=anything:5000:-2e-4"], None, False),   # S27
    ("simulate_then_bootstrap_sweeps", [SIM, BOOT, "--bootstrap-sweep=b:1:0", "--simulate-sweep=a:1:0", "--simulate-sweep=c:1:x"],
     None, False),                                                                       # S27 (simulate's first)
    # ---- tail
    ("tail_df_odd", [TAIL, "--n-permute=5", "--tail-df=3"], None, False),                # S28
    ("tail_df_zero", [TAIL, "--n-permute=5", "--tail-df=0"], None, False),               # S28
    ("tail_df_too_large", [TAIL, "--n-permute=5", "--tail-df=1000002"], None, False),    # S28
    ("tail_df_fraction", [TAIL, "--n-permute=5", "--tail-df=2.5"], None, False),         # S28
    ("tail_df_word", [TAIL, "--n-permute=5", "--tail-df=four"], None, False),            # S28
    ("tail_df_empty", [TAIL, "--n-permute=5", "--tail-df="], None, False),               # S28
    ("tail_df_without_file", ["--tail-df=3"], None, False),                              # S28
    ("tail_no_permutations", [TAIL], None, False),                                       # S29
    ("tail_no_scan", [TAIL, "-p", "5", "--no-scan"], None, False),                       # S30
    ("tail_several_ranks", [TAIL, "--n-permute=5"], RANKS, False),                       # S31
    ("tail_min_n_zero", [TAIL, "--n-permute=5", "--tail-min-n=0"], None, False),         # S32
    # ---- family-wise
    ("familywise_trials_without_file", ["--familywise-trials=10"], None, False),         # S33
    ("familywise_seed_without_file", ["--familywise-seed=5"], None, False),              # S33
    ("familywise_null_without_file", [f("familywise-null-file", "n.txt")], None, False),  # S33
    ("familywise_trials_zero", [FW, "--familywise-trials=0"], None, False),              # S34
    ("familywise_trials_word", [FW, "--familywise-trials=ten"], None, False),            # S34
    ("familywise_trials_too_many", [FW, "--familywise-trials=100000001"], None, False),  # S34
    ("familywise_trials_bad_without_file", ["--familywise-trials=2.5"], None, False),    # S33 S34
    ("familywise_no_scan", [FW, "--no-scan"], None, False),                              # S35
    ("familywise_grid", [FW, "--scan-mode=grid", "-g", "5000"], None, False),            # S36
    ("familywise_several_ranks", [FW], {"WORLD_SIZE": "4", "RANK": "0"}, False),         # S37
    # ---- surface
    ("surface_no_scan", [SUR, "--no-scan"], None, False),                                # S38
    ("surface_top_negative", ["--surface-top=-1"], None, False),                         # S39
    ("surface_halfwidth_negative", [SUR, "--surface-halfwidth=-5"], None, False),        # S40 S61 (no --jackknife-halfwidth)
    ("surface_step_zero", [SUR, "--surface-step=0"], None, False),                       # S41 S62
    ("surface_step_zero_jackknife_step_given", [SUR, "--surface-step=0", "--jackknife-step=7"], None, False),  # S41
    ("surface_drop_negative", [SUR, "--surface-drop=-0.5"], None, False),                # S42
    ("surface_alphas_count", [SUR, f"--surface-alphas={GRID_BAD}"], None, False),        # S43
    ("surface_alphas_low", [SUR, "--surface-alphas=-21:4:10"], None, False),             # S43
    ("surface_alphas_trailing", [SUR, "--surface-alphas=-20:4:10x"], None, False),       # S43
    ("surface_alphas_short", ["--surface-alphas=-20:4"], None, False),                   # S43
    ("fine_grid_zero_without_surface_file", ["-g", "0", f("output-bs", "bs.txt"), JK], None, False),  # S62 (the default chain)
    # ---- conditional
    ("conditional_no_scan", [CD, "--no-scan"], None, False),                             # S44
    ("given_sweep_without_file", ["--given-sweep=chr1:1000:1e-3"], None, False),         # S45
    ("conditional_step_without_file", ["--conditional-step=500"], None, False),          # S45
    ("conditional_halfwidth_without_file", ["--conditional-halfwidth=0"], None, False),  # S45
    ("conditional_rounds_without_file", ["--conditional-rounds=1"], None, False),        # S45
    ("conditional_min_clr_without_file", ["--conditional-min-clr=0"], None, False),      # S45
    ("conditional_alphas_without_file", ["--conditional-alphas=-20:4:7"], None, False),  # S45
    ("conditional_step_zero", [CD, "--conditional-step=0"], None, False),                # S46
    ("conditional_step_trailing", [CD, "--conditional-step=7x"], None, False),           # S46
    ("conditional_step_from_fine_grid", [CD, "-g", "0", f("output-bs", "bs.txt")], None, False),  # S46 (the default chain)
    ("conditional_halfwidth_negative", [CD, "--conditional-halfwidth=-5"], None, False),  # S47
    ("conditional_halfwidth_word", [CD, "--conditional-halfwidth=wide"], None, False),   # S47
    ("conditional_rounds_zero", [CD, "--conditional-rounds=0"], None, False),            # S48
    ("conditional_rounds_nine", [CD, "--conditional-rounds=9"], None, False),            # S48
    ("conditional_rounds_huge", [CD, "--conditional-rounds=99999999999999999999"], None, False),  # S48
    ("conditional_min_clr_nan", [CD, "--conditional-min-clr=nan"], None, False),         # S49
    ("conditional_min_clr_word", [CD, "--conditional-min-clr=1.5x"], None, False),       # S49
    ("conditional_alphas_count", [CD, f"--conditional-alphas={GRID_BAD}"], None, False),  # S50
    ("given_sweep_alpha_zero", [CD, "--given-sweep=chr1:1000:0"], None, False),          # S51
    ("given_sweep_alpha_large", [CD, "--given-sweep=chr1:1000:1e9"], None, False),       # S51
    ("given_sweep_no_colon", [CD, "--given-sweep=chr1"], None, False),                   # S51
    # ---- expect
    ("expect_top_without_file", ["--expect-top=2"], None, False),                        # S52
    ("expect_bins_without_file", ["--expect-bins=12"], None, False),                     # S52
    ("expect_alphas_without_file", ["--expect-alphas=-20:4:9"], None, False),            # S52
    ("expect_sweep_without_file", ["--expect-sweep=chr1:5000:1e-4"], None, False),       # S52
    ("expect_no_scan", [EX, "--no-scan"], None, False),                                  # S53
    ("expect_top_negative", [EX, "--expect-top=-1"], None, False),                       # S54
    ("expect_top_word", [EX, "--expect-top=x"], None, False),                            # S54
    ("expect_bins_zero", [EX, "--expect-bins=0"], None, False),                          # S55
    ("expect_bins_65", [EX, "--expect-bins=65"], None, False),                           # S55
    ("expect_alphas_count", [EX, f"--expect-alphas={GRID_BAD}"], None, False),           # S56
    ("expect_alphas_descending", [EX, "--expect-alphas=2:1:10"], None, False),           # S56
    ("expect_sweep_alpha_zero", [EX, "--expect-sweep=chr1:5000:0"], None, False),        # S57
    ("expect_sweep_alpha_small", [EX, "--expect-sweep=chr1:5000:1e-10"], None, False),   # S57
    ("expect_sweep_no_alpha", [EX, "--expect-sweep=chr1:5000"], None, False),            # S57
    # ---- jackknife
    ("jackknife_no_scan", [JK, "--no-scan"], None, False),                               # S58
    ("jackknife_top_negative", ["--jackknife-top=-1"], None, False),                     # S59
    ("jackknife_block_zero", [JK, "--jackknife-block=0"], None, False),                  # S60
    ("jackknife_block_from_coarse_grid", [JK, "-G", "0"], None, False),                  # S15 (block: max(G/2, 1), accepted)
    ("jackknife_halfwidth_negative", [JK, "--jackknife-halfwidth=-5"], None, False),     # S61
    ("jackknife_step_zero", [JK, "--jackknife-step=0"], None, False),                    # S62
    ("jackknife_alphas_count", [JK, f"--jackknife-alphas={GRID_BAD}"], None, False),     # S63
    ("jackknife_alphas_equal_ends", [JK, "--jackknife-alphas=1:1:2"], None, False),      # S63
    # ---- several bad options at once: the order of the lines
    ("many_surface_jackknife_conditional_expect",
     [SUR, JK, CD, EX, "--expect-bins=0", "--jackknife-alphas=a:b:c", "--conditional-rounds=9", "--surface-step=0",
      "--jackknife-block=0", "--expect-alphas=5:6:7", "--given-sweep=chr1:5:0", "--surface-alphas=0:5:10", "--expect-sweep=chr1",
      "--conditional-alphas=-20:4:0", "--surface-drop=-1", "--jackknife-top=-2", "--conditional-min-clr=", "--expect-top=-4",
      "--surface-top=-3", "--conditional-halfwidth=-1", "--conditional-step=0"], None, False),
    ("many_surface_halfwidth_alone", [SUR, JK, "--surface-halfwidth=-7", "--jackknife-block=-3", "--surface-top=-1"], None, False),
    ("many_scan_options", ["--splines=3", "-d", "1", "-g", "7", "--sites-top=-2", "--alpha-drop=-2", "-G", "-5", "--n-gpus=-2",
                           "--permute-mode=x", "--scan-mode=y", "--ms-segment-length=5", "--permute-seed=1"], None, False),
    ("many_one_process", [BOOT, TAIL, FW, "--scan-mode=grid", "--tail-df=5", "--familywise-trials=-1", "--bootstrap-reps=-2",
                          "--tail-min-n=0", "--no-scan"], {"WORLD_SIZE": "3", "RANK": "2"}, False),
    ("many_no_scan", [f("profile-file", "p.txt"), f("alpha-file", "a.txt"), f("sites-file", "i.txt"), SUR, JK, CD, EX, BOOT, TAIL, FW,
                      "--no-scan"], None, False),
    ("many_need_their_file", ["--familywise-seed=1", "--conditional-rounds=0", "--expect-bins=99", "--given-sweep=x"], None, False),
    ("world_size_one_is_one_process", [BOOT, "--scan-mode=grid"], {"WORLD_SIZE": "1", "RANK": "0"}, False),  # S23 alone
    ("world_size_without_rank", [BOOT, "--n-gpus=-1"], {"WORLD_SIZE": "2"}, False),      # S16 alone
    # ---- the lenient side, and the argument loop
    ("lenient_sites_top_word", ["--sites-top=abc", "--no-scan"], None, False),           # 0: accepted
    ("lenient_surface_step_minus_one", ["--surface-step=-1", "--no-scan"], None, False),  # not given: accepted
    ("lenient_surface_halfwidth_minus_one", ["--surface-halfwidth=-1", "--jackknife-halfwidth=-1", "--jackknife-step=-1",
                                             "--jackknife-block=-1", "--bootstrap-window=-9", "--no-scan"], None, False),
    ("lenient_surface_step_minus_two", ["--surface-step=-2"], None, False),              # S41 S62
    ("help", ["--help"], None, True),
    ("help_after_options", ["--n-gpus=-1", "--help"], None, False),
    ("no_arguments", [], None, True),
    ("missing_value_long", ["--sites-top"], None, False),
    ("missing_value_long_with_space", ["--snpfile", G1], None, True),
    ("missing_value_short", ["-g"], None, False),
    ("unrecognised_option", ["--no-such-option=3", "--n-gpus=-1", "-Z"], None, False),
    ("flag_given_twice", ["--no-scan", f("alpha-file", "a.txt"), "--no-scan", "--n-gpus=-1"], None, False),  # (toggles: S16 alone)
    # ---- once the data is loaded, before the device is opened
    ("unknown_chromosome_simulate", [SIM, "--no-scan", "--simulate-sweep=no_such_chromosome:5000:1e-4"], None, False),
    ("unknown_chromosome_simulate_without_file", ["--simulate-sweep=no_such_chromosome:5000:1e-4"], None, False),
    ("unknown_chromosome_bootstrap", [BOOT, "--bootstrap-sweep=no_such_chromosome:5000:1e-4"], None, False),
    ("unknown_chromosome_given", [CD, "--given-sweep=no-such-chromosome:1000:1e-3"], None, False),
    ("unknown_chromosome_expect", [EX, "--no-scan", "--expect-sweep=no-such-chromosome:5000:1e-4"], None, False),
    ("sweep_without_colons", [SIM, "--no-scan", "--simulate-sweep=chr1"], None, False),
    ("sweep_order_simulate_first", [SIM, BOOT, CD, EX, "--expect-sweep=q:1:1e-3", "--given-sweep=q:1:1e-3", "--bootstrap-sweep=q:1:1e-3",
                                    "--simulate-sweep=chr1:1:1e-3", "--simulate-sweep=q:1:1e-3"], None, False),
    ("conditional_check_cap", [CD, "--given-sweep=chr1:1000:1e-3"], {"FSCL_AMD_COND_CAP": "100"}, False),
    ("conditional_check_65_given", [CD] + [f"--given-sweep=chr1:{1000 + i}:1e-3" for i in range(65)], None, False),
    ("conditional_check_before_expect_sweeps", [CD, EX, "--given-sweep=chr1:1000:1e-3", "--expect-sweep=q:1:1e-3"],
     {"FSCL_AMD_COND_CAP": "100"}, False),
    ("expect_check_position", [EX, "--expect-sweep=chr1:2147483600:1e-4"], None, False),
    ("expect_check_cap", [EX, "--expect-sweep=chr1:5000:1e-4"], {"FSCL_AMD_EXPECT_CAP": "100"}, False),
    ("familywise_check_cap", [FW], {"FSCL_AMD_FWER_CAP": "239"}, False),                 # g1 has 30 cells: 240 bytes a trial
    ("expect_check_before_familywise_check", [EX, FW, "--expect-sweep=chr1:2147483600:1e-4"], {"FSCL_AMD_FWER_CAP": "239"}, False),
]


def main() -> int:
    out = []
    names = set()
    for name, args, env, bare in CASES:
        assert name not in names, name
        names.add(name)
        case = {"name": name, "args": list(args) if bare else BASE + list(args), "env": env or {}}
        with tempfile.TemporaryDirectory() as d:
            case["exit"], case["lines"] = observe(case, Path(d))
        out.append(case)
        print(f"{name}: exit {case['exit']}, {len(case['lines'])} lines")
    (HERE / "cli_refusals.json").write_text(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
