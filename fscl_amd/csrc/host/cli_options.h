/* cli_options.h -- the `fscl` command line's options (cli_options.c): one record of every option's
 * value, the argument loop that fills it and the pass that checks it and resolves its defaults.
 * Nothing here looks at a scan or a device; it links against surface.c and util.c alone. */
#ifndef FSCL_CLI_OPTIONS_H
#define FSCL_CLI_OPTIONS_H

#include "fscl_host.h"

typedef struct { char **v; int n; } strlist_t; /* an option that may be given several times */
typedef struct { double lo, hi; int n; } alpha_grid_t; /* LO:HI:N, natural-log alpha */

/* "not given" is NULL for a string (the _s options are parsed by the check pass) and -1 for the
   ints whose default follows another option */
typedef struct {
  /* the reference's options (fscl.c:38-102, defaults :127-178); the library reads spline_pts, n_permute,
     output_fname and prepend_label from its globals of these names, which main() sets from here */
  char *snp_fname, *ms_fname, *bs_fname, *output_bs_fname, *output_fname, *prepend_label;
  int force_neutral, ms_segment_length, ms_folded, ms_sample_first, ms_sample_size;
  int asc_depth, asc_min_freq, bg_only, include_invariant, maximum_only;
  int small_grid_sp, large_grid_sp, dont_scan, minimum_obs_depth, n_threads, verbosity, spline_pts, n_permute;
  double permute_nbp, alpha_factor, scan_width_mb;
  /* the device, the scan and permutation modes */
  int n_gpus;
  char *permute_mode, *permute_seed, *scan_mode;
  int grid_mode, throughput; /* (resolved: --scan-mode=grid, --permute-mode=throughput) */
  /* one output file each */
  char *profile_fname;
  char *alpha_fname;
  double alpha_drop;
  char *sites_fname;
  int sites_top;
  char *simulate_fname, *simulate_seed;
  strlist_t simulate_sweep;
  int simulate_rep;
  char *bootstrap_fname;
  strlist_t bootstrap_sweep;
  int bootstrap_reps, bootstrap_window, bootstrap_top;
  char *tail_fname, *tail_df_s;
  int tail_df, tail_min_n;
  char *fw_fname, *fw_trials_s, *fw_seed_s, *fw_null_fname;
  int fw_trials;
  char *surface_fname, *surface_alphas;
  int surface_top, surface_halfwidth, surface_step;
  double surface_drop;
  alpha_grid_t surface_grid;
  char *jackknife_fname, *jackknife_alphas;
  int jackknife_top, jackknife_block, jackknife_halfwidth, jackknife_step;
  alpha_grid_t jackknife_grid;
  char *cond_fname, *cond_alphas, *cond_halfwidth_s, *cond_step_s, *cond_rounds_s, *cond_min_clr_s;
  strlist_t given_sweep;
  int cond_halfwidth, cond_step, cond_rounds;
  double cond_min_clr;
  alpha_grid_t cond_grid;
  char *expect_fname, *expect_alphas, *expect_top_s, *expect_bins_s;
  strlist_t expect_sweep;
  int expect_top, expect_bins;
  alpha_grid_t expect_grid;
} cli_opts_t;

/* the defaults, then argv ("--long=value" or "-x value", flags toggle): -1 to go on, else main()'s exit code */
int cli_parse(int argc, char **argv, cli_opts_t *o);
void cli_opts_free(cli_opts_t *o); /* (the strings cli_parse copied, for a caller that parses more than once; main() keeps them) */
/* every refusal that needs the options alone, in a fixed order, and the defaults that follow other
   options; 1 where something was refused */
int cli_check(cli_opts_t *o);
/* $WORLD_SIZE where a launcher runs several ranks of this job (with $RANK set), else NULL */
const char *cli_multi_rank(void);
/* this process writes the analysis files: the only rank, or rank 0 */
int cli_rank0(void);

#endif
