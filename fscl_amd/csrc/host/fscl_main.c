/* fscl_main.c -- the `fscl` command line, drop-in for the reference's
 * (option table fscl.c:38-102, defaults :127-178, validation :180-258,
 * main :272-341, parsing cmdline-utils.c:28-100: "--long=value" or
 * "-x value", flags toggle).  The scan path runs on the GPU.
 *
 * Deliberate differences: "--long value" without '=' is an
 * error instead of a NULL dereference; -m reads ms output with defined
 * semantics (all blocks form one genome, one chromosome per block, --max-only
 * prints the maximum of each block); -b reads the format --output-bs writes.
 */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "fscl_host.h"

enum { T_STR, T_INT, T_DBL, T_FLAG, T_LIST };
typedef struct { char **v; int n; } strlist_t; /* T_LIST: an option that may be given several times */
typedef struct { char s; const char *l; void *v; int t; const char *doc; } opt_t;

/* fscl.c:33-34 */
char *prepend_label, *output_fname;
int spline_pts, n_permute;

static void usage(const opt_t *o) {
  fprintf(stderr, "fscl (MI355X) -- composite-likelihood selective sweep scan\n");
  for (; o->v; o++) {
    if (o->s) fprintf(stderr, "  -%c, --%-28s %s\n", o->s, o->l, o->doc);
    else fprintf(stderr, "      --%-28s %s\n", o->l, o->doc);
  }
}

static void list_add(strlist_t *l, const char *arg) {
  l->v = realloc(l->v, sizeof(char *) * (size_t)(l->n + 1));
  if (!l->v) { fprintf(stderr, "out of memory (options)\n"); exit(1); }
  l->v[l->n++] = strdup(arg);
}

/* a whole decimal integer within the int range: 1 and *out, else 0 */
static int int_option(const char *t, int *out) {
  char *end = NULL;
  long v;
  errno = 0;
  v = strtol(t, &end, 10);
  if (end == t || *end || errno || v < -2147483647L || v > 2147483647L) return 0;
  *out = (int)v;
  return 1;
}

/* "chr:pos:alpha" options into sweeps; a bad one is fatal before anything runs on the device */
static fscl_amd_sweep_t *parse_sweeps(const scan_t *s, const strlist_t *l, const char *opt) {
  fscl_amd_sweep_t *sw = malloc(sizeof *sw * (size_t)(l->n ? l->n : 1));
  int i;
  if (!sw) logmsg(MSG_FATAL, "fscl: out of memory (sweeps)");
  for (i = 0; i < l->n; i++) {
    const int r = fscl_amd_parse_sweep(s, l->v[i], sw + i);
    if (r == -2) logmsg(MSG_FATAL, "fscl: --%s=%s: unknown chromosome name", opt, l->v[i]);
    if (r == -3) logmsg(MSG_FATAL, "fscl: --%s=%s: alpha must be positive", opt, l->v[i]);
    if (r != 0) logmsg(MSG_FATAL, "fscl: --%s=%s: expected chr:pos:alpha", opt, l->v[i]);
  }
  return sw;
}

/* the --bootstrap-top scan points: descending CLR (ties in scan order, a NaN never), at their fitted
   sweep_pos and alpha, skipping a point within window_bp of one already chosen on its chromosome */
static int sampler_takes_alpha(const scan_pt_t *p) { /* (positive and finite: else the sampler refuses) */
  const double alpha = exp(p->lalpha);
  return alpha > 0.0 && !(alpha > 1.7976931348623157e308);
}

static fscl_amd_sweep_t *top_sweeps(const scan_t *s, int top, int window_bp, int *n_out) {
  fscl_amd_sweep_t *sw = malloc(sizeof *sw * (size_t)(top > 0 ? top : 1));
  int *point = malloc(sizeof *point * (size_t)(top > 0 ? top : 1));
  int n, k;
  if (!sw || !point) logmsg(MSG_FATAL, "fscl: out of memory (sweeps)");
  n = fscl_amd_top_points(s, top, window_bp, sampler_takes_alpha, point);
  for (k = 0; k < n; k++) {
    const scan_pt_t *p = s->scan_pts + point[k];
    sw[k].chr = p->chr; sw[k].pos = p->sweep_pos; sw[k].alpha = exp(p->lalpha);
  }
  free(point);
  *n_out = n > 0 ? n : 0;
  return sw;
}

/* --max-only for ms input: one line per block (fscl.c:68-69, :307-308) */
static void output_block_maxima(const char *fname, scan_t *s, const char *label) {
  FILE *f = fname ? fopen(fname, "w") : stdout;
  int c, i;
  if (!f) { fprintf(stderr, "Can't open output file \"%s\"\n", fname); return; }
  for (c = 0; c < s->n_chromosomes; c++) {
    const scan_pt_t *b = NULL;
    for (i = 0; i < s->n_scan_pts; i++)
      if (s->scan_pts[i].chr == c && (!b || s->scan_pts[i].clr > b->clr)) b = s->scan_pts + i;
    if (!b) continue;
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\t%1.2f\t%1.3e\t%d\t%d\t%d\n", s->chr_limits[c].name, b->sweep_pos, b->clr, exp(b->lalpha),
            b->n_snps, s->snps[b->window_start].pos, s->snps[b->window_end].pos);
  }
  if (fname) fclose(f);
}

int main(int argc, char **argv) {
  char *snp_fname = NULL, *ms_fname = NULL, *bs_fname = NULL, *output_bs_fname = NULL;
  int force_neutral = 0, ms_segment_length = 0, ms_folded = 0, ms_sample_first = 0, ms_sample_size = 0;
  int asc_depth = 0, asc_min_freq = 1, bg_only = 0, include_invariant = 0, maximum_only = 0;
  int small_grid_sp = 1000, large_grid_sp = 100000, dont_scan = 0, minimum_obs_depth = 5, n_threads = 1;
  int verbosity = MSG_STATUS, eval_range = 81920, bp_resl = 128, stop = 0, i, n_gpus = 0;
  double permute_nbp = 0.1, alpha_factor = 1.0, scan_width_mb = 1.0;
  char *permute_mode = NULL, *permute_seed = NULL, *profile_fname = NULL, *scan_mode = NULL, *alpha_fname = NULL;
  double alpha_drop = 2.0;
  char *sites_fname = NULL;
  int sites_top = 10;
  int grid_mode = 0;
  char *simulate_fname = NULL, *simulate_seed = NULL, *bootstrap_fname = NULL;
  strlist_t simulate_sweep = {NULL, 0}, bootstrap_sweep = {NULL, 0};
  int simulate_rep = 0, bootstrap_reps = 100, bootstrap_window = -1, bootstrap_top = 3, need_tables;
  char *tail_fname = NULL, *tail_df_str = NULL;
  char *surface_fname = NULL, *surface_alphas = NULL;
  int surface_top = 3, surface_halfwidth = -1, surface_step = -1, surface_n = 33;
  double surface_drop = 2.0, surface_lo = LOG_AD_MIN, surface_hi = LOG_AD_MAX;
  char *jackknife_fname = NULL, *jackknife_alphas = NULL;
  char *cond_fname = NULL, *cond_alphas = NULL;
  strlist_t given_sweep = {NULL, 0};
  char *cond_halfwidth_s = NULL, *cond_step_s = NULL, *cond_rounds_s = NULL, *cond_min_clr_s = NULL; /* (NULL: not given) */
  int cond_halfwidth = 0, cond_step = 1, cond_rounds = 1, cond_n = -1;
  double cond_min_clr = 0.0, cond_lo = LOG_AD_MIN, cond_hi = LOG_AD_MAX;
  int jackknife_top = 3, jackknife_block = -1, jackknife_halfwidth = -1, jackknife_step = -1, jackknife_n = 33;
  double jackknife_lo = LOG_AD_MIN, jackknife_hi = LOG_AD_MAX;
  int tail_df = 2, tail_min_n = 20;
  char *fw_fname = NULL, *fw_trials_s = NULL, *fw_seed_s = NULL, *fw_null_fname = NULL; /* (NULL: not given) */
  int fw_trials = 1000;
  char *expect_fname = NULL, *expect_alphas = NULL, *expect_top_s = NULL, *expect_bins_s = NULL; /* (NULL: not given) */
  strlist_t expect_sweep = {NULL, 0};
  int expect_top = 3, expect_bins = 24, expect_n = -1;
  double expect_lo = LOG_AD_MIN, expect_hi = LOG_AD_MAX;
  scan_t *s;
  double **fsp;
  opt_t opts[] = {
      {'f', "snpfile", &snp_fname, T_STR, "File name of file with SNP frequency data"},
      {'d', "asc-depth", &asc_depth, T_INT, "Depth of SNP ascertainment sample"},
      {0, "asc-minimum-freq", &asc_min_freq, T_INT, "minimum number of observations of both alleles for SNP ascertainment"},
      {'p', "n-permute", &n_permute, T_INT, "number of snp block permutations for p-value computations"},
      {0, "permute-nbp", &permute_nbp, T_DBL, "probability for switching to a new snp block for permutations"},
      {0, "n-threads", &n_threads, T_INT, "accepted for compatibility (the GPU evaluates all points at once)"},
      {'a', "alpha-factor", &alpha_factor, T_DBL, "multiply 1/alpha by this factor to determine single sweep window size"},
      {'g', "fine-grid-spacing", &small_grid_sp, T_INT, "Spacing in bp of the CLR profile's positions (--profile-file); must divide -G"},
      {'G', "coarse-grid-spacing", &large_grid_sp, T_INT, "Size of coarse grid in which CLR maxima will be selected"},
      {'w', "sweep-width", &scan_width_mb, T_DBL, "maximum width of sweep effect in scanning, in Mb"},
      {0, "minimum-depth", &minimum_obs_depth, T_INT, "minimum depth of sample (lower depth SNPs ignored)"},
      {'m', "msfile", &ms_fname, T_STR, "Name of an ms output file"},
      {0, "ms-segment-length", &ms_segment_length, T_INT, "Length in bp of simulated ms segments (use with -m option only)"},
      {0, "ms-folded", &ms_folded, T_FLAG, "For ms input, treat all sites as folded"},
      {0, "max-only", &maximum_only, T_FLAG, "for ms input, output only the maximum CLR for each input block"},
      {0, "ms-sample-first", &ms_sample_first, T_INT, "index of first chromosome in ms sample to analyze"},
      {0, "ms-sample-size", &ms_sample_size, T_INT, "number of consecutive chromosomes in ms output to take as the sample"},
      {0, "force-neutral-spectrum", &force_neutral, T_FLAG, "Do not estimate background spectrum from the data. Use sum(1/i)/i"},
      {'b', "background-spectrum", &bs_fname, T_STR, "Load the background frequency spectrum from a file"},
      {0, "output-bs", &output_bs_fname, T_STR, "write estimated background site-frequency spectra to file"},
      {0, "include-invariant", &include_invariant, T_FLAG, "Include invariant sites in analysis (default is to ignore them)"},
      {0, "splines", &spline_pts, T_INT, "Number of knot points to approximate sweep model w/ respect to alpha"},
      {0, "prepend-label", &prepend_label, T_STR, "optional token to prepend to each line of the sweep scan output"},
      {'v', "verbosity", &verbosity, T_INT, "verbosity level 0-5, default 3, debug 4 and above"},
      {'o', "output-file", &output_fname, T_STR, "output file for scan results"},
      {0, "no-scan", &dont_scan, T_FLAG, "do not scan chromosome, compute background frequency spectrum only"},
      {0, "ascbias-background-only", &bg_only, T_FLAG, "correct for ascertainment bias only in estimating the background site frequency spectrum"},
      {0, "n-gpus", &n_gpus, T_INT, "GPUs to use (default: every visible GPU, or $FSCL_AMD_DEVICE alone when set)"},
      {0, "permute-mode", &permute_mode, T_STR, "parity (default: the reference's rand() stream, identical results) or "
                                                "throughput (counter-based random numbers, trials independent; not identical)"},
      {0, "profile-file", &profile_fname, T_STR, "write CLR and alpha at every -g spaced position (the likelihood profile) to this file"},
      {0, "alpha-file", &alpha_fname, T_STR, "write every scan point's alpha likelihood curve and support interval to this file"},
      {0, "alpha-drop", &alpha_drop, T_DBL, "log-likelihood drop of the support interval in --alpha-file (default 2.0; descriptive: "
                                            "the likelihood is composite)"},
      {0, "sites-file", &sites_fname, T_STR, "write the per-site likelihood terms of the scan points' walks, and a footprint summary per "
                                             "point, to this file"},
      {0, "sites-top", &sites_top, T_INT, "--sites-file takes this many points of greatest CLR (default 10; 0: every point)"},
      {0, "scan-mode", &scan_mode, T_STR, "bisection (default: search_maxpos in every cell) or grid (the maximum over each cell's "
                                          "-g spaced positions, in the scan and in the permutation test; one process, parity only)"},
      {0, "permute-seed", &permute_seed, T_STR, "seed of the throughput mode's random numbers (default 0xFD821A6)"},
      {0, "simulate-file", &simulate_fname, T_STR, "write one replicate of the data simulated under the sweep model (SNP input format) "
                                                   "to this file; needs no scan"},
      {0, "simulate-sweep", &simulate_sweep, T_LIST, "chr:pos:alpha of a sweep planted in --simulate-file (may be given several times; "
                                                     "none: a neutral replicate)"},
      {0, "simulate-seed", &simulate_seed, T_STR, "seed of the simulation and the bootstrap (default 0xFD821A6)"},
      {0, "simulate-rep", &simulate_rep, T_INT, "replicate number of --simulate-file (default 0)"},
      {0, "bootstrap-file", &bootstrap_fname, T_STR, "parametric bootstrap: simulate under the planted sweeps, rescan, write every "
                                                     "replicate's estimate and a quantile summary per sweep to this file"},
      {0, "bootstrap-reps", &bootstrap_reps, T_INT, "replicates of --bootstrap-file (default 100)"},
      {0, "bootstrap-window", &bootstrap_window, T_INT, "a replicate's estimate is its best scan point within this many bp of the planted "
                                                        "position (default: the -G spacing)"},
      {0, "bootstrap-sweep", &bootstrap_sweep, T_LIST, "chr:pos:alpha of a sweep to bootstrap (may be given several times; none: the "
                                                       "--bootstrap-top scan points)"},
      {0, "bootstrap-top", &bootstrap_top, T_INT, "without --bootstrap-sweep, bootstrap this many scan points of greatest CLR (default 3)"},
      {0, "tail-file", &tail_fname, T_STR, "after the permutation test, write every scan point's p-value projected from a noncentral "
                                           "chi-square fit of its null CLRs (below 1/n-permute) to this file"},
      {0, "tail-df", &tail_df_str, T_STR, "degrees of freedom of the --tail-file fit: an even integer >= 2 (default 2)"},
      {0, "surface-file", &surface_fname, T_STR, "write the position-by-alpha likelihood surface around the scan points of greatest "
                                                 "CLR, and a region summary per point, to this file"},
      {0, "surface-top", &surface_top, T_INT, "--surface-file takes this many points of greatest CLR (default 3)"},
      {0, "surface-halfwidth", &surface_halfwidth, T_INT, "half-width in bp of a surface's positions around its point (default: the -G spacing)"},
      {0, "surface-step", &surface_step, T_INT, "spacing in bp of a surface's positions (default: the -g spacing; at least 1)"},
      {0, "surface-alphas", &surface_alphas, T_STR, "LO:HI:N, the surface's alpha grid: natural-log alpha endpoints within [-20, 4] and a "
                                                    "count N <= 63 (default -20:4:33, steps of 0.75); the point's fitted alpha is added"},
      {0, "surface-drop", &surface_drop, T_DBL, "log-likelihood drop of the region in --surface-file (default 2.0, as --alpha-drop; a joint "
                                                "two-parameter 95 % region under the chi-square reading would be about 3.0; descriptive: "
                                                "the likelihood is composite)"},
      {0, "conditional-file", &cond_fname, T_STR, "write the conditional sweep scan -- the likelihood ratio of one more sweep at every "
                                                  "grid position, given the --given-sweep sweeps held fixed -- to this file"},
      {0, "given-sweep", &given_sweep, T_LIST, "chr:pos:alpha of a sweep held fixed in --conditional-file (may be given several times; "
                                               "default: the scan point of greatest CLR at its fitted alpha)"},
      {0, "conditional-halfwidth", &cond_halfwidth_s, T_STR, "evaluate only the positions within this many bp of a given sweep "
                                                           "(default 0: the whole chromosome)"},
      {0, "conditional-step", &cond_step_s, T_STR, "spacing in bp of the --conditional-file positions (default: the -g spacing; at least 1)"},
      {0, "conditional-alphas", &cond_alphas, T_STR, "LO:HI:N, the candidate's alpha grid (default: the --surface-alphas value)"},
      {0, "conditional-rounds", &cond_rounds_s, T_STR, "forward selection: after a round each chromosome's position of greatest conditional "
                                                     "CLR joins the given sweeps (1 .. 8, default 1)"},
      {0, "conditional-min-clr", &cond_min_clr_s, T_STR, "a round's maximum joins the given sweeps only above this conditional CLR (default 0)"},
      {0, "jackknife-file", &jackknife_fname, T_STR, "write a delete-one-block jackknife of the scan points of greatest CLR (the "
                                                     "re-maximised position, alpha and CLR with each genomic block left out, and their "
                                                     "standard errors) to this file"},
      {0, "jackknife-top", &jackknife_top, T_INT, "--jackknife-file takes this many points of greatest CLR (default 3)"},
      {0, "jackknife-block", &jackknife_block, T_INT, "block length in bp of the jackknife (default: half the -G spacing; at least 1)"},
      {0, "jackknife-halfwidth", &jackknife_halfwidth, T_INT, "half-width in bp of the jackknife's positions (default: --surface-halfwidth)"},
      {0, "jackknife-step", &jackknife_step, T_INT, "spacing in bp of the jackknife's positions (default: --surface-step)"},
      {0, "jackknife-alphas", &jackknife_alphas, T_STR, "LO:HI:N, the jackknife's alpha grid (default: --surface-alphas)"},
      {0, "expect-file", &expect_fname, T_STR, "write what the fitted model expects at the sweeps of greatest CLR -- the expectation and SD of "
                                               "the CLR under the sweep and under neutrality, per bin of log(alpha d), along an alpha "
                                               "list, and in all -- to this file"},
      {0, "expect-top", &expect_top_s, T_STR, "--expect-file takes this many points of greatest CLR (default 3)"},
      {0, "expect-sweep", &expect_sweep, T_LIST, "chr:pos:alpha of a sweep for --expect-file (may be given several times; replaces the "
                                                 "--expect-top choice)"},
      {0, "expect-alphas", &expect_alphas, T_STR, "LO:HI:N, the alpha list of --expect-file's curve rows (default: the --surface-alphas "
                                                  "value); the sweep's own alpha is added"},
      {0, "expect-bins", &expect_bins_s, T_STR, "equal-width bins of log(alpha d) over [-20, 4] in --expect-file (1 .. 64, default 24)"},
      {0, "tail-min-n", &tail_min_n, T_INT, "--tail-file fits a point with at least this many positive null CLRs (default 20)"},
      {0, "familywise-file", &fw_fname, T_STR, "after the permutation test and the output, write every scan point's family-wise adjusted "
                                               "p-values (Westfall-Young maxT over unpruned permutation trials: single-step, per "
                                               "chromosome and step-down) and the genome-wide CLR thresholds to this file"},
      {0, "familywise-trials", &fw_trials_s, T_STR, "unpruned trials of --familywise-file, each a full scan (default 1000; at least 1)"},
      {0, "familywise-seed", &fw_seed_s, T_STR, "seed of the --familywise-file permutations, those of the throughput mode under this "
                                                "seed (default 0xFD821A6)"},
      {0, "familywise-null-file", &fw_null_fname, T_STR, "write every --familywise-file trial's genome and chromosome maxima to this file"},
      {0, NULL, NULL, 0, NULL}};

  spline_pts = N_SPLINE_KNOTS;
  n_permute = 0;
  init_log_table();
  if (argc == 1) { usage(opts); return 255; }
  for (i = 1; i < argc;) {
    const char *a = argv[i], *arg;
    char name[256];
    int lng, j;
    if (a[0] != '-') { i++; continue; }
    if (a[1] == '-') {
      const char *eq = strchr(a + 2, '=');
      size_t ln = eq ? (size_t)(eq - (a + 2)) : strlen(a + 2);
      if (ln >= sizeof name) ln = sizeof name - 1;
      memcpy(name, a + 2, ln);
      name[ln] = 0;
      arg = eq ? eq + 1 : NULL;
      lng = 1;
    } else {
      name[0] = a[1];
      name[1] = 0;
      arg = i + 1 < argc ? argv[i + 1] : NULL;
      lng = 0;
    }
    if (lng && !strcmp(name, "help")) { usage(opts); return 0; }
    for (j = 0; opts[j].v; j++)
      if (lng ? strcmp(name, opts[j].l) == 0 : opts[j].s == name[0]) break;
    if (!opts[j].v) fprintf(stderr, "Unrecognized option \"%s\"\n", a);
    else if (opts[j].t == T_FLAG) *(int *)opts[j].v ^= 1;
    else if (!arg) { fprintf(stderr, "Option \"%s\" needs a value (--%s=value or -x value)\n", a, opts[j].l); return 255; }
    else if (opts[j].t == T_STR) *(char **)opts[j].v = strdup(arg);
    else if (opts[j].t == T_LIST) list_add((strlist_t *)opts[j].v, arg);
    else if (opts[j].t == T_INT) *(int *)opts[j].v = atoi(arg);
    else *(double *)opts[j].v = atof(arg);
    i += (lng || (opts[j].v && opts[j].t == T_FLAG)) ? 1 : 2;
  }

  /* fscl.c:180-258 */
  if (verbosity < 0) verbosity = 0;
  configure_logmsg(verbosity);
  if (bg_only) logmsg(MSG_STATUS, "ascertainment bias correction to background site frequency spectrum only\n");
  if (minimum_obs_depth < 5) minimum_obs_depth = 5;
  if (spline_pts < N_SPLINE_KNOTS) {
    logmsg(MSG_ERROR, "Error: must use at least %d spline functions to approximate sweep model\nlikelihood function.\n",
           N_SPLINE_KNOTS);
    stop = 1;
  }
  if (spline_pts > 500)
    logmsg(MSG_WARN, "Warning: estimating %d spline functions will significantly inflate execution\ntime with little "
                     "gain in accuracy...\n", spline_pts);
  if (!snp_fname && !ms_fname) {
    logmsg(MSG_ERROR, "Error: input snp frequency file or ms file not specified. Use -f option or -m option.\n");
    stop = 1;
  }
  if (snp_fname && ms_fname) { logmsg(MSG_ERROR, "Specify either a snp frequency file or an ms file, not both.\n"); stop = 1; }
  if (!output_fname) { logmsg(MSG_ERROR, "Specify an output file name with -o option\n"); stop = 1; }
  if (ms_segment_length && !ms_fname) {
    logmsg(MSG_WARN, "Warning: --ms-segment-length option ignored if -m option is not used.\n");
    ms_segment_length = 0;
  }
  if (asc_depth == 1 || asc_depth < 0) {
    logmsg(MSG_ERROR, "Error: if specified, ascertainment sample depth must be at least 2.\n");
    stop = 1;
  }
  if (asc_depth >= 2 && asc_min_freq > 2 * asc_depth) {
    logmsg(MSG_ERROR, "Error: SNP ascertainment is impossible with asc. sample depth and asc. minimum allele "
                      "frequency setting\n");
    stop = 1;
  }
  if (asc_depth >= 2 && asc_min_freq == 0) asc_min_freq = 1;
  if (small_grid_sp < 1 && !output_bs_fname) {
    logmsg(MSG_ERROR, "Error: specify sweep position grid spacing with -g option (in bp).\n");
    stop = 1;
  }
  if ((profile_fname || !output_bs_fname) && small_grid_sp > 0 && large_grid_sp > 0 && large_grid_sp % small_grid_sp != 0) {
    logmsg(MSG_ERROR, "Error: fine grid spacing must evenly divide coarse grid spacing.\n");
    stop = 1;
  }
  if (profile_fname && dont_scan) { logmsg(MSG_ERROR, "Error: --profile-file needs the scan (not with --no-scan).\n"); stop = 1; }
  if (profile_fname && small_grid_sp < 1) { logmsg(MSG_ERROR, "Error: --profile-file needs a positive -g spacing.\n"); stop = 1; }
  if (alpha_fname && dont_scan) { logmsg(MSG_ERROR, "Error: --alpha-file needs the scan (not with --no-scan).\n"); stop = 1; }
  if (sites_fname && dont_scan) { logmsg(MSG_ERROR, "Error: --sites-file needs the scan (not with --no-scan).\n"); stop = 1; }
  if (sites_top < 0) { logmsg(MSG_ERROR, "Error: --sites-top must be >= 0.\n"); stop = 1; }
  if (!(alpha_drop >= 0.0)) { logmsg(MSG_ERROR, "Error: --alpha-drop must be >= 0.\n"); stop = 1; }
  if (large_grid_sp < 1) { logmsg(MSG_ERROR, "Error: coarse grid spacing must be positive.\n"); stop = 1; }
  if (n_gpus < 0) { logmsg(MSG_ERROR, "Error: --n-gpus must be >= 0.\n"); stop = 1; }
  if (permute_mode && strcmp(permute_mode, "parity") && strcmp(permute_mode, "throughput")) {
    logmsg(MSG_ERROR, "Error: --permute-mode must be parity or throughput.\n");
    stop = 1;
  }
  if (scan_mode && strcmp(scan_mode, "bisection") && strcmp(scan_mode, "grid")) {
    logmsg(MSG_ERROR, "Error: --scan-mode must be bisection or grid.\n");
    stop = 1;
  }
  grid_mode = scan_mode && !strcmp(scan_mode, "grid");
  if (grid_mode && permute_mode && !strcmp(permute_mode, "throughput")) {
    logmsg(MSG_ERROR, "Error: --scan-mode=grid runs on the parity stream only (not with --permute-mode=throughput).\n");
    stop = 1;
  }
  if (grid_mode && getenv("WORLD_SIZE") && getenv("RANK") && atoi(getenv("WORLD_SIZE")) > 1) {
    logmsg(MSG_ERROR, "Error: --scan-mode=grid runs in one process (not with WORLD_SIZE=%s ranks).\n", getenv("WORLD_SIZE"));
    stop = 1;
  }
  if (grid_mode && small_grid_sp < 1) { logmsg(MSG_ERROR, "Error: --scan-mode=grid needs a positive -g spacing.\n"); stop = 1; }
  if (bootstrap_fname && dont_scan && bootstrap_sweep.n == 0) {
    logmsg(MSG_ERROR, "Error: --bootstrap-file with --no-scan needs --bootstrap-sweep (no scan points to take).\n");
    stop = 1;
  }
  if (bootstrap_fname && grid_mode) { logmsg(MSG_ERROR, "Error: --bootstrap-file rescans by bisection (not with --scan-mode=grid).\n"); stop = 1; }
  if (bootstrap_fname && getenv("WORLD_SIZE") && getenv("RANK") && atoi(getenv("WORLD_SIZE")) > 1) {
    logmsg(MSG_ERROR, "Error: --bootstrap-file runs in one process (not with WORLD_SIZE=%s ranks).\n", getenv("WORLD_SIZE"));
    stop = 1;
  }
  if (bootstrap_fname && bootstrap_reps < 0) { logmsg(MSG_ERROR, "Error: --bootstrap-reps must be >= 0.\n"); stop = 1; }
  if (bootstrap_fname && bootstrap_top < 0) { logmsg(MSG_ERROR, "Error: --bootstrap-top must be >= 0.\n"); stop = 1; }
  if (bootstrap_window < 0) bootstrap_window = large_grid_sp;
  for (i = 0; i < simulate_sweep.n + bootstrap_sweep.n; i++) { /* (the chromosome names are checked once the data is loaded) */
    const char *t = i < simulate_sweep.n ? simulate_sweep.v[i] : bootstrap_sweep.v[i - simulate_sweep.n];
    const char *c = strrchr(t, ':');
    if (c && !(atof(c + 1) > 0.0)) {
      logmsg(MSG_ERROR, "Error: --%s-sweep=%s: alpha must be positive.\n", i < simulate_sweep.n ? "simulate" : "bootstrap", t);
      stop = 1;
    }
  }
  if (tail_df_str) {
    char *end;
    const long v = strtol(tail_df_str, &end, 10);
    if (end == tail_df_str || *end || v < 2 || v > 1000000 || (v & 1)) {
      logmsg(MSG_ERROR, "Error: --tail-df must be an even integer >= 2 (not \"%s\").\n", tail_df_str);
      stop = 1;
    } else tail_df = (int)v;
  }
  if (tail_fname && n_permute <= 0) { logmsg(MSG_ERROR, "Error: --tail-file needs the permutation test (--n-permute > 0).\n"); stop = 1; }
  if (tail_fname && dont_scan) { logmsg(MSG_ERROR, "Error: --tail-file needs the scan (not with --no-scan).\n"); stop = 1; }
  if (tail_fname && getenv("WORLD_SIZE") && getenv("RANK") && atoi(getenv("WORLD_SIZE")) > 1) {
    logmsg(MSG_ERROR, "Error: --tail-file runs in one process (not with WORLD_SIZE=%s ranks).\n", getenv("WORLD_SIZE"));
    stop = 1;
  }
  if (tail_fname && tail_min_n < 1) { logmsg(MSG_ERROR, "Error: --tail-min-n must be >= 1.\n"); stop = 1; }
  if (!fw_fname && (fw_trials_s || fw_seed_s || fw_null_fname)) {
    logmsg(MSG_ERROR, "Error: --familywise-trials, --familywise-seed and --familywise-null-file need --familywise-file.\n");
    stop = 1;
  }
  if (fw_trials_s) {
    char *end;
    const long v = strtol(fw_trials_s, &end, 10);
    if (end == fw_trials_s || *end || v < 1 || v > 100000000) {
      logmsg(MSG_ERROR, "Error: --familywise-trials must be an integer >= 1 (not \"%s\").\n", fw_trials_s);
      stop = 1;
    } else fw_trials = (int)v;
  }
  if (fw_fname && dont_scan) { logmsg(MSG_ERROR, "Error: --familywise-file needs the scan (not with --no-scan).\n"); stop = 1; }
  if (fw_fname && grid_mode) {
    logmsg(MSG_ERROR, "Error: --familywise-file evaluates the bisection scan's cells (not with --scan-mode=grid).\n");
    stop = 1;
  }
  if (fw_fname && getenv("WORLD_SIZE") && getenv("RANK") && atoi(getenv("WORLD_SIZE")) > 1) {
    logmsg(MSG_ERROR, "Error: --familywise-file runs in one process (not with WORLD_SIZE=%s ranks).\n", getenv("WORLD_SIZE"));
    stop = 1;
  }
  if (surface_fname && dont_scan) { logmsg(MSG_ERROR, "Error: --surface-file needs the scan (not with --no-scan).\n"); stop = 1; }
  if (surface_top < 0) { logmsg(MSG_ERROR, "Error: --surface-top must be >= 0.\n"); stop = 1; }
  if (surface_halfwidth < 0) surface_halfwidth = surface_halfwidth == -1 ? large_grid_sp : -2;
  if (surface_halfwidth == -2) { logmsg(MSG_ERROR, "Error: --surface-halfwidth must be >= 0.\n"); stop = 1; }
  if (jackknife_step == -1) jackknife_step = surface_step == -1 ? small_grid_sp : surface_step; /* --surface-step, given or default */
  if (surface_step == -1) surface_step = surface_fname ? small_grid_sp : 1;
  if (surface_step < 1) { logmsg(MSG_ERROR, "Error: --surface-step must be at least 1.\n"); stop = 1; }
  if (!(surface_drop >= 0.0)) { logmsg(MSG_ERROR, "Error: --surface-drop must be >= 0.\n"); stop = 1; }
  if (surface_alphas) {
    char tail_c = 0;
    double probe[FSCL_AMD_SURFACE_MAX_LA];
    if (sscanf(surface_alphas, "%lf:%lf:%d%c", &surface_lo, &surface_hi, &surface_n, &tail_c) != 3 ||
        fscl_amd_surface_alphas(surface_lo, surface_hi, surface_n, NAN, probe) < 1) {
      logmsg(MSG_ERROR, "Error: --surface-alphas must be LO:HI:N with -20 <= LO <= HI <= 4 (natural-log alpha), 1 <= N <= 63, "
                        "and LO < HI unless N is 1 (not \"%s\").\n", surface_alphas);
      stop = 1;
    }
  }
  if (cond_fname && dont_scan && given_sweep.n == 0) {
    logmsg(MSG_ERROR, "Error: --conditional-file with --no-scan needs explicit --given-sweep sweeps.\n");
    stop = 1;
  }
  if (!cond_fname && (given_sweep.n || cond_halfwidth_s || cond_step_s || cond_rounds_s || cond_min_clr_s || cond_alphas)) {
    logmsg(MSG_ERROR, "Error: --given-sweep and the --conditional-* options need --conditional-file.\n");
    stop = 1;
  }
  cond_step = small_grid_sp;
  if (cond_step_s && !int_option(cond_step_s, &cond_step)) cond_step = 0;
  if (cond_fname && cond_step < 1) { logmsg(MSG_ERROR, "Error: --conditional-step must be at least 1.\n"); stop = 1; }
  if (cond_halfwidth_s && !int_option(cond_halfwidth_s, &cond_halfwidth)) cond_halfwidth = -1;
  if (cond_halfwidth < 0) { logmsg(MSG_ERROR, "Error: --conditional-halfwidth must be >= 0.\n"); stop = 1; }
  if (cond_rounds_s && !int_option(cond_rounds_s, &cond_rounds)) cond_rounds = 0;
  if (cond_rounds < 1 || cond_rounds > FSCL_AMD_COND_MAX_ROUNDS) { logmsg(MSG_ERROR, "Error: --conditional-rounds must be 1 .. 8.\n"); stop = 1; }
  if (cond_min_clr_s) {
    char *end = NULL;
    cond_min_clr = strtod(cond_min_clr_s, &end);
    if (end == cond_min_clr_s || *end || !(cond_min_clr == cond_min_clr)) { logmsg(MSG_ERROR, "Error: --conditional-min-clr must be a number.\n"); stop = 1; }
  }
  if (cond_alphas) {
    char tail_c = 0;
    double probe[FSCL_AMD_SURFACE_MAX_LA];
    if (sscanf(cond_alphas, "%lf:%lf:%d%c", &cond_lo, &cond_hi, &cond_n, &tail_c) != 3 ||
        fscl_amd_surface_alphas(cond_lo, cond_hi, cond_n, NAN, probe) < 1) {
      logmsg(MSG_ERROR, "Error: --conditional-alphas must be LO:HI:N with -20 <= LO <= HI <= 4 (natural-log alpha), 1 <= N <= 63, "
                        "and LO < HI unless N is 1 (not \"%s\").\n", cond_alphas);
      stop = 1;
    }
  }
  for (i = 0; i < given_sweep.n; i++) { /* (the chromosome names are checked once the data is loaded, before the scan) */
    const char *t = given_sweep.v[i], *c2 = strrchr(t, ':');
    const double a = c2 ? atof(c2 + 1) : 0.0;
    if (!c2 || !(a > 0.0) || !(log(a) >= LOG_AD_MIN && log(a) <= LOG_AD_MAX)) {
      logmsg(MSG_ERROR, "Error: --given-sweep=%s: expected chr:pos:alpha, alpha positive with its natural log within [-20, 4].\n", t);
      stop = 1;
    }
  }
  if (!expect_fname && (expect_sweep.n || expect_alphas || expect_top_s || expect_bins_s)) {
    logmsg(MSG_ERROR, "Error: --expect-sweep, --expect-top, --expect-alphas and --expect-bins need --expect-file.\n");
    stop = 1;
  }
  if (expect_fname && dont_scan && expect_sweep.n == 0) {
    logmsg(MSG_ERROR, "Error: --expect-file with --no-scan needs explicit --expect-sweep sweeps.\n");
    stop = 1;
  }
  if (expect_top_s && (!int_option(expect_top_s, &expect_top) || expect_top < 0)) { logmsg(MSG_ERROR, "Error: --expect-top must be >= 0.\n"); stop = 1; }
  if (expect_bins_s && (!int_option(expect_bins_s, &expect_bins) || expect_bins < 1 || expect_bins > FSCL_AMD_EXPECT_MAX_BINS)) {
    logmsg(MSG_ERROR, "Error: --expect-bins must be 1 .. 64.\n");
    stop = 1;
  }
  if (expect_alphas) {
    char tail_c = 0;
    double probe[FSCL_AMD_SURFACE_MAX_LA];
    if (sscanf(expect_alphas, "%lf:%lf:%d%c", &expect_lo, &expect_hi, &expect_n, &tail_c) != 3 ||
        fscl_amd_surface_alphas(expect_lo, expect_hi, expect_n, NAN, probe) < 1) {
      logmsg(MSG_ERROR, "Error: --expect-alphas must be LO:HI:N with -20 <= LO <= HI <= 4 (natural-log alpha), 1 <= N <= 63, "
                        "and LO < HI unless N is 1 (not \"%s\").\n", expect_alphas);
      stop = 1;
    }
  }
  for (i = 0; i < expect_sweep.n; i++) { /* (the chromosome names are checked once the data is loaded, before the scan) */
    const char *t = expect_sweep.v[i], *c2 = strrchr(t, ':');
    const double a = c2 ? atof(c2 + 1) : 0.0;
    if (!c2 || !(a > 0.0) || !(log(a) >= LOG_AD_MIN && log(a) <= LOG_AD_MAX)) {
      logmsg(MSG_ERROR, "Error: --expect-sweep=%s: expected chr:pos:alpha, alpha positive with its natural log within [-20, 4].\n", t);
      stop = 1;
    }
  }
  if (jackknife_fname && dont_scan) { logmsg(MSG_ERROR, "Error: --jackknife-file needs the scan (not with --no-scan).\n"); stop = 1; }
  if (jackknife_top < 0) { logmsg(MSG_ERROR, "Error: --jackknife-top must be >= 0.\n"); stop = 1; }
  if (jackknife_block == -1) jackknife_block = large_grid_sp / 2 > 1 ? large_grid_sp / 2 : 1;
  if (jackknife_block < 1) { logmsg(MSG_ERROR, "Error: --jackknife-block must be at least 1.\n"); stop = 1; }
  if (jackknife_halfwidth == -1) jackknife_halfwidth = surface_halfwidth;
  if (jackknife_halfwidth < 0) { logmsg(MSG_ERROR, "Error: --jackknife-halfwidth must be >= 0.\n"); stop = 1; }
  if (jackknife_step < 1) { logmsg(MSG_ERROR, "Error: --jackknife-step must be at least 1.\n"); stop = 1; }
  if (jackknife_alphas) {
    char tail_c = 0;
    double probe[FSCL_AMD_SURFACE_MAX_LA];
    if (sscanf(jackknife_alphas, "%lf:%lf:%d%c", &jackknife_lo, &jackknife_hi, &jackknife_n, &tail_c) != 3 ||
        fscl_amd_surface_alphas(jackknife_lo, jackknife_hi, jackknife_n, NAN, probe) < 1) {
      logmsg(MSG_ERROR, "Error: --jackknife-alphas must be LO:HI:N with -20 <= LO <= HI <= 4 (natural-log alpha), 1 <= N <= 63, "
                        "and LO < HI unless N is 1 (not \"%s\").\n", jackknife_alphas);
      stop = 1;
    }
  } else {
    jackknife_lo = surface_lo; jackknife_hi = surface_hi; jackknife_n = surface_n;
  }
  if (permute_seed && !(permute_mode && !strcmp(permute_mode, "throughput")))
    logmsg(MSG_WARN, "Warning: --permute-seed is used only with --permute-mode=throughput.\n");
  if (stop) {
    if (verbosity <= MSG_FATAL) logmsg(MSG_FATAL, "Fatal errors have occurred, use -v 1 or greater to see them.\n");
    exit(-1);
  }

  s = ms_fname ? fh_load_ms(ms_fname, ms_segment_length, ms_folded, ms_sample_first, ms_sample_size)
               : load_snp_input(snp_fname, include_invariant, minimum_obs_depth);
  fsp = background_fsp(s, force_neutral, bs_fname, include_invariant);
  if (output_bs_fname) output_background_fs(output_bs_fname, s, fsp);
  if (!cond_alphas) { cond_lo = surface_lo; cond_hi = surface_hi; cond_n = surface_n; }
  if (!expect_alphas) { expect_lo = surface_lo; expect_hi = surface_hi; expect_n = surface_n; }
  need_tables = !dont_scan || simulate_fname || bootstrap_fname || cond_fname || expect_fname;
  if (need_tables) {
    sm_ptable_t *sm;
    const unsigned long long sim_seed = simulate_seed ? strtoull(simulate_seed, NULL, 0) : 0xFD821A6ull;
    fscl_amd_sweep_t *sim_sw = parse_sweeps(s, &simulate_sweep, "simulate-sweep");
    fscl_amd_sweep_t *boot_sw = parse_sweeps(s, &bootstrap_sweep, "bootstrap-sweep");
    /* the given sweeps and every host-only refusal of the conditional scan, on every rank, before any device work */
    fscl_amd_sweep_t *given_sw = parse_sweeps(s, &given_sweep, "given-sweep");
    double cond_la[FSCL_AMD_SURFACE_MAX_LA];
    const int cond_n_la = cond_fname ? fscl_amd_surface_alphas(cond_lo, cond_hi, cond_n, NAN, cond_la) : 0;
    if (cond_fname && fscl_amd_conditional_check(s, given_sw, given_sweep.n, cond_halfwidth, cond_step, cond_la, cond_n_la, cond_rounds,
                                                 cond_min_clr) != 0)
      logmsg(MSG_FATAL, "fscl: %s", fscl_amd_conditional_error());
    /* the expect sweeps and every host-only refusal of --expect-file, on every rank, before any device work */
    fscl_amd_sweep_t *expect_sw = parse_sweeps(s, &expect_sweep, "expect-sweep");
    fsclg_site_req_t *expect_req = malloc(sizeof *expect_req * (size_t)(expect_sweep.n > 0 ? expect_sweep.n : 1));
    double expect_la[FSCL_AMD_SURFACE_MAX_LA];
    const int expect_n_la = expect_fname ? fscl_amd_surface_alphas(expect_lo, expect_hi, expect_n, NAN, expect_la) : 0;
    int n_boot = bootstrap_sweep.n;
    const char *ws = getenv("WORLD_SIZE"), *rk = getenv("RANK");
    if (!expect_req) logmsg(MSG_FATAL, "fscl: out of memory (expect sweeps)");
    for (i = 0; i < expect_sweep.n; i++) {
      expect_req[i].chr = expect_sw[i].chr; expect_req[i].pos = expect_sw[i].pos; expect_req[i].lalpha = log(expect_sw[i].alpha);
    }
    if (expect_fname && fscl_amd_expect_check(s, expect_req, expect_sweep.n, expect_la, expect_n_la, expect_bins) != 0)
      logmsg(MSG_FATAL, "fscl: %s", fscl_amd_expect_error());
    /* every host-only refusal of --familywise-file, before any device work */
    if (fw_fname && fscl_amd_familywise_check(s, large_grid_sp, fw_trials) != 0)
      logmsg(MSG_FATAL, "fscl: --familywise-file: %s", fscl_amd_familywise_error());
    if (ws && rk && atoi(ws) > 1) {
      /* one process per GPU (e.g. under torch.distributed.run): GPU $LOCAL_RANK (or
         $FSCL_AMD_DEVICE), results exchanged through a shared-memory segment named by
         $FSCL_AMD_SHM_NAME, else the launcher's run id or port; rank 0 writes the output */
      const char *id = getenv("FSCL_AMD_SHM_NAME"), *run = getenv("TORCHELASTIC_RUN_ID"), *port = getenv("MASTER_PORT"),
                 *addr = getenv("MASTER_ADDR"), *sj = getenv("SLURM_JOB_ID"), *ss = getenv("SLURM_STEP_ID");
      char name[200];
      if (id) snprintf(name, sizeof name, "/fscl_amd_%s", id);
      else if (port || (run && strcmp(run, "none")) || sj)
        /* values a launcher gives every rank of one job alike, and two concurrent jobs on a node
           not: the rendezvous port (torch.distributed.run, mpirun wrappers), the launcher's run id
           (plain torchrun sets "none"), the Slurm job and step -- not the parent's pid, which
           differs between ranks started through a per-rank wrapper (a shell script, srun) */
        snprintf(name, sizeof name, "/fscl_amd_%s_%s_%s_%s_%s", run && strcmp(run, "none") ? run : "job",
                 addr ? addr : "-", port ? port : "0", sj ? sj : "-", ss ? ss : "-");
      else /* no launcher variables: the ranks of one launch are assumed to share their parent */
        snprintf(name, sizeof name, "/fscl_amd_job_%ld", (long)getppid());
      if (n_gpus > 1) logmsg(MSG_WARN, "Warning: --n-gpus is ignored with one process per GPU (WORLD_SIZE=%s).\n", ws);
      if (fscl_amd_set_ranks_shm(atoi(rk), atoi(ws), name) != 0)
        logmsg(MSG_FATAL, "fscl: rank %s of %s could not meet the other ranks (%s)", rk, ws, name);
    } else if ((n_gpus > 0 || !getenv("FSCL_AMD_DEVICE")) && fscl_amd_set_devices(NULL, n_gpus) != 0)
      logmsg(MSG_FATAL, "fscl: --n-gpus=%d: at most 16 GPUs per process", n_gpus);
    if (permute_mode && !strcmp(permute_mode, "throughput")) {
      fscl_amd_set_permute_mode(FSCL_AMD_PERMUTE_THROUGHPUT, permute_seed ? strtoull(permute_seed, NULL, 0) : 0xFD821A6ull);
      logmsg(MSG_STATUS, "permutation test in throughput mode (counter-based random numbers; not the reference's stream)\n");
    }
    sm = compute_sweep_model_tables(s, fsp, asc_depth, asc_min_freq, bg_only, include_invariant);
    compute_snp_null_model(s, fsp);
    if (simulate_fname && !(ws && rk && atoi(ws) > 1 && atoi(rk) != 0)) {
      /* one replicate under the model, at the data's own sites (rank 0 alone); no rand() draw */
      int *freq = malloc(sizeof(int) * (size_t)(s->n_snps > 0 ? s->n_snps : 1));
      unsigned long long n_deg = 0;
      scan_t *q;
      int r;
      if (!freq) logmsg(MSG_FATAL, "fscl: out of memory (simulation)");
      r = fscl_amd_simulate(s, sm, sim_sw, simulate_sweep.n, sim_seed, simulate_rep, freq, &n_deg);
      if (r != 0) logmsg(MSG_FATAL, "fscl: simulation failed (code %d)", r);
      q = fscl_amd_simulate_scan(s, freq);
      if (fscl_amd_simulate_output(simulate_fname, q) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", simulate_fname);
      logmsg(MSG_STATUS, "Simulation: %d sites, %d sweeps, replicate %d, %llu degenerate sites, kernel %.3f ms\n", s->n_snps,
             simulate_sweep.n, simulate_rep, n_deg, fscl_amd_simulate_last_ms());
      fscl_amd_scan_free(q);
      free(freq);
    }
    if (dont_scan) {
      /* tables only: the simulation above, and a bootstrap of explicit sweeps below */
    } else if (grid_mode) {
      logmsg(MSG_STATUS, "scan mode grid: each cell's statistic is its maximum over the %d bp grid positions, in the scan "
                         "and in every permutation trial\n", small_grid_sp);
      fscl_amd_scan_chromosome_grid(s, sm, eval_range, small_grid_sp, large_grid_sp);
    } else {
      scan_chromosome(s, sm, eval_range, bp_resl, large_grid_sp, n_threads);
    }
    if (profile_fname) { /* the likelihood profile at -g spacing, of the data as loaded (rank 0 alone) */
      fscl_amd_profile_t *pf = fscl_amd_scan_profile(s, sm, eval_range, small_grid_sp, large_grid_sp);
      if (pf) {
        int n_missed = 0;
        fscl_amd_profile_cell_max(pf, s, NULL, &n_missed);
        fscl_amd_profile_output(profile_fname, s, pf, prepend_label);
        logmsg(MSG_STATUS, "Profile: %d grid points at %d bp, kernel %.3f ms, %d of %d cells have a grid point above the bisection's maximum\n",
               pf->n_pts, small_grid_sp, fscl_amd_profile_last_ms(), n_missed, s->n_scan_pts);
        fscl_amd_profile_free(pf);
      }
    }
    if (alpha_fname && !(ws && rk && atoi(ws) > 1 && atoi(rk) != 0)) {
      /* the scan points' alpha curves, of the data as loaded (rank 0 alone); no rand() draw */
      fscl_amd_curve_t *cv = malloc(sizeof *cv * (size_t)(s->n_scan_pts > 0 ? s->n_scan_pts : 1));
      int r;
      if (!cv) logmsg(MSG_FATAL, "fscl: out of memory (alpha curves)");
      r = fscl_amd_scan_point_curves(s, sm, eval_range, cv);
      if (r != 0) logmsg(MSG_FATAL, "fscl: alpha curves failed (code %d)", r);
      fscl_amd_curve_output(alpha_fname, s, cv, s->n_scan_pts, alpha_drop, prepend_label);
      logmsg(MSG_STATUS, "Alpha curves: %d points, kernel %.3f ms, %llu walks summed sequentially for the curves alone\n",
             s->n_scan_pts, fscl_amd_curve_last_ms(), fscl_amd_curve_forced());
      free(cv);
    }
    if (sites_fname && !(ws && rk && atoi(ws) > 1 && atoi(rk) != 0)) {
      /* the per-site terms of the scan points' walks, of the data as loaded (rank 0 alone); no rand() draw */
      fscl_amd_sites_t st;
      const int r = fscl_amd_scan_point_sites(s, sm, eval_range, sites_top, &st);
      if (r != 0) logmsg(MSG_FATAL, "fscl: site terms failed (code %d)", r);
      fscl_amd_sites_output(sites_fname, s, &st, prepend_label);
      logmsg(MSG_STATUS, "Site terms: %d walks, %llu terms, kernel %.3f ms\n", st.n, (unsigned long long)st.n_terms,
             fscl_amd_sites_last_ms());
      fscl_amd_sites_free(&st);
    }
    if (surface_fname && !(ws && rk && atoi(ws) > 1 && atoi(rk) != 0)) {
      /* the likelihood surfaces around the points of greatest CLR, of the data as loaded (rank 0 alone); no rand() draw */
      fscl_amd_surfaces_t sf;
      const int r = fscl_amd_scan_point_surfaces(s, sm, eval_range, surface_top, surface_halfwidth, surface_step, surface_lo,
                                                 surface_hi, surface_n, &sf);
      if (r != 0) logmsg(MSG_FATAL, "fscl: likelihood surfaces failed (code %d)", r);
      if (fscl_amd_surface_output(surface_fname, s, &sf, surface_drop, prepend_label) != 0)
        logmsg(MSG_FATAL, "fscl: cannot write %s", surface_fname);
      logmsg(MSG_STATUS, "Surfaces: %d points, %llu cells, %llu terms, kernel %.3f ms\n", sf.n, (unsigned long long)sf.n_cells,
             sf.n_terms, fscl_amd_surface_last_ms());
      fscl_amd_surfaces_free(&sf);
    }
    if (jackknife_fname && !(ws && rk && atoi(ws) > 1 && atoi(rk) != 0)) {
      /* the delete-one-block jackknife of the points of greatest CLR, of the data as loaded (rank 0 alone); no rand() draw */
      fscl_amd_blocks_t bk;
      const int r = fscl_amd_scan_point_jackknife(s, sm, eval_range, jackknife_top, jackknife_halfwidth, jackknife_step,
                                                  jackknife_lo, jackknife_hi, jackknife_n, jackknife_block, &bk);
      if (r != 0) logmsg(MSG_FATAL, "fscl: jackknife failed (code %d)", r);
      if (fscl_amd_jackknife_output(jackknife_fname, s, &bk, prepend_label) != 0)
        logmsg(MSG_FATAL, "fscl: cannot write %s", jackknife_fname);
      logmsg(MSG_STATUS, "Jackknife: %d peaks, %llu block cells, %llu terms, kernel %.3f ms\n", bk.n, (unsigned long long)bk.n_cells,
             bk.n_terms, fscl_amd_blocks_last_ms());
      fscl_amd_blocks_free(&bk);
    }
    if (cond_fname && !(ws && rk && atoi(ws) > 1 && atoi(rk) != 0)) {
      /* the conditional sweep scan given fixed sweeps, of the data as loaded (rank 0 alone); no rand() draw */
      fscl_amd_sweep_t *gsw = given_sw, top1;
      fscl_amd_conditional_t cd;
      int ng = given_sweep.n, r, bi = -1;
      if (ng == 0) { /* the scan point of greatest CLR (the first on a tie, never a NaN), at its fitted alpha */
        for (i = 0; i < s->n_scan_pts; i++)
          if (s->scan_pts[i].clr == s->scan_pts[i].clr && (bi < 0 || s->scan_pts[i].clr > s->scan_pts[bi].clr)) bi = i;
        if (bi >= 0) {
          top1.chr = s->scan_pts[bi].chr; top1.pos = s->scan_pts[bi].sweep_pos; top1.alpha = exp(s->scan_pts[bi].lalpha);
          gsw = &top1; ng = 1;
        }
      }
      r = fscl_amd_scan_conditional(s, sm, eval_range, gsw, ng, cond_halfwidth, cond_step, cond_la, cond_n_la, cond_rounds, cond_min_clr, &cd);
      if (r != 0) logmsg(MSG_FATAL, "fscl: conditional scan failed (code %d): %s", r, fscl_amd_conditional_error());
      if (fscl_amd_conditional_output(cond_fname, s, &cd, prepend_label) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", cond_fname);
      logmsg(MSG_STATUS, "Conditional scan: %llu positions, %llu terms, kernel %.3f ms, base folds %.3f s\n",
             (unsigned long long)cd.n_rows, cd.n_terms, fscl_amd_conditional_last_ms(), cd.fold_s);
      fscl_amd_conditional_free(&cd);
    }
    if (expect_fname && !(ws && rk && atoi(ws) > 1 && atoi(rk) != 0)) {
      /* what the model expects at the sweeps, of the data as loaded (rank 0 alone); no rand() draw */
      fscl_amd_expect_t ex;
      const int r = expect_sweep.n ? fscl_amd_scan_expect(s, sm, fsp, eval_range, expect_req, expect_sweep.n, expect_la, expect_n_la,
                                                          expect_bins, &ex)
                                   : fscl_amd_scan_point_expect(s, sm, fsp, eval_range, expect_top, large_grid_sp, expect_la,
                                                                expect_n_la, expect_bins, &ex);
      if (r != 0) logmsg(MSG_FATAL, "fscl: expectation failed (code %d): %s", r, fscl_amd_expect_error());
      if (fscl_amd_expect_output(expect_fname, s, &ex, prepend_label) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", expect_fname);
      logmsg(MSG_STATUS, "Expectation: %d sweeps, %d walks, kernel %.3f ms\n", ex.n, ex.n_tasks, fscl_amd_expect_last_ms());
      fscl_amd_expect_free(&ex);
    }
    if (dont_scan) {
      /* nothing to test or to write */
    } else if (n_permute > 0 && grid_mode)
      fscl_amd_scan_permute_grid(s, sm, n_permute, permute_nbp, eval_range, small_grid_sp, large_grid_sp, scan_width_mb);
    else if (n_permute > 0)
      scan_permute(s, sm, n_permute, permute_nbp, alpha_factor, n_threads, eval_range, bp_resl, large_grid_sp,
                   scan_width_mb);
    if (dont_scan) {
    } else if (ms_fname && maximum_only) output_block_maxima(output_fname, s, prepend_label);
    else scan_output(output_fname, s, maximum_only, n_permute, prepend_label);
    if (tail_fname) {
      /* the projected p-values, from the null CLRs the permutation test saved; no rand() draw */
      fscl_amd_tail_t tl;
      const int r = fscl_amd_tail_fit(s, tail_df, tail_min_n, &tl);
      if (r != 0) logmsg(MSG_FATAL, "fscl: tail fit failed (code %d)", r);
      if (fscl_amd_tail_output(tail_fname, s, &tl, prepend_label) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", tail_fname);
      logmsg(MSG_STATUS, "Tail fit: df %d, %d fit, %d central, %d nofit, kernel %.3f ms (%.3f s in all); calibration over %d points "
                         "with permute_p >= 5: median log10(p_tail / p_empirical) = %.3f\n", tail_df, tl.n_fit, tl.n_central,
             tl.n_nofit, tl.kernel_ms, tl.wall_s, tl.n_calibration, tl.calibration);
      fscl_amd_tail_free(&tl);
    }
    if (fw_fname) {
      /* the family-wise adjusted p-values, from unpruned trials of their own; no rand() draw, no record touched */
      fscl_amd_familywise_t fw;
      const unsigned long long fw_seed = fw_seed_s ? strtoull(fw_seed_s, NULL, 0) : 0xFD821A6ull;
      const int r = fscl_amd_familywise(s, sm, fw_trials, fw_seed, permute_nbp, eval_range, bp_resl, large_grid_sp, scan_width_mb,
                                        0, &fw);
      if (r != 0) logmsg(MSG_FATAL, "fscl: family-wise maxima failed (code %d): %s", r, fscl_amd_familywise_error());
      if (fscl_amd_familywise_output(fw_fname, s, &fw, prepend_label) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", fw_fname);
      if (fw_null_fname && fscl_amd_familywise_null_output(fw_null_fname, s, &fw, prepend_label) != 0)
        logmsg(MSG_FATAL, "fscl: cannot write %s", fw_null_fname);
      logmsg(MSG_STATUS, "Family-wise maxima: M %d unpruned trials of %d points, maxt kernel %.3f ms, %.3f s in all, %.0f grid points x "
                         "trials per second\n", fw.trials, fw.n, fw.kernel_ms, fw.wall_s,
             fw.wall_s > 0 ? (double)fw.n * (double)fw.trials / fw.wall_s : 0.0);
      fscl_amd_familywise_free(&fw);
    }
    if (bootstrap_fname) {
      /* the parametric bootstrap, last: simulate under the sweeps, rescan, summarise */
      fscl_amd_boot_t *bt;
      double tm[5];
      int r;
      if (n_boot == 0) { free(boot_sw); boot_sw = top_sweeps(s, bootstrap_top, bootstrap_window, &n_boot); }
      bt = malloc(sizeof *bt * ((size_t)n_boot * (size_t)bootstrap_reps + 1));
      if (!bt) logmsg(MSG_FATAL, "fscl: out of memory (bootstrap)");
      r = fscl_amd_bootstrap(s, sm, fsp, boot_sw, n_boot, bootstrap_reps, sim_seed, bootstrap_window, eval_range, bp_resl,
                             large_grid_sp, bt);
      if (r != 0) logmsg(MSG_FATAL, "fscl: bootstrap failed (code %d)", r);
      fscl_amd_bootstrap_output(bootstrap_fname, s, boot_sw, n_boot, bootstrap_reps, bt, prepend_label);
      fscl_amd_bootstrap_times(tm);
      logmsg(MSG_STATUS, "Bootstrap: %d sweeps, %d replicates, %.3f s (simulation %.3f s, null model %.3f s, upload %.3f s, "
                         "scan %.3f s)\n", n_boot, bootstrap_reps, tm[0], tm[1], tm[2], tm[3], tm[4]);
      free(bt);
    }
    free(sim_sw); free(boot_sw); free(given_sw); free(expect_sw); free(expect_req);
    if (verbosity >= MSG_DEBUG1) {
      fscl_amd_stats_t st;
      fscl_amd_get_stats(&st);
      fprintf(stderr, "fscl_amd: scan %.3f s, permute %.3f s (host permutation %.3f s, %d trials), kernels %.3f s, "
                      "%llu grid-point evaluations, %llu terms, unsafe walks %llu, slow walks %llu, ties %llu, negj %llu\n",
              st.scan_s, st.permute_s, st.host_perm_s, st.trials, st.kernel_ms / 1e3, st.gp_evals, st.n_terms,
              st.n_unsafe, st.n_slow, st.n_ties, st.negj);
    }
    fscl_amd_shutdown();
  }
  return 0;
}
