/* cli_options.c -- the `fscl` command line's option table (the reference's fscl.c:38-102 and this
 * project's own), the argument loop (cmdline-utils.c:28-100: "--long=value" or "-x value", flags
 * toggle) and the check-and-resolve pass (fscl.c:180-258 and every later option's refusals).
 *
 * Deliberate difference: "--long value" without '=' is an error instead of a NULL
 * dereference. */
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_options.h"

enum { T_STR, T_INT, T_DBL, T_FLAG, T_LIST };
typedef struct { char s; const char *l; size_t at; int t; const char *doc; } opt_t; /* (at: the value's offset in cli_opts_t) */
#define AT(field) offsetof(cli_opts_t, field)

static const cli_opts_t defaults = {
    .asc_min_freq = 1, .small_grid_sp = 1000, .large_grid_sp = 100000, .minimum_obs_depth = 5, .n_threads = 1,
    .verbosity = MSG_STATUS, .spline_pts = N_SPLINE_KNOTS, .permute_nbp = 0.1, .alpha_factor = 1.0, .scan_width_mb = 1.0,
    .alpha_drop = 2.0, .sites_top = 10, .bootstrap_reps = 100, .bootstrap_window = -1, .bootstrap_top = 3,
    .tail_df = 2, .tail_min_n = 20, .fw_trials = 1000,
    .surface_top = 3, .surface_halfwidth = -1, .surface_step = -1, .surface_drop = 2.0, .surface_grid = {LOG_AD_MIN, LOG_AD_MAX, 33},
    .jackknife_top = 3, .jackknife_block = -1, .jackknife_halfwidth = -1, .jackknife_step = -1,
    .cond_halfwidth = 0, .cond_rounds = 1, .cond_min_clr = 0.0, .expect_top = 3, .expect_bins = 24};

static const opt_t opts[] = {
    {'f', "snpfile", AT(snp_fname), T_STR, "File name of file with SNP frequency data"},
    {'d', "asc-depth", AT(asc_depth), T_INT, "Depth of SNP ascertainment sample"},
    {0, "asc-minimum-freq", AT(asc_min_freq), T_INT, "minimum number of observations of both alleles for SNP ascertainment"},
    {'p', "n-permute", AT(n_permute), T_INT, "number of snp block permutations for p-value computations"},
    {0, "permute-nbp", AT(permute_nbp), T_DBL, "probability for switching to a new snp block for permutations"},
    {0, "n-threads", AT(n_threads), T_INT, "accepted for compatibility (the GPU evaluates all points at once)"},
    {'a', "alpha-factor", AT(alpha_factor), T_DBL, "multiply 1/alpha by this factor to determine single sweep window size"},
    {'g', "fine-grid-spacing", AT(small_grid_sp), T_INT, "Spacing in bp of the CLR profile's positions (--profile-file); must divide -G"},
    {'G', "coarse-grid-spacing", AT(large_grid_sp), T_INT, "Size of coarse grid in which CLR maxima will be selected"},
    {'w', "sweep-width", AT(scan_width_mb), T_DBL, "maximum width of sweep effect in scanning, in Mb"},
    {0, "minimum-depth", AT(minimum_obs_depth), T_INT, "minimum depth of sample (lower depth SNPs ignored)"},
    {'m', "msfile", AT(ms_fname), T_STR, "Name of an ms output file"},
    {0, "ms-segment-length", AT(ms_segment_length), T_INT, "Length in bp of simulated ms segments (use with -m option only)"},
    {0, "ms-folded", AT(ms_folded), T_FLAG, "For ms input, treat all sites as folded"},
    {0, "max-only", AT(maximum_only), T_FLAG, "for ms input, output only the maximum CLR for each input block"},
    {0, "ms-sample-first", AT(ms_sample_first), T_INT, "index of first chromosome in ms sample to analyze"},
    {0, "ms-sample-size", AT(ms_sample_size), T_INT, "number of consecutive chromosomes in ms output to take as the sample"},
    {0, "force-neutral-spectrum", AT(force_neutral), T_FLAG, "Do not estimate background spectrum from the data. Use sum(1/i)/i"},
    {'b', "background-spectrum", AT(bs_fname), T_STR, "Load the background frequency spectrum from a file"},
    {0, "output-bs", AT(output_bs_fname), T_STR, "write estimated background site-frequency spectra to file"},
    {0, "include-invariant", AT(include_invariant), T_FLAG, "Include invariant sites in analysis (default is to ignore them)"},
    {0, "splines", AT(spline_pts), T_INT, "Number of knot points to approximate sweep model w/ respect to alpha"},
    {0, "prepend-label", AT(prepend_label), T_STR, "optional token to prepend to each line of the sweep scan output"},
    {'v', "verbosity", AT(verbosity), T_INT, "verbosity level 0-5, default 3, debug 4 and above"},
    {'o', "output-file", AT(output_fname), T_STR, "output file for scan results"},
    {0, "no-scan", AT(dont_scan), T_FLAG, "do not scan chromosome, compute background frequency spectrum only"},
    {0, "ascbias-background-only", AT(bg_only), T_FLAG, "correct for ascertainment bias only in estimating the background site frequency spectrum"},
    {0, "n-gpus", AT(n_gpus), T_INT, "GPUs to use (default: every visible GPU, or $FSCL_AMD_DEVICE alone when set)"},
    {0, "permute-mode", AT(permute_mode), T_STR, "parity (default: the reference's rand() stream, identical results) or "
                                                 "throughput (counter-based random numbers, trials independent; not identical)"},
    {0, "profile-file", AT(profile_fname), T_STR, "write CLR and alpha at every -g spaced position (the likelihood profile) to this file"},
    {0, "alpha-file", AT(alpha_fname), T_STR, "write every scan point's alpha likelihood curve and support interval to this file"},
    {0, "alpha-drop", AT(alpha_drop), T_DBL, "log-likelihood drop of the support interval in --alpha-file (default 2.0; descriptive: "
                                             "the likelihood is composite)"},
    {0, "sites-file", AT(sites_fname), T_STR, "write the per-site likelihood terms of the scan points' walks, and a footprint summary per "
                                              "point, to this file"},
    {0, "sites-top", AT(sites_top), T_INT, "--sites-file takes this many points of greatest CLR (default 10; 0: every point)"},
    {0, "scan-mode", AT(scan_mode), T_STR, "bisection (default: search_maxpos in every cell) or grid (the maximum over each cell's "
                                           "-g spaced positions, in the scan and in the permutation test; one process, parity only)"},
    {0, "permute-seed", AT(permute_seed), T_STR, "seed of the throughput mode's random numbers (default 0xFD821A6)"},
    {0, "simulate-file", AT(simulate_fname), T_STR, "write one replicate of the data simulated under the sweep model (SNP input format) "
                                                    "to this file; needs no scan"},
    {0, "simulate-sweep", AT(simulate_sweep), T_LIST, "chr:pos:alpha of a sweep planted in --simulate-file (may be given several times; "
                                                      "none: a neutral replicate)"},
    {0, "simulate-seed", AT(simulate_seed), T_STR, "seed of the simulation and the bootstrap (default 0xFD821A6)"},
    {0, "simulate-rep", AT(simulate_rep), T_INT, "replicate number of --simulate-file (default 0)"},
    {0, "bootstrap-file", AT(bootstrap_fname), T_STR, "parametric bootstrap: simulate under the planted sweeps, rescan, write every "
                                                      "replicate's estimate and a quantile summary per sweep to this file"},
    {0, "bootstrap-reps", AT(bootstrap_reps), T_INT, "replicates of --bootstrap-file (default 100)"},
    {0, "bootstrap-window", AT(bootstrap_window), T_INT, "a replicate's estimate is its best scan point within this many bp of the planted "
                                                         "position (default: the -G spacing)"},
    {0, "bootstrap-sweep", AT(bootstrap_sweep), T_LIST, "chr:pos:alpha of a sweep to bootstrap (may be given several times; none: the "
                                                        "--bootstrap-top scan points)"},
    {0, "bootstrap-top", AT(bootstrap_top), T_INT, "without --bootstrap-sweep, bootstrap this many scan points of greatest CLR (default 3)"},
    {0, "tail-file", AT(tail_fname), T_STR, "after the permutation test, write every scan point's p-value projected from a noncentral "
                                            "chi-square fit of its null CLRs (below 1/n-permute) to this file"},
    {0, "tail-df", AT(tail_df_s), T_STR, "degrees of freedom of the --tail-file fit: an even integer >= 2 (default 2)"},
    {0, "surface-file", AT(surface_fname), T_STR, "write the position-by-alpha likelihood surface around the scan points of greatest "
                                                  "CLR, and a region summary per point, to this file"},
    {0, "surface-top", AT(surface_top), T_INT, "--surface-file takes this many points of greatest CLR (default 3)"},
    {0, "surface-halfwidth", AT(surface_halfwidth), T_INT, "half-width in bp of a surface's positions around its point (default: the -G spacing)"},
    {0, "surface-step", AT(surface_step), T_INT, "spacing in bp of a surface's positions (default: the -g spacing; at least 1)"},
    {0, "surface-alphas", AT(surface_alphas), T_STR, "LO:HI:N, the surface's alpha grid: natural-log alpha endpoints within [-20, 4] and a "
                                                     "count N <= 63 (default -20:4:33, steps of 0.75); the point's fitted alpha is added"},
    {0, "surface-drop", AT(surface_drop), T_DBL, "log-likelihood drop of the region in --surface-file (default 2.0, as --alpha-drop; a joint "
                                                 "two-parameter 95 % region under the chi-square reading would be about 3.0; descriptive: "
                                                 "the likelihood is composite)"},
    {0, "conditional-file", AT(cond_fname), T_STR, "write the conditional sweep scan -- the likelihood ratio of one more sweep at every "
                                                   "grid position, given the --given-sweep sweeps held fixed -- to this file"},
    {0, "given-sweep", AT(given_sweep), T_LIST, "chr:pos:alpha of a sweep held fixed in --conditional-file (may be given several times; "
                                                "default: the scan point of greatest CLR at its fitted alpha)"},
    {0, "conditional-halfwidth", AT(cond_halfwidth_s), T_STR, "evaluate only the positions within this many bp of a given sweep "
                                                              "(default 0: the whole chromosome)"},
    {0, "conditional-step", AT(cond_step_s), T_STR, "spacing in bp of the --conditional-file positions (default: the -g spacing; at least 1)"},
    {0, "conditional-alphas", AT(cond_alphas), T_STR, "LO:HI:N, the candidate's alpha grid (default: the --surface-alphas value)"},
    {0, "conditional-rounds", AT(cond_rounds_s), T_STR, "forward selection: after a round each chromosome's position of greatest conditional "
                                                        "CLR joins the given sweeps (1 .. 8, default 1)"},
    {0, "conditional-min-clr", AT(cond_min_clr_s), T_STR, "a round's maximum joins the given sweeps only above this conditional CLR (default 0)"},
    {0, "jackknife-file", AT(jackknife_fname), T_STR, "write a delete-one-block jackknife of the scan points of greatest CLR (the "
                                                      "re-maximised position, alpha and CLR with each genomic block left out, and their "
                                                      "standard errors) to this file"},
    {0, "jackknife-top", AT(jackknife_top), T_INT, "--jackknife-file takes this many points of greatest CLR (default 3)"},
    {0, "jackknife-block", AT(jackknife_block), T_INT, "block length in bp of the jackknife (default: half the -G spacing; at least 1)"},
    {0, "jackknife-halfwidth", AT(jackknife_halfwidth), T_INT, "half-width in bp of the jackknife's positions (default: --surface-halfwidth)"},
    {0, "jackknife-step", AT(jackknife_step), T_INT, "spacing in bp of the jackknife's positions (default: --surface-step)"},
    {0, "jackknife-alphas", AT(jackknife_alphas), T_STR, "LO:HI:N, the jackknife's alpha grid (default: --surface-alphas)"},
    {0, "expect-file", AT(expect_fname), T_STR, "write what the fitted model expects at the sweeps of greatest CLR -- the expectation and SD of "
                                                "the CLR under the sweep and under neutrality, per bin of log(alpha d), along an alpha "
                                                "list, and in all -- to this file"},
    {0, "expect-top", AT(expect_top_s), T_STR, "--expect-file takes this many points of greatest CLR (default 3)"},
    {0, "expect-sweep", AT(expect_sweep), T_LIST, "chr:pos:alpha of a sweep for --expect-file (may be given several times; replaces the "
                                                  "--expect-top choice)"},
    {0, "expect-alphas", AT(expect_alphas), T_STR, "LO:HI:N, the alpha list of --expect-file's curve rows (default: the --surface-alphas "
                                                   "value); the sweep's own alpha is added"},
    {0, "expect-bins", AT(expect_bins_s), T_STR, "equal-width bins of log(alpha d) over [-20, 4] in --expect-file (1 .. 64, default 24)"},
    {0, "tail-min-n", AT(tail_min_n), T_INT, "--tail-file fits a point with at least this many positive null CLRs (default 20)"},
    {0, "familywise-file", AT(fw_fname), T_STR, "after the permutation test and the output, write every scan point's family-wise adjusted "
                                                "p-values (Westfall-Young maxT over unpruned permutation trials: single-step, per "
                                                "chromosome and step-down) and the genome-wide CLR thresholds to this file"},
    {0, "familywise-trials", AT(fw_trials_s), T_STR, "unpruned trials of --familywise-file, each a full scan (default 1000; at least 1)"},
    {0, "familywise-seed", AT(fw_seed_s), T_STR, "seed of the --familywise-file permutations, those of the throughput mode under this "
                                                 "seed (default 0xFD821A6)"},
    {0, "familywise-null-file", AT(fw_null_fname), T_STR, "write every --familywise-file trial's genome and chromosome maxima to this file"},
    {0, NULL, 0, 0, NULL}};

static void usage(const opt_t *o) {
  fprintf(stderr, "fscl (MI355X) -- composite-likelihood selective sweep scan\n");
  for (; o->l; o++) {
    if (o->s) fprintf(stderr, "  -%c, --%-28s %s\n", o->s, o->l, o->doc);
    else fprintf(stderr, "      --%-28s %s\n", o->l, o->doc);
  }
}

static void list_add(strlist_t *l, const char *arg) {
  l->v = realloc(l->v, sizeof(char *) * (size_t)(l->n + 1));
  if (!l->v) { fprintf(stderr, "out of memory (options)\n"); exit(1); }
  l->v[l->n++] = strdup(arg);
}

int cli_parse(int argc, char **argv, cli_opts_t *o) {
  int i;
  *o = defaults;
  if (argc == 1) { usage(opts); return 255; }
  for (i = 1; i < argc;) {
    const char *a = argv[i], *arg;
    char name[256];
    void *v;
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
    for (j = 0; opts[j].l; j++)
      if (lng ? strcmp(name, opts[j].l) == 0 : opts[j].s == name[0]) break;
    v = (char *)o + opts[j].at;
    if (!opts[j].l) fprintf(stderr, "Unrecognized option \"%s\"\n", a);
    else if (opts[j].t == T_FLAG) *(int *)v ^= 1;
    else if (!arg) { fprintf(stderr, "Option \"%s\" needs a value (--%s=value or -x value)\n", a, opts[j].l); return 255; }
    else if (opts[j].t == T_STR) *(char **)v = strdup(arg);
    else if (opts[j].t == T_LIST) list_add((strlist_t *)v, arg);
    else if (opts[j].t == T_INT) *(int *)v = atoi(arg);
    else *(double *)v = atof(arg);
    i += (lng || (opts[j].l && opts[j].t == T_FLAG)) ? 1 : 2;
  }
  return -1;
}

void cli_opts_free(cli_opts_t *o) {
  int j, k;
  for (j = 0; opts[j].l; j++) {
    void *v = (char *)o + opts[j].at;
    if (opts[j].t == T_STR) free(*(char **)v);
    if (opts[j].t == T_LIST) {
      strlist_t *l = v;
      for (k = 0; k < l->n; k++) free(l->v[k]);
      free(l->v);
    }
  }
  *o = defaults;
}

/* ---- the helpers of the check pass: each rule exists once ---- */

const char *cli_multi_rank(void) {
  const char *ws = getenv("WORLD_SIZE");
  return ws && getenv("RANK") && atoi(ws) > 1 ? ws : NULL;
}

int cli_rank0(void) { return !cli_multi_rank() || atoi(getenv("RANK")) == 0; }

/* where `bad`: the message at MSG_ERROR, and 1 */
__attribute__((format(printf, 2, 3))) static int refuse(int bad, const char *fmt, ...) {
  char buf[4096];
  va_list ap;
  if (!bad) return 0;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  logmsg(MSG_ERROR, "%s", buf);
  return 1;
}

static int one_process(int on, const char *what) {
  return refuse(on && cli_multi_rank(), "Error: %s runs in one process (not with WORLD_SIZE=%s ranks).\n", what, cli_multi_rank());
}

/* a whole decimal integer within [lo, hi]: 1 and *out, else 0 and *out untouched */
static int int_in_range(const char *t, long lo, long hi, int *out) {
  char *end = NULL;
  long v;
  errno = 0;
  v = strtol(t, &end, 10);
  if (end == t || *end || errno || v < lo || v > hi) return 0;
  *out = (int)v;
  return 1;
}

/* --NAME-alphas=LO:HI:N into the grid: 1 and the message where it is none the library takes */
static int alpha_grid_option(const char *name, const char *text, alpha_grid_t *g) {
  char tail_c = 0;
  double probe[FSCL_AMD_SURFACE_MAX_LA];
  return refuse(sscanf(text, "%lf:%lf:%d%c", &g->lo, &g->hi, &g->n, &tail_c) != 3 ||
                    fscl_amd_surface_alphas(g->lo, g->hi, g->n, NAN, probe) < 1,
                "Error: --%s-alphas must be LO:HI:N with -20 <= LO <= HI <= 4 (natural-log alpha), 1 <= N <= 63, "
                "and LO < HI unless N is 1 (not \"%s\").\n", name, text);
}

/* the alpha of every chr:pos:alpha text of one option (the chromosome names are checked once the data is loaded,
   before the scan): positive where a last colon is found, or, with log_range, present and within the tables' range */
static int sweep_texts(const strlist_t *l, const char *opt, int log_range) {
  int i, stop = 0;
  for (i = 0; i < l->n; i++) {
    const char *t = l->v[i], *c = strrchr(t, ':');
    const double a = c ? atof(c + 1) : 0.0;
    if (log_range)
      stop |= refuse(!c || !(a > 0.0) || !(log(a) >= LOG_AD_MIN && log(a) <= LOG_AD_MAX),
                     "Error: --%s=%s: expected chr:pos:alpha, alpha positive with its natural log within [-20, 4].\n", opt, t);
    else
      stop |= refuse(c && !(a > 0.0), "Error: --%s=%s: alpha must be positive.\n", opt, t);
  }
  return stop;
}

/* ---- the check pass, in the order the messages have always come ---- */

/* fscl.c:180-258 */
static int check_reference_options(cli_opts_t *o) {
  int stop = 0;
  if (o->verbosity < 0) o->verbosity = 0;
  configure_logmsg(o->verbosity);
  if (o->bg_only) logmsg(MSG_STATUS, "ascertainment bias correction to background site frequency spectrum only\n");
  if (o->minimum_obs_depth < 5) o->minimum_obs_depth = 5;
  stop |= refuse(o->spline_pts < N_SPLINE_KNOTS,
                 "Error: must use at least %d spline functions to approximate sweep model\nlikelihood function.\n", N_SPLINE_KNOTS);
  if (o->spline_pts > 500)
    logmsg(MSG_WARN, "Warning: estimating %d spline functions will significantly inflate execution\ntime with little "
                     "gain in accuracy...\n", o->spline_pts);
  stop |= refuse(!o->snp_fname && !o->ms_fname,
                 "Error: input snp frequency file or ms file not specified. Use -f option or -m option.\n");
  stop |= refuse(o->snp_fname && o->ms_fname, "Specify either a snp frequency file or an ms file, not both.\n");
  stop |= refuse(!o->output_fname, "Specify an output file name with -o option\n");
  if (o->ms_segment_length && !o->ms_fname) {
    logmsg(MSG_WARN, "Warning: --ms-segment-length option ignored if -m option is not used.\n");
    o->ms_segment_length = 0;
  }
  stop |= refuse(o->asc_depth == 1 || o->asc_depth < 0, "Error: if specified, ascertainment sample depth must be at least 2.\n");
  stop |= refuse(o->asc_depth >= 2 && o->asc_min_freq > 2 * o->asc_depth,
                 "Error: SNP ascertainment is impossible with asc. sample depth and asc. minimum allele frequency setting\n");
  if (o->asc_depth >= 2 && o->asc_min_freq == 0) o->asc_min_freq = 1;
  stop |= refuse(o->small_grid_sp < 1 && !o->output_bs_fname, "Error: specify sweep position grid spacing with -g option (in bp).\n");
  stop |= refuse((o->profile_fname || !o->output_bs_fname) && o->small_grid_sp > 0 && o->large_grid_sp > 0 &&
                     o->large_grid_sp % o->small_grid_sp != 0,
                 "Error: fine grid spacing must evenly divide coarse grid spacing.\n");
  return stop;
}

static int check_scan_options(cli_opts_t *o) {
  int stop = 0;
  stop |= refuse(o->profile_fname && o->dont_scan, "Error: --profile-file needs the scan (not with --no-scan).\n");
  stop |= refuse(o->profile_fname && o->small_grid_sp < 1, "Error: --profile-file needs a positive -g spacing.\n");
  stop |= refuse(o->alpha_fname && o->dont_scan, "Error: --alpha-file needs the scan (not with --no-scan).\n");
  stop |= refuse(o->sites_fname && o->dont_scan, "Error: --sites-file needs the scan (not with --no-scan).\n");
  stop |= refuse(o->sites_top < 0, "Error: --sites-top must be >= 0.\n");
  stop |= refuse(!(o->alpha_drop >= 0.0), "Error: --alpha-drop must be >= 0.\n");
  stop |= refuse(o->large_grid_sp < 1, "Error: coarse grid spacing must be positive.\n");
  stop |= refuse(o->n_gpus < 0, "Error: --n-gpus must be >= 0.\n");
  o->throughput = o->permute_mode && !strcmp(o->permute_mode, "throughput");
  stop |= refuse(o->permute_mode && strcmp(o->permute_mode, "parity") && !o->throughput,
                 "Error: --permute-mode must be parity or throughput.\n");
  o->grid_mode = o->scan_mode && !strcmp(o->scan_mode, "grid");
  stop |= refuse(o->scan_mode && strcmp(o->scan_mode, "bisection") && !o->grid_mode, "Error: --scan-mode must be bisection or grid.\n");
  stop |= refuse(o->grid_mode && o->throughput,
                 "Error: --scan-mode=grid runs on the parity stream only (not with --permute-mode=throughput).\n");
  stop |= one_process(o->grid_mode, "--scan-mode=grid");
  stop |= refuse(o->grid_mode && o->small_grid_sp < 1, "Error: --scan-mode=grid needs a positive -g spacing.\n");
  return stop;
}

static int check_bootstrap(cli_opts_t *o) {
  int stop = 0;
  stop |= refuse(o->bootstrap_fname && o->dont_scan && o->bootstrap_sweep.n == 0,
                 "Error: --bootstrap-file with --no-scan needs --bootstrap-sweep (no scan points to take).\n");
  stop |= refuse(o->bootstrap_fname && o->grid_mode, "Error: --bootstrap-file rescans by bisection (not with --scan-mode=grid).\n");
  stop |= one_process(o->bootstrap_fname != NULL, "--bootstrap-file");
  stop |= refuse(o->bootstrap_fname && o->bootstrap_reps < 0, "Error: --bootstrap-reps must be >= 0.\n");
  stop |= refuse(o->bootstrap_fname && o->bootstrap_top < 0, "Error: --bootstrap-top must be >= 0.\n");
  if (o->bootstrap_window < 0) o->bootstrap_window = o->large_grid_sp;
  stop |= sweep_texts(&o->simulate_sweep, "simulate-sweep", 0);
  stop |= sweep_texts(&o->bootstrap_sweep, "bootstrap-sweep", 0);
  return stop;
}

static int check_tail_and_familywise(cli_opts_t *o) {
  int stop = 0;
  stop |= refuse(o->tail_df_s && (!int_in_range(o->tail_df_s, 2, 1000000, &o->tail_df) || (o->tail_df & 1)),
                 "Error: --tail-df must be an even integer >= 2 (not \"%s\").\n", o->tail_df_s);
  stop |= refuse(o->tail_fname && o->n_permute <= 0, "Error: --tail-file needs the permutation test (--n-permute > 0).\n");
  stop |= refuse(o->tail_fname && o->dont_scan, "Error: --tail-file needs the scan (not with --no-scan).\n");
  stop |= one_process(o->tail_fname != NULL, "--tail-file");
  stop |= refuse(o->tail_fname && o->tail_min_n < 1, "Error: --tail-min-n must be >= 1.\n");
  stop |= refuse(!o->fw_fname && (o->fw_trials_s || o->fw_seed_s || o->fw_null_fname),
                 "Error: --familywise-trials, --familywise-seed and --familywise-null-file need --familywise-file.\n");
  stop |= refuse(o->fw_trials_s && !int_in_range(o->fw_trials_s, 1, 100000000, &o->fw_trials),
                 "Error: --familywise-trials must be an integer >= 1 (not \"%s\").\n", o->fw_trials_s);
  stop |= refuse(o->fw_fname && o->dont_scan, "Error: --familywise-file needs the scan (not with --no-scan).\n");
  stop |= refuse(o->fw_fname && o->grid_mode,
                 "Error: --familywise-file evaluates the bisection scan's cells (not with --scan-mode=grid).\n");
  stop |= one_process(o->fw_fname != NULL, "--familywise-file");
  return stop;
}

static int check_surface(cli_opts_t *o) {
  int stop = 0;
  stop |= refuse(o->surface_fname && o->dont_scan, "Error: --surface-file needs the scan (not with --no-scan).\n");
  stop |= refuse(o->surface_top < 0, "Error: --surface-top must be >= 0.\n");
  if (o->surface_halfwidth < 0) o->surface_halfwidth = o->surface_halfwidth == -1 ? o->large_grid_sp : -2; /* (-2: refused) */
  stop |= refuse(o->surface_halfwidth == -2, "Error: --surface-halfwidth must be >= 0.\n");
  if (o->jackknife_step == -1) o->jackknife_step = o->surface_step == -1 ? o->small_grid_sp : o->surface_step; /* --surface-step as given */
  if (o->surface_step == -1) o->surface_step = o->surface_fname ? o->small_grid_sp : 1;
  stop |= refuse(o->surface_step < 1, "Error: --surface-step must be at least 1.\n");
  stop |= refuse(!(o->surface_drop >= 0.0), "Error: --surface-drop must be >= 0.\n");
  if (o->surface_alphas) stop |= alpha_grid_option("surface", o->surface_alphas, &o->surface_grid);
  return stop;
}

static int check_conditional(cli_opts_t *o) {
  int stop = 0;
  stop |= refuse(o->cond_fname && o->dont_scan && o->given_sweep.n == 0,
                 "Error: --conditional-file with --no-scan needs explicit --given-sweep sweeps.\n");
  stop |= refuse(!o->cond_fname && (o->given_sweep.n || o->cond_halfwidth_s || o->cond_step_s || o->cond_rounds_s ||
                                    o->cond_min_clr_s || o->cond_alphas),
                 "Error: --given-sweep and the --conditional-* options need --conditional-file.\n");
  o->cond_step = o->small_grid_sp;
  if (o->cond_step_s && !int_in_range(o->cond_step_s, 1, INT_MAX, &o->cond_step)) o->cond_step = 0;
  stop |= refuse(o->cond_fname && o->cond_step < 1, "Error: --conditional-step must be at least 1.\n");
  stop |= refuse(o->cond_halfwidth_s && !int_in_range(o->cond_halfwidth_s, 0, INT_MAX, &o->cond_halfwidth),
                 "Error: --conditional-halfwidth must be >= 0.\n");
  stop |= refuse(o->cond_rounds_s && !int_in_range(o->cond_rounds_s, 1, FSCL_AMD_COND_MAX_ROUNDS, &o->cond_rounds),
                 "Error: --conditional-rounds must be 1 .. 8.\n");
  if (o->cond_min_clr_s) {
    char *end = NULL;
    o->cond_min_clr = strtod(o->cond_min_clr_s, &end);
    stop |= refuse(end == o->cond_min_clr_s || *end || !(o->cond_min_clr == o->cond_min_clr), "Error: --conditional-min-clr must be a number.\n");
  }
  o->cond_grid = o->surface_grid;
  if (o->cond_alphas) stop |= alpha_grid_option("conditional", o->cond_alphas, &o->cond_grid);
  stop |= sweep_texts(&o->given_sweep, "given-sweep", 1);
  return stop;
}

static int check_expect(cli_opts_t *o) {
  int stop = 0;
  stop |= refuse(!o->expect_fname && (o->expect_sweep.n || o->expect_alphas || o->expect_top_s || o->expect_bins_s),
                 "Error: --expect-sweep, --expect-top, --expect-alphas and --expect-bins need --expect-file.\n");
  stop |= refuse(o->expect_fname && o->dont_scan && o->expect_sweep.n == 0,
                 "Error: --expect-file with --no-scan needs explicit --expect-sweep sweeps.\n");
  stop |= refuse(o->expect_top_s && !int_in_range(o->expect_top_s, 0, INT_MAX, &o->expect_top), "Error: --expect-top must be >= 0.\n");
  stop |= refuse(o->expect_bins_s && !int_in_range(o->expect_bins_s, 1, FSCL_AMD_EXPECT_MAX_BINS, &o->expect_bins),
                 "Error: --expect-bins must be 1 .. 64.\n");
  o->expect_grid = o->surface_grid;
  if (o->expect_alphas) stop |= alpha_grid_option("expect", o->expect_alphas, &o->expect_grid);
  stop |= sweep_texts(&o->expect_sweep, "expect-sweep", 1);
  return stop;
}

/* (after check_surface: the half-width and the alpha grid default to the surface's as resolved there) */
static int check_jackknife(cli_opts_t *o) {
  int stop = 0;
  stop |= refuse(o->jackknife_fname && o->dont_scan, "Error: --jackknife-file needs the scan (not with --no-scan).\n");
  stop |= refuse(o->jackknife_top < 0, "Error: --jackknife-top must be >= 0.\n");
  if (o->jackknife_block == -1) o->jackknife_block = o->large_grid_sp / 2 > 1 ? o->large_grid_sp / 2 : 1;
  stop |= refuse(o->jackknife_block < 1, "Error: --jackknife-block must be at least 1.\n");
  if (o->jackknife_halfwidth == -1) o->jackknife_halfwidth = o->surface_halfwidth;
  stop |= refuse(o->jackknife_halfwidth < 0, "Error: --jackknife-halfwidth must be >= 0.\n");
  stop |= refuse(o->jackknife_step < 1, "Error: --jackknife-step must be at least 1.\n");
  o->jackknife_grid = o->surface_grid;
  if (o->jackknife_alphas) stop |= alpha_grid_option("jackknife", o->jackknife_alphas, &o->jackknife_grid);
  return stop;
}

int cli_check(cli_opts_t *o) {
  int stop = check_reference_options(o);
  stop |= check_scan_options(o);
  stop |= check_bootstrap(o);
  stop |= check_tail_and_familywise(o);
  stop |= check_surface(o);
  stop |= check_conditional(o);
  stop |= check_expect(o);
  stop |= check_jackknife(o);
  if (o->permute_seed && !o->throughput) logmsg(MSG_WARN, "Warning: --permute-seed is used only with --permute-mode=throughput.\n");
  if (stop && o->verbosity <= MSG_FATAL) logmsg(MSG_FATAL, "Fatal errors have occurred, use -v 1 or greater to see them.\n");
  return stop;
}
