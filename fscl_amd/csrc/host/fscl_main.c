/* fscl_main.c -- the `fscl` command line, drop-in for the reference's (main fscl.c:272-341; the
 * options, their parsing and their checks are cli_options.c).  The scan path runs on the GPU.
 *
 * main() is parse, check, load, tables and then a fixed sequence around the scan, the permutation
 * test and the output: one function per output file, each with its call, its failure message, its
 * status line and its free.
 *
 * Deliberate differences: -m reads ms output with defined semantics (all blocks form
 * one genome, one chromosome per block, --max-only prints the maximum of each block); -b reads the
 * format --output-bs writes.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "cli_options.h"

enum { EVAL_RANGE = 81920, BP_RESL = 128 };
#define DEFAULT_SEED 0xFD821A6ull

/* fscl.c:33-34 */
char *prepend_label, *output_fname;
int spline_pts, n_permute;

/* what the steps of one run share */
typedef struct {
  const cli_opts_t *o;
  scan_t *s;
  sm_ptable_t *sm;
  double **fsp;
  fscl_amd_sweep_t *sim_sw, *boot_sw, *given_sw, *expect_sw; /* the --*-sweep options, parsed */
  fsclg_site_req_t *expect_req;                              /* expect_sw as requests */
  double cond_la[FSCL_AMD_SURFACE_MAX_LA], expect_la[FSCL_AMD_SURFACE_MAX_LA];
  int cond_n_la, expect_n_la;
  unsigned long long sim_seed;
} cli_run_t;

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
/* the sweep options and every host-only refusal of the conditional scan, --expect-file and
   --familywise-file, once the data is loaded: on every rank, before any device work */
static void parse_and_check(cli_run_t *c) {
  const cli_opts_t *o = c->o;
  int i;
  c->sim_seed = o->simulate_seed ? strtoull(o->simulate_seed, NULL, 0) : DEFAULT_SEED;
  c->sim_sw = parse_sweeps(c->s, &o->simulate_sweep, "simulate-sweep");
  c->boot_sw = parse_sweeps(c->s, &o->bootstrap_sweep, "bootstrap-sweep");
  c->given_sw = parse_sweeps(c->s, &o->given_sweep, "given-sweep");
  c->cond_n_la = o->cond_fname ? fscl_amd_surface_alphas(o->cond_grid.lo, o->cond_grid.hi, o->cond_grid.n, NAN, c->cond_la) : 0;
  if (o->cond_fname && fscl_amd_conditional_check(c->s, c->given_sw, o->given_sweep.n, o->cond_halfwidth, o->cond_step, c->cond_la,
                                                  c->cond_n_la, o->cond_rounds, o->cond_min_clr) != 0)
    logmsg(MSG_FATAL, "fscl: %s", fscl_amd_conditional_error());
  c->expect_sw = parse_sweeps(c->s, &o->expect_sweep, "expect-sweep");
  c->expect_req = malloc(sizeof *c->expect_req * (size_t)(o->expect_sweep.n > 0 ? o->expect_sweep.n : 1));
  if (!c->expect_req) logmsg(MSG_FATAL, "fscl: out of memory (expect sweeps)");
  for (i = 0; i < o->expect_sweep.n; i++) {
    c->expect_req[i].chr = c->expect_sw[i].chr; c->expect_req[i].pos = c->expect_sw[i].pos;
    c->expect_req[i].lalpha = log(c->expect_sw[i].alpha);
  }
  c->expect_n_la = o->expect_fname ? fscl_amd_surface_alphas(o->expect_grid.lo, o->expect_grid.hi, o->expect_grid.n, NAN, c->expect_la) : 0;
  if (o->expect_fname && fscl_amd_expect_check(c->s, c->expect_req, o->expect_sweep.n, c->expect_la, c->expect_n_la, o->expect_bins) != 0)
    logmsg(MSG_FATAL, "fscl: %s", fscl_amd_expect_error());
  if (o->fw_fname && fscl_amd_familywise_check(c->s, o->large_grid_sp, o->fw_trials) != 0)
    logmsg(MSG_FATAL, "fscl: --familywise-file: %s", fscl_amd_familywise_error());
}

/* the GPUs of this process and the permutation mode */
static void open_devices(const cli_opts_t *o) {
  const char *ws = cli_multi_rank(), *rk = getenv("RANK");
  if (ws) {
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
    if (o->n_gpus > 1) logmsg(MSG_WARN, "Warning: --n-gpus is ignored with one process per GPU (WORLD_SIZE=%s).\n", ws);
    if (fscl_amd_set_ranks_shm(atoi(rk), atoi(ws), name) != 0)
      logmsg(MSG_FATAL, "fscl: rank %s of %s could not meet the other ranks (%s)", rk, ws, name);
  } else if ((o->n_gpus > 0 || !getenv("FSCL_AMD_DEVICE")) && fscl_amd_set_devices(NULL, o->n_gpus) != 0)
    logmsg(MSG_FATAL, "fscl: --n-gpus=%d: at most 16 GPUs per process", o->n_gpus);
  if (o->throughput) {
    fscl_amd_set_permute_mode(FSCL_AMD_PERMUTE_THROUGHPUT, o->permute_seed ? strtoull(o->permute_seed, NULL, 0) : DEFAULT_SEED);
    logmsg(MSG_STATUS, "permutation test in throughput mode (counter-based random numbers; not the reference's stream)\n");
  }
}

/* ---- one step per output file; none draws from rand().  Those before the permutation test see the data as loaded ---- */

/* --simulate-file: one replicate under the model, at the data's own sites */
static void write_simulation(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  int *freq = malloc(sizeof(int) * (size_t)(c->s->n_snps > 0 ? c->s->n_snps : 1));
  unsigned long long n_deg = 0;
  scan_t *q;
  int r;
  if (!freq) logmsg(MSG_FATAL, "fscl: out of memory (simulation)");
  r = fscl_amd_simulate(c->s, c->sm, c->sim_sw, o->simulate_sweep.n, c->sim_seed, o->simulate_rep, freq, &n_deg);
  if (r != 0) logmsg(MSG_FATAL, "fscl: simulation failed (code %d)", r);
  q = fscl_amd_simulate_scan(c->s, freq);
  if (fscl_amd_simulate_output(o->simulate_fname, q) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", o->simulate_fname);
  logmsg(MSG_STATUS, "Simulation: %d sites, %d sweeps, replicate %d, %llu degenerate sites, kernel %.3f ms\n", c->s->n_snps,
         o->simulate_sweep.n, o->simulate_rep, n_deg, fscl_amd_simulate_last_ms());
  fscl_amd_scan_free(q);
  free(freq);
}

/* --profile-file: the likelihood profile at -g spacing */
static void write_profile(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  fscl_amd_profile_t *pf = fscl_amd_scan_profile(c->s, c->sm, EVAL_RANGE, o->small_grid_sp, o->large_grid_sp);
  int n_missed = 0;
  if (!pf) return;
  fscl_amd_profile_cell_max(pf, c->s, NULL, &n_missed);
  fscl_amd_profile_output(o->profile_fname, c->s, pf, prepend_label);
  logmsg(MSG_STATUS, "Profile: %d grid points at %d bp, kernel %.3f ms, %d of %d cells have a grid point above the bisection's maximum\n",
         pf->n_pts, o->small_grid_sp, fscl_amd_profile_last_ms(), n_missed, c->s->n_scan_pts);
  fscl_amd_profile_free(pf);
}

/* --alpha-file: the scan points' alpha curves */
static void write_alpha_curves(const cli_run_t *c) {
  scan_t *s = c->s;
  fscl_amd_curve_t *cv = malloc(sizeof *cv * (size_t)(s->n_scan_pts > 0 ? s->n_scan_pts : 1));
  int r;
  if (!cv) logmsg(MSG_FATAL, "fscl: out of memory (alpha curves)");
  r = fscl_amd_scan_point_curves(s, c->sm, EVAL_RANGE, cv);
  if (r != 0) logmsg(MSG_FATAL, "fscl: alpha curves failed (code %d)", r);
  fscl_amd_curve_output(c->o->alpha_fname, s, cv, s->n_scan_pts, c->o->alpha_drop, prepend_label);
  logmsg(MSG_STATUS, "Alpha curves: %d points, kernel %.3f ms, %llu walks summed sequentially for the curves alone\n",
         s->n_scan_pts, fscl_amd_curve_last_ms(), fscl_amd_curve_forced());
  free(cv);
}

/* --sites-file: the per-site terms of the scan points' walks */
static void write_sites(const cli_run_t *c) {
  fscl_amd_sites_t st;
  const int r = fscl_amd_scan_point_sites(c->s, c->sm, EVAL_RANGE, c->o->sites_top, &st);
  if (r != 0) logmsg(MSG_FATAL, "fscl: site terms failed (code %d)", r);
  fscl_amd_sites_output(c->o->sites_fname, c->s, &st, prepend_label);
  logmsg(MSG_STATUS, "Site terms: %d walks, %llu terms, kernel %.3f ms\n", st.n, (unsigned long long)st.n_terms,
         fscl_amd_sites_last_ms());
  fscl_amd_sites_free(&st);
}

/* --surface-file: the likelihood surfaces around the points of greatest CLR */
static void write_surfaces(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  fscl_amd_surfaces_t sf;
  const int r = fscl_amd_scan_point_surfaces(c->s, c->sm, EVAL_RANGE, o->surface_top, o->surface_halfwidth, o->surface_step,
                                             o->surface_grid.lo, o->surface_grid.hi, o->surface_grid.n, &sf);
  if (r != 0) logmsg(MSG_FATAL, "fscl: likelihood surfaces failed (code %d)", r);
  if (fscl_amd_surface_output(o->surface_fname, c->s, &sf, o->surface_drop, prepend_label) != 0)
    logmsg(MSG_FATAL, "fscl: cannot write %s", o->surface_fname);
  logmsg(MSG_STATUS, "Surfaces: %d points, %llu cells, %llu terms, kernel %.3f ms\n", sf.n, (unsigned long long)sf.n_cells,
         sf.n_terms, fscl_amd_surface_last_ms());
  fscl_amd_surfaces_free(&sf);
}

/* --jackknife-file: the delete-one-block jackknife of the points of greatest CLR */
static void write_jackknife(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  fscl_amd_blocks_t bk;
  const int r = fscl_amd_scan_point_jackknife(c->s, c->sm, EVAL_RANGE, o->jackknife_top, o->jackknife_halfwidth, o->jackknife_step,
                                              o->jackknife_grid.lo, o->jackknife_grid.hi, o->jackknife_grid.n, o->jackknife_block, &bk);
  if (r != 0) logmsg(MSG_FATAL, "fscl: jackknife failed (code %d)", r);
  if (fscl_amd_jackknife_output(o->jackknife_fname, c->s, &bk, prepend_label) != 0)
    logmsg(MSG_FATAL, "fscl: cannot write %s", o->jackknife_fname);
  logmsg(MSG_STATUS, "Jackknife: %d peaks, %llu block cells, %llu terms, kernel %.3f ms\n", bk.n, (unsigned long long)bk.n_cells,
         bk.n_terms, fscl_amd_blocks_last_ms());
  fscl_amd_blocks_free(&bk);
}

/* --conditional-file: the conditional sweep scan given fixed sweeps */
static void write_conditional(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  const scan_t *s = c->s;
  const fscl_amd_sweep_t *gsw = c->given_sw;
  fscl_amd_sweep_t top1;
  fscl_amd_conditional_t cd;
  int ng = o->given_sweep.n, r, i;
  if (ng == 0 && fscl_amd_top_points(s, 1, 0, NULL, &i) == 1) { /* the scan point of greatest CLR, at its fitted alpha */
    top1.chr = s->scan_pts[i].chr; top1.pos = s->scan_pts[i].sweep_pos; top1.alpha = exp(s->scan_pts[i].lalpha);
    gsw = &top1; ng = 1;
  }
  r = fscl_amd_scan_conditional(c->s, c->sm, EVAL_RANGE, gsw, ng, o->cond_halfwidth, o->cond_step, c->cond_la, c->cond_n_la,
                                o->cond_rounds, o->cond_min_clr, &cd);
  if (r != 0) logmsg(MSG_FATAL, "fscl: conditional scan failed (code %d): %s", r, fscl_amd_conditional_error());
  if (fscl_amd_conditional_output(o->cond_fname, s, &cd, prepend_label) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", o->cond_fname);
  logmsg(MSG_STATUS, "Conditional scan: %llu positions, %llu terms, kernel %.3f ms, base folds %.3f s\n",
         (unsigned long long)cd.n_rows, cd.n_terms, fscl_amd_conditional_last_ms(), cd.fold_s);
  fscl_amd_conditional_free(&cd);
}

/* --expect-file: what the model expects at the sweeps */
static void write_expectation(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  fscl_amd_expect_t ex;
  const int r = o->expect_sweep.n ? fscl_amd_scan_expect(c->s, c->sm, c->fsp, EVAL_RANGE, c->expect_req, o->expect_sweep.n, c->expect_la,
                                                         c->expect_n_la, o->expect_bins, &ex)
                                  : fscl_amd_scan_point_expect(c->s, c->sm, c->fsp, EVAL_RANGE, o->expect_top, o->large_grid_sp,
                                                               c->expect_la, c->expect_n_la, o->expect_bins, &ex);
  if (r != 0) logmsg(MSG_FATAL, "fscl: expectation failed (code %d): %s", r, fscl_amd_expect_error());
  if (fscl_amd_expect_output(o->expect_fname, c->s, &ex, prepend_label) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", o->expect_fname);
  logmsg(MSG_STATUS, "Expectation: %d sweeps, %d walks, kernel %.3f ms\n", ex.n, ex.n_tasks, fscl_amd_expect_last_ms());
  fscl_amd_expect_free(&ex);
}

/* --tail-file: the projected p-values, from the null CLRs the permutation test saved */
static void write_tail(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  fscl_amd_tail_t tl;
  const int r = fscl_amd_tail_fit(c->s, o->tail_df, o->tail_min_n, &tl);
  if (r != 0) logmsg(MSG_FATAL, "fscl: tail fit failed (code %d)", r);
  if (fscl_amd_tail_output(o->tail_fname, c->s, &tl, prepend_label) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", o->tail_fname);
  logmsg(MSG_STATUS, "Tail fit: df %d, %d fit, %d central, %d nofit, kernel %.3f ms (%.3f s in all); calibration over %d points "
                     "with permute_p >= 5: median log10(p_tail / p_empirical) = %.3f\n", o->tail_df, tl.n_fit, tl.n_central,
         tl.n_nofit, tl.kernel_ms, tl.wall_s, tl.n_calibration, tl.calibration);
  fscl_amd_tail_free(&tl);
}

/* --familywise-file: the family-wise adjusted p-values, from unpruned trials of their own; no record touched */
static void write_familywise(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  fscl_amd_familywise_t fw;
  const unsigned long long fw_seed = o->fw_seed_s ? strtoull(o->fw_seed_s, NULL, 0) : DEFAULT_SEED;
  const int r = fscl_amd_familywise(c->s, c->sm, o->fw_trials, fw_seed, o->permute_nbp, EVAL_RANGE, BP_RESL, o->large_grid_sp,
                                    o->scan_width_mb, 0, &fw);
  if (r != 0) logmsg(MSG_FATAL, "fscl: family-wise maxima failed (code %d): %s", r, fscl_amd_familywise_error());
  if (fscl_amd_familywise_output(o->fw_fname, c->s, &fw, prepend_label) != 0) logmsg(MSG_FATAL, "fscl: cannot write %s", o->fw_fname);
  if (o->fw_null_fname && fscl_amd_familywise_null_output(o->fw_null_fname, c->s, &fw, prepend_label) != 0)
    logmsg(MSG_FATAL, "fscl: cannot write %s", o->fw_null_fname);
  logmsg(MSG_STATUS, "Family-wise maxima: M %d unpruned trials of %d points, maxt kernel %.3f ms, %.3f s in all, %.0f grid points x "
                     "trials per second\n", fw.trials, fw.n, fw.kernel_ms, fw.wall_s,
         fw.wall_s > 0 ? (double)fw.n * (double)fw.trials / fw.wall_s : 0.0);
  fscl_amd_familywise_free(&fw);
}

/* --bootstrap-file: the parametric bootstrap, last: simulate under the sweeps, rescan, summarise */
static void write_bootstrap(cli_run_t *c) {
  const cli_opts_t *o = c->o;
  fscl_amd_boot_t *bt;
  double tm[5];
  int n_boot = o->bootstrap_sweep.n, r;
  if (n_boot == 0) { free(c->boot_sw); c->boot_sw = top_sweeps(c->s, o->bootstrap_top, o->bootstrap_window, &n_boot); }
  bt = malloc(sizeof *bt * ((size_t)n_boot * (size_t)o->bootstrap_reps + 1));
  if (!bt) logmsg(MSG_FATAL, "fscl: out of memory (bootstrap)");
  r = fscl_amd_bootstrap(c->s, c->sm, c->fsp, c->boot_sw, n_boot, o->bootstrap_reps, c->sim_seed, o->bootstrap_window, EVAL_RANGE,
                         BP_RESL, o->large_grid_sp, bt);
  if (r != 0) logmsg(MSG_FATAL, "fscl: bootstrap failed (code %d)", r);
  fscl_amd_bootstrap_output(o->bootstrap_fname, c->s, c->boot_sw, n_boot, o->bootstrap_reps, bt, prepend_label);
  fscl_amd_bootstrap_times(tm);
  logmsg(MSG_STATUS, "Bootstrap: %d sweeps, %d replicates, %.3f s (simulation %.3f s, null model %.3f s, upload %.3f s, "
                     "scan %.3f s)\n", n_boot, o->bootstrap_reps, tm[0], tm[1], tm[2], tm[3], tm[4]);
  free(bt);
}

/* ---- the scan, the permutation test and the output (fscl.c:316-337) ---- */

static void run_scan(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  if (o->grid_mode) {
    logmsg(MSG_STATUS, "scan mode grid: each cell's statistic is its maximum over the %d bp grid positions, in the scan "
                       "and in every permutation trial\n", o->small_grid_sp);
    fscl_amd_scan_chromosome_grid(c->s, c->sm, EVAL_RANGE, o->small_grid_sp, o->large_grid_sp);
  } else {
    scan_chromosome(c->s, c->sm, EVAL_RANGE, BP_RESL, o->large_grid_sp, o->n_threads);
  }
}

static void permute_and_output(const cli_run_t *c) {
  const cli_opts_t *o = c->o;
  if (n_permute > 0 && o->grid_mode)
    fscl_amd_scan_permute_grid(c->s, c->sm, n_permute, o->permute_nbp, EVAL_RANGE, o->small_grid_sp, o->large_grid_sp, o->scan_width_mb);
  else if (n_permute > 0)
    scan_permute(c->s, c->sm, n_permute, o->permute_nbp, o->alpha_factor, o->n_threads, EVAL_RANGE, BP_RESL, o->large_grid_sp,
                 o->scan_width_mb);
  if (o->ms_fname && o->maximum_only) output_block_maxima(output_fname, c->s, prepend_label);
  else scan_output(output_fname, c->s, o->maximum_only, n_permute, prepend_label);
}

static void finish(cli_run_t *c) {
  free(c->sim_sw); free(c->boot_sw); free(c->given_sw); free(c->expect_sw); free(c->expect_req);
  if (c->o->verbosity >= MSG_DEBUG1) {
    fscl_amd_stats_t st;
    fscl_amd_get_stats(&st);
    fprintf(stderr, "fscl_amd: scan %.3f s, permute %.3f s (host permutation %.3f s, %d trials), kernels %.3f s, "
                    "%llu grid-point evaluations, %llu terms, unsafe walks %llu, slow walks %llu, ties %llu, negj %llu\n",
            st.scan_s, st.permute_s, st.host_perm_s, st.trials, st.kernel_ms / 1e3, st.gp_evals, st.n_terms,
            st.n_unsafe, st.n_slow, st.n_ties, st.negj);
  }
  fscl_amd_shutdown();
}

int main(int argc, char **argv) {
  cli_opts_t o;
  cli_run_t c;
  int r, writer;

  init_log_table();
  r = cli_parse(argc, argv, &o);
  if (r >= 0) return r;
  if (cli_check(&o)) exit(-1);
  spline_pts = o.spline_pts; n_permute = o.n_permute; output_fname = o.output_fname; prepend_label = o.prepend_label;

  memset(&c, 0, sizeof c);
  c.o = &o;
  c.s = o.ms_fname ? fh_load_ms(o.ms_fname, o.ms_segment_length, o.ms_folded, o.ms_sample_first, o.ms_sample_size)
                   : load_snp_input(o.snp_fname, o.include_invariant, o.minimum_obs_depth);
  c.fsp = background_fsp(c.s, o.force_neutral, o.bs_fname, o.include_invariant);
  if (o.output_bs_fname) output_background_fs(o.output_bs_fname, c.s, c.fsp);
  if (o.dont_scan && !o.simulate_fname && !o.bootstrap_fname && !o.cond_fname && !o.expect_fname) return 0; /* no tables needed */

  parse_and_check(&c);
  open_devices(&o);
  c.sm = compute_sweep_model_tables(c.s, c.fsp, o.asc_depth, o.asc_min_freq, o.bg_only, o.include_invariant);
  compute_snp_null_model(c.s, c.fsp);

  /* with one process per GPU, rank 0 alone writes the analysis files (--profile-file has no such guard) */
  writer = cli_rank0();
  if (o.simulate_fname && writer) write_simulation(&c);
  if (!o.dont_scan) run_scan(&c); /* (--no-scan: tables only, for the simulation above and the explicit sweeps below) */
  if (o.profile_fname) write_profile(&c);
  if (o.alpha_fname && writer) write_alpha_curves(&c);
  if (o.sites_fname && writer) write_sites(&c);
  if (o.surface_fname && writer) write_surfaces(&c);
  if (o.jackknife_fname && writer) write_jackknife(&c);
  if (o.cond_fname && writer) write_conditional(&c);
  if (o.expect_fname && writer) write_expectation(&c);
  if (!o.dont_scan) permute_and_output(&c);
  if (o.tail_fname) write_tail(&c);
  if (o.fw_fname) write_familywise(&c);
  if (o.bootstrap_fname) write_bootstrap(&c);
  finish(&c);
  return 0;
}
