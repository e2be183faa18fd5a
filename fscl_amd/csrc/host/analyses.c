/* analyses.c -- the analysis drivers over scan.c's device state: profile, alpha curves, surfaces,
 * conditional scan, block sums, site terms, sampler and bootstrap, expected terms, tail fit.  Each
 * scan has its own g_*_ms, its *_runs test handle and its scan_point_* convenience entry; what
 * needs no device is in the host-only file of its name (surface.c, conditional.c, ...).
 */
#include <errno.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scan_internal.h"

/* the sampler's tables (fscl_amd_simulate): the context they went to (NULL: none) and their key */
static struct {
  fsclg_ctx *ctx;
  uint64_t hash;
  int n_depths;
  unsigned long long gen; /* uploads so far (the expect tables go with one) */
} SMP;

void fh_sampler_forget(void) { SMP.ctx = NULL; }

/* --------------------------------------------------------------- profile */
/* The fine grid (-g) of the reference's disabled loops (scan-chromosome.c:269-327): every
   small_grid_sp-spaced position of each chromosome over the extent its coarse cells cover, and
   the cell of each position.  Host only: no device is touched. */
int fscl_amd_profile_grid(const scan_t *s, int small_grid_sp, int large_grid_sp, int **chr_out, int **pos_out,
                          int **cell_out) {
  fsclg_cell_t *cells;
  int n_cells = 0, n = 0, cap = 1024, a, b;
  int *gc, *gp, *ge;
  if (chr_out) *chr_out = NULL;
  if (pos_out) *pos_out = NULL;
  if (cell_out) *cell_out = NULL;
  if (!s || small_grid_sp < 1 || large_grid_sp < 1 || large_grid_sp % small_grid_sp != 0) return -1;
  cells = fh_scan_cells(s, large_grid_sp, &n_cells);
  gc = fh_malloc(sizeof(int) * cap, "grid"); gp = fh_malloc(sizeof(int) * cap, "grid"); ge = fh_malloc(sizeof(int) * cap, "grid");
  for (a = 0; a < n_cells; a = b) { /* cells [a, b): one chromosome's */
    const int start = cells[a].start_pos;
    long long p;
    int end, k = a;
    for (b = a + 1; b < n_cells && cells[b].chr == cells[a].chr; b++) {}
    end = cells[b - 1].end_pos; /* the last cell's (clipped) end */
    for (p = start; p <= end; p += p + small_grid_sp <= end || p == end ? small_grid_sp : end - p) {
      /* the cell whose [start, end] holds p; a shared boundary belongs to the lower cell */
      while (k < b - 1 && p > cells[k].end_pos) k++;
      if (n == cap) {
        cap *= 2;
        gc = fh_realloc(gc, sizeof(int) * cap, "grid"); gp = fh_realloc(gp, sizeof(int) * cap, "grid");
        ge = fh_realloc(ge, sizeof(int) * cap, "grid");
      }
      gc[n] = cells[a].chr; gp[n] = (int)p; ge[n] = k;
      n++;
    }
  }
  free(cells);
  if (chr_out) *chr_out = gc; else free(gc);
  if (pos_out) *pos_out = gp; else free(gp);
  if (cell_out) *cell_out = ge; else free(ge);
  return n;
}

static double g_profile_ms;
double fscl_amd_profile_last_ms(void) { return g_profile_ms; }

/* init_scan_result + search_maxalpha at every position of the runs, on the data as loaded.  One
   device takes the runs as they are (fsclg_profile cuts them into the kernel's chunks).  Several
   devices: the chunks are dealt in contiguous cost-balanced shares (fscl_amd_partition's rule;
   cost: window size x positions), and each device gets its share as runs again -- a run the
   share boundary falls in is split there, at a chunk boundary -- so the chunks, and with them
   every point, are those of one device */
int fscl_amd_profile_runs(scan_t *s, sm_ptable_t *sm, const fsclg_run_t *runs, int n_runs, int eval_range,
                          fsclg_point_t *out) {
  const int CH = fsclg_profile_chunk();
  fsclg_run_t *dr;
  double *cost;
  int *crun;
  long long *coff;
  int lo[FH_MAX_DEV], hi[FH_MAX_DEV];
  int i, k, l, n = 0, cap = 0, r = FSCLG_OK;
  if (!s || !sm || (!runs && n_runs) || n_runs < 0) return FSCLG_E_ARG;
  fh_prepare(s, sm);
  for (i = 0; i < n_runs; i++) {
    if (runs[i].step < 1 || runs[i].count < 0 || runs[i].chr < 0 || runs[i].chr >= D.n_chr) return FSCLG_E_ARG;
    cap += (runs[i].count + CH - 1) / CH;
  }
  fh_set_original_rows();
  g_profile_ms = 0.;
  if (D.n_dev <= 1) {
    r = fsclg_profile(D.ctx[0], runs, n_runs, eval_range, out);
    g_profile_ms = fsclg_profile_last_ms(D.ctx[0]);
    return r;
  }
  cost = fh_malloc(sizeof(double) * (cap ? cap : 1), "profile chunks");
  crun = fh_malloc(sizeof(int) * (cap ? cap : 1), "profile chunks");           /* the chunk's run */
  coff = fh_malloc(sizeof(long long) * ((size_t)cap + 1), "profile chunks");  /* its first point in out */
  coff[0] = 0;
  for (i = 0; i < n_runs; i++)
    for (k = 0; k < runs[i].count; k += CH) {
      const int cnt = runs[i].count - k < CH ? runs[i].count - k : CH;
      cost[n] = fh_window_cost(runs[i].chr, eval_range) * cnt;
      crun[n] = i;
      coff[n + 1] = coff[n] + cnt;
      n++;
    }
  dr = fh_malloc(sizeof(fsclg_run_t) * ((size_t)n_runs + 2), "profile runs");
  for (l = 0; l < D.n_dev; l++) fscl_amd_partition(cost, n, l, D.n_dev, &lo[l], &hi[l]);
  for (l = 0; l < D.n_dev && r == FSCLG_OK; l++) {
    int nr = 0, c0;
    for (c0 = lo[l]; c0 < hi[l];) { /* chunks [c0, c1) of one run */
      const fsclg_run_t *q = runs + crun[c0];
      long long first = coff[c0], run0 = first; /* the run's first point: back to its first chunk */
      int c1 = c0, cb = c0;
      while (cb > 0 && crun[cb - 1] == crun[c0]) cb--;
      run0 = coff[cb];
      while (c1 < hi[l] && crun[c1] == crun[c0]) c1++;
      dr[nr].chr = q->chr; dr[nr].step = q->step;
      dr[nr].start_pos = (int)(q->start_pos + (first - run0) * q->step);
      dr[nr].count = (int)(coff[c1] - first);
      nr++;
      c0 = c1;
    }
    DBG("profile: device %d, chunks [%d, %d) as %d runs\n", D.dev[l], lo[l], hi[l], nr);
    r = fsclg_profile_submit(D.ctx[l], dr, nr, eval_range); /* (the runs are copied) */
  }
  for (k = 0; k < l; k++) {
    const int rw = fsclg_profile_wait(D.ctx[k], out + coff[lo[k] < n ? lo[k] : n]);
    const double ms = fsclg_profile_last_ms(D.ctx[k]);
    if (r == FSCLG_OK) r = rw;
    if (ms > g_profile_ms) g_profile_ms = ms; /* the devices run side by side */
  }
  free(dr); free(cost); free(crun); free(coff);
  return r;
}

fscl_amd_profile_t *fscl_amd_scan_profile(scan_t *s, sm_ptable_t *sm, int eval_range, int small_grid_sp,
                                          int large_grid_sp) {
  fscl_amd_profile_t *pf;
  fsclg_run_t *runs;
  fsclg_point_t *out;
  int *gc = NULL, n, i, a, nr = 0, r;
  if (D.world > 1 && D.rank != 0) return NULL; /* rank 0 alone evaluates and writes the profile */
  pf = fh_calloc(1, sizeof *pf, "profile");
  n = fscl_amd_profile_grid(s, small_grid_sp, large_grid_sp, &gc, &pf->grid_pos, &pf->cell);
  if (n < 0) logmsg(MSG_FATAL, "fscl_amd: profile: fine grid spacing %d must be positive and divide the coarse grid spacing %d",
                    small_grid_sp, large_grid_sp);
  pf->n_pts = n;
  /* maximal runs of equal step within a chromosome (the appended last point is a run of its own) */
  runs = fh_malloc(sizeof(fsclg_run_t) * (n ? n : 1), "profile runs");
  for (a = 0; a < n; a = i) {
    for (i = a + 1; i < n && gc[i] == gc[a] && pf->grid_pos[i] - pf->grid_pos[i - 1] == small_grid_sp; i++) {}
    runs[nr].chr = gc[a]; runs[nr].start_pos = pf->grid_pos[a]; runs[nr].step = small_grid_sp; runs[nr].count = i - a;
    nr++;
  }
  out = fh_malloc(sizeof(fsclg_point_t) * (n ? n : 1), "profile points");
  r = fscl_amd_profile_runs(s, sm, runs, nr, eval_range, out);
  fh_dev_check(r, "profile");
  pf->pts = fh_malloc(sizeof(scan_pt_t) * (n ? n : 1), "profile points");
  for (i = 0; i < n; i++) fh_to_scan_pt(pf->pts + i, out + i);
  free(out); free(runs); free(gc);
  return pf;
}

void fscl_amd_profile_free(fscl_amd_profile_t *pf) {
  if (!pf) return;
  free(pf->pts); free(pf->grid_pos); free(pf->cell);
  free(pf);
}

/* the strict maximum over the fine positions of each coarse cell, first wins
   (scan-chromosome.c:287): cell c's points are those with cell[] == c, preceded by the
   boundary point it shares with cell c - 1 of the same chromosome (that cell's last point) */
int fscl_amd_profile_cell_max(const fscl_amd_profile_t *pf, const scan_t *s, scan_pt_t *out_max, int *n_missed) {
  int i = 0, c, missed = 0;
  if (!pf || !s || !s->scan_pts || s->n_scan_pts <= 0) return -1;
  for (c = 0; c < s->n_scan_pts; c++) {
    int a, b, best;
    while (i < pf->n_pts && pf->cell[i] < c) i++;
    a = i;
    for (b = a; b < pf->n_pts && pf->cell[b] == c; b++) {}
    if (out_max) memset(out_max + c, 0, sizeof *out_max);
    if (a == b) continue;
    if (a > 0 && pf->cell[a - 1] == c - 1 && pf->pts[a - 1].chr == pf->pts[a].chr) a--;
    best = a;
    for (i = a + 1; i < b; i++)
      if (pf->pts[i].clr > pf->pts[best].clr) best = i;
    i = b;
    if (out_max) out_max[c] = pf->pts[best];
    if (pf->pts[best].clr > s->scan_pts[c].clr) missed++;
  }
  if (n_missed) *n_missed = missed;
  return s->n_scan_pts;
}

/* one line per grid point, scan_output's no-permutation row (scan-chromosome.c:741-745) */
void fscl_amd_profile_output(const char *fname, const scan_t *s, const fscl_amd_profile_t *pf, const char *label) {
  FILE *f = stdout;
  int i;
  if (!pf || !s) return;
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open profile file \"%s\" (%s)", fname, strerror(errno)); return; }
  }
  for (i = 0; i < pf->n_pts; i++) {
    const scan_pt_t *q = pf->pts + i;
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\t%1.2f\t%1.3e\t%d\t%d\t%d\n", s->chr_limits[q->chr].name, q->sweep_pos, q->clr, exp(q->lalpha),
            q->n_snps, s->snps[q->window_start].pos, s->snps[q->window_end].pos);
  }
  if (fname) fclose(f);
}

/* ------------------------------------------------------ alpha likelihood curves
   Every composite likelihood search_maxalpha evaluates at a position (fsclg_curve_submit), on
   the data as loaded.  Positions go to the device as runs of one; the local devices take
   contiguous shares balanced by window size, every device is submitted to before the first is
   waited for (the records are those of one device: a record depends on its position alone). */
static double g_curve_ms;
double fscl_amd_curve_last_ms(void) { return g_curve_ms; }

unsigned long long fscl_amd_curve_forced(void) {
  unsigned long long n = 0;
  int l;
  for (l = 0; l < D.n_dev; l++) n += fsclg_curve_forced(D.ctx[l]);
  return n;
}

static int curve_submit(int l, int lo, int hi, const dev_job_t *j) {
  return fsclg_curve_submit(D.ctx[l], 0, 0, j->runs + lo, hi - lo, j->eval_range); /* (the runs are copied) */
}
static int curve_wait(int k, int lo, const dev_job_t *j) { return fsclg_curve_wait(D.ctx[k], 0, j->curves + lo); }

int fscl_amd_scan_curves(scan_t *s, sm_ptable_t *sm, int eval_range, const int *chr, const int *pos, int n,
                         fscl_amd_curve_t *out) {
  dev_job_t job = {0};
  fsclg_run_t *runs;
  double *cost, dev_ms[FH_MAX_DEV] = {0.};
  int lo[FH_MAX_DEV], hi[FH_MAX_DEV], i, r;
  if (!s || !sm || n < 0 || (n && (!chr || !pos || !out))) return FSCLG_E_ARG;
  if (D.world > 1 && D.rank != 0) return FSCLG_OK; /* rank 0 alone evaluates, as the profile */
  fh_prepare(s, sm);
  for (i = 0; i < n; i++)
    if (chr[i] < 0 || chr[i] >= D.n_chr) return FSCLG_E_ARG;
  fh_set_original_rows();
  runs = fh_malloc(sizeof(fsclg_run_t) * (n ? n : 1), "curve runs");
  cost = fh_malloc(sizeof(double) * (n ? n : 1), "cost");
  for (i = 0; i < n; i++) {
    runs[i].chr = chr[i]; runs[i].start_pos = pos[i]; runs[i].step = 1; runs[i].count = 1;
    cost[i] = fh_window_cost(chr[i], eval_range);
  }
  fh_local_shares(cost, n, lo, hi);
  job.runs = runs; job.eval_range = eval_range; job.curves = out;
  r = fh_run_on_devices("curves", lo, hi, curve_submit, curve_wait, fsclg_curve_last_ms, &job, dev_ms, NULL);
  g_curve_ms = fh_dev_ms_max(dev_ms);
  free(runs); free(cost);
  return r;
}

int fscl_amd_scan_point_curves(scan_t *s, sm_ptable_t *sm, int eval_range, fscl_amd_curve_t *out) {
  int *cp, i, r, n;
  if (!s || !sm || !s->scan_pts || s->n_scan_pts < 0) return FSCLG_E_ARG;
  n = s->n_scan_pts;
  cp = fh_malloc(sizeof(int) * 2 * (size_t)(n ? n : 1), "curve positions");
  for (i = 0; i < n; i++) { cp[i] = s->scan_pts[i].chr; cp[n + i] = s->scan_pts[i].sweep_pos; }
  r = fscl_amd_scan_curves(s, sm, eval_range, cp, cp + n, n, out);
  free(cp);
  return r;
}

/* the test handle of fsclg_curve_submit / fsclg_curve_wait on the first device, for any runs: on
   the uploaded rows (rows NULL: slot 0, batch 0) or on `rows` (slot 1, batch 1), as
   fscl_amd_cellmax_runs */
int fscl_amd_curve_runs(scan_t *s, sm_ptable_t *sm, const fsclg_run_t *runs, int n_runs, int eval_range,
                        const uint32_t *rows, fscl_amd_curve_t *out) {
  int slot, r = fh_runs_handle_begin(s, sm, runs, n_runs, rows, &slot);
  if (r != FSCLG_OK) return r;
  g_curve_ms = 0.;
  r = fsclg_curve_submit(D.ctx[0], slot, slot, runs, n_runs, eval_range);
  if (r != FSCLG_OK) return r;
  r = fsclg_curve_wait(D.ctx[0], slot, out);
  g_curve_ms = fsclg_curve_last_ms(D.ctx[0], slot);
  return r;
}

/* the curve's distinct alphas in ascending order: idx[0 .. m) index la[] / sm[], an alpha
   evaluated twice (a coarse value that is also in the refine list) kept once, its first
   evaluation; *imax: where in idx the argmax is -- the first strict maximum of sm in evaluation
   order from -DBL_MAX, as search_maxalpha's two loops find it -- or -1 if no value beat
   -DBL_MAX (NaN never does).  Entries whose alpha is NaN are left out. */
static int curve_order(const fscl_amd_curve_t *c, int *idx, int *imax) {
  int n = c->n_coarse + c->n_refine, m = 0, k, j, best = -1;
  double bv = -DBL_MAX;
  if (n > FSCLG_CURVE_MAX) n = FSCLG_CURVE_MAX;
  if (n < 0) n = 0;
  for (k = 0; k < n; k++) {
    if (c->sm[k] > bv) { bv = c->sm[k]; best = k; }
    if (c->la[k] != c->la[k]) continue;
    for (j = 0; j < m && c->la[idx[j]] != c->la[k]; j++) {}
    if (j < m) continue; /* the same candidate again */
    for (j = m; j > 0 && c->la[idx[j - 1]] > c->la[k]; j--) idx[j] = idx[j - 1];
    idx[j] = k;
    m++;
  }
  *imax = -1;
  for (j = 0; best >= 0 && j < m; j++)
    if (c->la[idx[j]] == c->la[best]) *imax = j;
  return m;
}

int fscl_amd_curve_support(const fscl_amd_curve_t *c, double drop, double *la_lo, double *la_hi, int *open_lo,
                           int *open_hi) {
  int idx[FSCLG_CURVE_MAX], imax, m, a, b;
  double cut, nan_ = 0.0;
  nan_ = nan_ / nan_;
  if (la_lo) *la_lo = nan_;
  if (la_hi) *la_hi = nan_;
  if (open_lo) *open_lo = 0;
  if (open_hi) *open_hi = 0;
  if (!c || !(drop >= 0.0)) return -1;
  m = curve_order(c, idx, &imax);
  if (imax < 0) return 0;
  cut = c->sm[idx[imax]] - drop;
  for (a = imax; a > 0 && c->sm[idx[a - 1]] >= cut; a--) {}   /* (a NaN fails the comparison) */
  for (b = imax; b < m - 1 && c->sm[idx[b + 1]] >= cut; b++) {}
  if (la_lo) *la_lo = c->la[idx[a]];
  if (la_hi) *la_hi = c->la[idx[b]];
  if (open_lo) *open_lo = a == 0;
  if (open_hi) *open_hi = b == m - 1;
  return 1;
}

void fscl_amd_curve_output(const char *fname, const scan_t *s, const fscl_amd_curve_t *curves, int n, double drop,
                           const char *label) {
  FILE *f = stdout;
  int i, j;
  if (!curves || !s) return;
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open alpha curve file \"%s\" (%s)", fname, strerror(errno)); return; }
  }
  for (i = 0; i < n; i++) {
    const fscl_amd_curve_t *c = curves + i;
    const char *name = s->chr_limits[c->pt.chr].name;
    int idx[FSCLG_CURVE_MAX], imax, ol, oh;
    double lo, hi;
    const int m = curve_order(c, idx, &imax);
    for (j = 0; j < m; j++) {
      if (label) fprintf(f, "%s\t", label);
      fprintf(f, "%s\t%d\t%1.3e\t%1.2f\t%s\n", name, c->pt.sweep_pos, exp(c->la[idx[j]]),
              2.0 * (c->sm[idx[j]] - c->pt.null_logl), j == imax ? "*" : "-");
    }
    if (label) fprintf(f, "%s\t", label);
    if (fscl_amd_curve_support(c, drop, &lo, &hi, &ol, &oh) == 1)
      fprintf(f, "%s\t%d\tsupport\t%1.3e\t%1.3e\t%d\t%d\n", name, c->pt.sweep_pos, exp(lo), exp(hi), ol, oh);
    else
      fprintf(f, "%s\t%d\tsupport\tNA\tNA\t0\t0\n", name, c->pt.sweep_pos);
  }
  if (fname) fclose(f);
}

/* ------------------------------------------------------ likelihood surfaces
   The position-by-alpha surfaces of requests (fsclg_surface_submit), on the data as loaded.  A
   device call takes lists of one length, so the requests are evaluated one list length after
   another (the top-K helper's lists differ by one value at most); within a length the local
   devices take contiguous shares balanced by window size x cells, every device is submitted to
   before the first is waited for. */
static double g_surface_ms;
double fscl_amd_surface_last_ms(void) { return g_surface_ms; }

/* a list fsclg_surface_submit takes: 1 .. 64 values in [LOG_AD_MIN, LOG_AD_MAX], strictly ascending */
static int surface_list_ok(const double *la, int n) {
  int k;
  if (n < 1 || n > FSCL_AMD_SURFACE_MAX_LA) return 0;
  for (k = 0; k < n; k++)
    if (!(la[k] >= LOG_AD_MIN && la[k] <= LOG_AD_MAX) || (k && !(la[k] > la[k - 1]))) return 0;
  return 1;
}

static int surface_submit(int l, int lo, int hi, const dev_job_t *j) {
  return fsclg_surface_submit(D.ctx[l], 0, 0, j->runs + lo, hi - lo, j->la + (size_t)lo * j->n_la, j->n_la, j->eval_range);
}
static int surface_wait(int k, int lo, const dev_job_t *j) {
  return fsclg_surface_wait(D.ctx[k], 0, j->pts + j->poff[lo], j->val + j->poff[lo] * j->n_la);
}

int fscl_amd_scan_surface(scan_t *s, sm_ptable_t *sm, int eval_range, const fscl_amd_surface_req_t *req, int n,
                          fscl_amd_surfaces_t *out) {
  fsclg_run_t *runs;
  double *cost, dev_ms[FH_MAX_DEV] = {0.};
  int *idx, lo[FH_MAX_DEV], hi[FH_MAX_DEV], i, j, m, nla, r = FSCLG_OK;
  uint64_t po = 0, co = 0;
  if (!s || !sm || !out || n < 0 || (n && !req)) return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  if (D.world > 1 && D.rank != 0) return FSCLG_OK; /* rank 0 alone evaluates, as the curves */
  runs = fh_malloc(sizeof(fsclg_run_t) * (n ? n : 1), "surface runs");
  out->hdr = fh_calloc(n ? n : 1, sizeof *out->hdr, "surface headers");
  for (i = 0; i < n; i++) {
    fscl_amd_surface_hdr_t *h = out->hdr + i;
    if (!surface_list_ok(req[i].la, req[i].n_la) || fscl_amd_surface_run(s, req + i, runs + i) != 0) {
      free(runs); fscl_amd_surfaces_free(out);
      return FSCLG_E_ARG;
    }
    h->chr = req[i].chr; h->centre_pos = req[i].centre_pos; h->halfwidth = req[i].halfwidth; h->step = req[i].step;
    h->n_la = req[i].n_la; h->point = req[i].point; h->start_pos = runs[i].start_pos; h->n_pos = runs[i].count;
    memcpy(h->la, req[i].la, sizeof(double) * (size_t)h->n_la);
    h->pos_off = po; h->cell_off = co;
    po += (uint64_t)h->n_pos; co += (uint64_t)h->n_pos * (uint64_t)h->n_la;
  }
  fh_prepare(s, sm); /* (the requests are checked before the first device call) */
  out->n = n; out->n_pos = (size_t)po; out->n_cells = (size_t)co;
  out->pts = fh_calloc(po ? po : 1, sizeof *out->pts, "surface points");
  out->sm = fh_calloc(co ? co : 1, sizeof *out->sm, "surface values");
  fh_set_original_rows();
  idx = fh_malloc(sizeof(int) * (n ? n : 1), "surface requests");
  cost = fh_malloc(sizeof(double) * (n ? n : 1), "cost");
  for (nla = 1; nla <= FSCL_AMD_SURFACE_MAX_LA && r == FSCLG_OK; nla++) {
    dev_job_t job = {0};
    fsclg_run_t *gr;
    fsclg_point_t *gp;
    double *la, *gs;
    size_t *poff, np;
    for (i = 0, m = 0; i < n; i++)
      if (req[i].n_la == nla) { idx[m] = i; cost[m] = fh_window_cost(req[i].chr, eval_range) * runs[i].count * nla; m++; }
    if (m == 0) continue;
    gr = fh_malloc(sizeof *gr * (size_t)m, "surface runs");
    la = fh_malloc(sizeof(double) * (size_t)m * nla, "surface alphas");
    for (j = 0; j < m; j++) { gr[j] = runs[idx[j]]; memcpy(la + (size_t)j * nla, req[idx[j]].la, sizeof(double) * (size_t)nla); }
    poff = fh_run_offsets(gr, m);
    np = poff[m];
    gp = fh_malloc(sizeof *gp * (np ? np : 1), "surface points");
    gs = fh_malloc(sizeof(double) * (np ? np : 1) * nla, "surface values");
    fh_local_shares(cost, m, lo, hi);
    job.runs = gr; job.la = la; job.n_la = nla; job.eval_range = eval_range; job.poff = poff; job.pts = gp; job.val = gs;
    r = fh_run_on_devices("surfaces", lo, hi, surface_submit, surface_wait, fsclg_surface_last_ms, &job, dev_ms, &out->n_terms);
    for (j = 0; j < m && r == FSCLG_OK; j++) { /* back into request order */
      const fscl_amd_surface_hdr_t *h = out->hdr + idx[j];
      memcpy(out->pts + h->pos_off, gp + poff[j], sizeof *gp * (size_t)h->n_pos);
      memcpy(out->sm + h->cell_off, gs + poff[j] * nla, sizeof(double) * (size_t)h->n_pos * nla);
    }
    free(gr); free(la); free(poff); free(gp); free(gs);
  }
  g_surface_ms = fh_dev_ms_max(dev_ms); /* (a length after another on each device, the devices side by side) */
  free(runs); free(idx); free(cost);
  if (r != FSCLG_OK) fscl_amd_surfaces_free(out);
  return r;
}

/* the requests around the scan points of greatest CLR, `top` at most (fscl_amd_top_points, none
   within `halfwidth` of one already taken), each centred on its point with the point's lalpha
   inserted into the alpha grid.  Returns them malloc'd, *n_out their number; NULL: the grid was
   refused */
static fscl_amd_surface_req_t *top_peak_requests(const scan_t *s, int top, int halfwidth, int step, double la_lo,
                                                 double la_hi, int n_grid, int *n_out) {
  fscl_amd_surface_req_t *req = fh_calloc(top ? top : 1, sizeof *req, "peak requests");
  int *point = fh_calloc(top ? top : 1, sizeof *point, "peak requests");
  const int n = fscl_amd_top_points(s, top, halfwidth, NULL, point);
  int k;
  for (k = 0; k < n; k++) {
    const int best = point[k];
    req[k].chr = s->scan_pts[best].chr; req[k].centre_pos = s->scan_pts[best].sweep_pos;
    req[k].halfwidth = halfwidth; req[k].step = step; req[k].point = best;
    req[k].n_la = fscl_amd_surface_alphas(la_lo, la_hi, n_grid, s->scan_pts[best].lalpha, req[k].la);
    if (req[k].n_la < 1) { free(req); free(point); return NULL; }
  }
  free(point);
  *n_out = n;
  return req;
}

int fscl_amd_scan_point_surfaces(scan_t *s, sm_ptable_t *sm, int eval_range, int top, int halfwidth, int step,
                                 double la_lo, double la_hi, int n_grid, fscl_amd_surfaces_t *out) {
  fscl_amd_surface_req_t *req;
  int n, r;
  if (!s || !sm || !out || (!s->scan_pts && s->n_scan_pts) || s->n_scan_pts < 0 || top < 0 || halfwidth < 0 || step < 1)
    return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  req = top_peak_requests(s, top, halfwidth, step, la_lo, la_hi, n_grid, &n);
  if (!req) return FSCLG_E_ARG;
  r = fscl_amd_scan_surface(s, sm, eval_range, req, n, out);
  free(req);
  return r;
}

/* the test handle of fsclg_surface_submit / fsclg_surface_wait on the first device, for any runs
   and batch: on the uploaded rows (rows NULL: slot 0) or on `rows` (slot 1), as fscl_amd_cellmax_runs */
int fscl_amd_surface_runs(scan_t *s, sm_ptable_t *sm, const fsclg_run_t *runs, int n_runs, const double *la, int n_la,
                          int eval_range, const uint32_t *rows, int batch, fsclg_point_t *pts, double *smv) {
  int slot, r = fh_runs_handle_begin(s, sm, runs, n_runs, rows, &slot);
  if (r != FSCLG_OK) return r;
  g_surface_ms = 0.;
  r = fsclg_surface_submit(D.ctx[0], batch, slot, runs, n_runs, la, n_la, eval_range);
  if (r != FSCLG_OK) return r;
  r = fsclg_surface_wait(D.ctx[0], batch, pts, smv);
  g_surface_ms = fsclg_surface_last_ms(D.ctx[0], batch);
  return r;
}

/* ------------------------------------------------------ conditional sweep scan
   The likelihood ratio of one more sweep given fixed sweeps (fsclg_cond_submit), on the data as
   loaded.  Every refusal comes first, on the host.  Per round: the given sweeps' walks by
   fscl_amd_scan_sites and their terms per site; per chromosome with a given sweep the grid's
   positions in pieces of COND_PIECE, each position's clip from fscl_amd_cond_clip; the local
   devices take contiguous shares of the pieces balanced by window size x cells, all are
   submitted to before the first wait; then the base folds and the ratio on the host
   (conditional.c), one position after another. */
#define COND_PIECE 4096
static double g_cond_ms;
double fscl_amd_conditional_last_ms(void) { return g_cond_ms; }
static int cond_iv_cmp(const void *a, const void *b) {
  const long long *x = a, *y = b;
  return x[0] < y[0] ? -1 : (x[0] > y[0] ? 1 : 0);
}

/* the grid indices k of a chromosome's positions start_pos + k * step to evaluate, as merged ascending
   intervals iv[2 * i], iv[2 * i + 1] (at most n_given of them, or 1): the whole span [start_pos, bp_length]
   (halfwidth 0), or its part within halfwidth of a given sweep of the chromosome; returns their number */
static int cond_intervals(const scan_t *s, int chr, const fscl_amd_sweep_t *gv, int ng, int halfwidth, int step,
                          long long *iv) {
  const long long a = s->chr_limits[chr].start_pos, K = ((long long)s->chr_limits[chr].bp_length - a) / step;
  int i, n = 0, m = 0;
  if (s->chr_limits[chr].bp_length < a) return 0;
  if (halfwidth <= 0) { iv[0] = 0; iv[1] = K; return 1; }
  for (i = 0; i < ng; i++) {
    long long lo, hi;
    if (gv[i].chr != chr) continue;
    lo = (long long)gv[i].pos - halfwidth - a; hi = (long long)gv[i].pos + halfwidth - a;
    lo = lo <= 0 ? 0 : (lo + step - 1) / step;
    hi = hi < 0 ? -1 : hi / step;
    if (hi > K) hi = K;
    if (lo > hi) continue;
    iv[2 * n] = lo; iv[2 * n + 1] = hi; n++;
  }
  qsort(iv, (size_t)n, 2 * sizeof *iv, cond_iv_cmp);
  for (i = 0; i < n; i++) {
    if (m && iv[2 * i] <= iv[2 * m - 1] + 1) { if (iv[2 * i + 1] > iv[2 * m - 1]) iv[2 * m - 1] = iv[2 * i + 1]; }
    else { iv[2 * m] = iv[2 * i]; iv[2 * m + 1] = iv[2 * i + 1]; m++; }
  }
  return m;
}

static int cond_submit(int l, int lo, int hi, const dev_job_t *j) {
  return fsclg_cond_submit(D.ctx[l], 0, 0, j->runs + lo, hi - lo, j->la + (size_t)lo * j->n_la, j->n_la,
                           j->clip + 2 * j->poff[lo], j->eval_range);
}
static int cond_wait(int k, int lo, const dev_job_t *j) {
  return fsclg_cond_wait(D.ctx[k], 0, j->pts + j->poff[lo], j->val + j->poff[lo] * j->n_la);
}

int fscl_amd_scan_conditional(scan_t *s, sm_ptable_t *sm, int eval_range, const fscl_amd_sweep_t *given, int n_given,
                              int halfwidth, int step, const double *alphas, int n_la, int rounds, double min_clr,
                              fscl_amd_conditional_t *out) {
  fscl_amd_sweep_t *gv;
  long long iv[2 * (FSCL_AMD_COND_MAX_GIVEN + FSCL_AMD_COND_MAX_ROUNDS)];
  double dev_ms[FH_MAX_DEV] = {0.}, t0;
  size_t rows_cap = 0, given_cap = 0;
  int ng, i, j, c, round, r = FSCLG_OK, blk_cap = 0;
  if (!sm || !out) return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  if (fscl_amd_conditional_check(s, given, n_given, halfwidth, step, alphas, n_la, rounds, min_clr) != 0) return FSCLG_E_ARG;
  if (D.world > 1 && D.rank != 0) return FSCLG_OK; /* rank 0 alone evaluates, as the surfaces */
  ng = n_given;
  gv = fh_malloc(sizeof *gv * (size_t)(n_given + FSCL_AMD_COND_MAX_ROUNDS * (s->n_chromosomes > 0 ? s->n_chromosomes : 1)), "given sweeps");
  if (n_given) memcpy(gv, given, sizeof *gv * (size_t)n_given);
  for (round = 1; round <= rounds && r == FSCLG_OK; round++) {
    dev_job_t job = {0};
    fscl_amd_sites_t st;
    fsclg_site_req_t *req = fh_malloc(sizeof *req * (size_t)(ng ? ng : 1), "given walks");
    fsclg_run_t *runs = NULL;
    fsclg_point_t *pts;
    int32_t *clip, *want;
    int *run_chr_first; /* per chromosome: its first run, or -1 */
    double *cost, *lav, *smv, **g;
    size_t *poff, np, off;
    int n_runs = 0, run_cap = 0, lo[FH_MAX_DEV], hi[FH_MAX_DEV], added = 0, blk0 = out->n_blocks;
    for (i = 0; i < ng; i++) { req[i].chr = gv[i].chr; req[i].pos = gv[i].pos; req[i].lalpha = log(gv[i].alpha); }
    r = fscl_amd_scan_sites(s, sm, eval_range, req, ng, &st); /* (prepare, the original rows in slot 0) */
    free(req);
    if (r != FSCLG_OK) break;
    g = fh_calloc(s->n_chromosomes > 0 ? s->n_chromosomes : 1, sizeof *g, "given terms");
    run_chr_first = fh_malloc(sizeof(int) * (size_t)(s->n_chromosomes + 1), "runs");
    for (c = 0; c < s->n_chromosomes; c++) {
      int m, has = 0;
      run_chr_first[c] = n_runs;
      for (i = 0; i < ng; i++) has |= gv[i].chr == c;
      if (!has) continue;
      g[c] = fh_malloc(sizeof(double) * (size_t)(s->chr_limits[c].n_snps > 0 ? s->chr_limits[c].n_snps : 1), "given terms");
      if (fscl_amd_cond_given_terms(s, gv, ng, c, st.hdr, st.terms, g[c]) != 0) logmsg(MSG_FATAL, "fscl_amd: conditional scan: given terms");
      m = cond_intervals(s, c, gv, ng, halfwidth, step, iv);
      for (i = 0; i < m; i++) {
        long long k0;
        for (k0 = iv[2 * i]; k0 <= iv[2 * i + 1]; k0 += COND_PIECE) {
          const long long cnt = iv[2 * i + 1] - k0 + 1 < COND_PIECE ? iv[2 * i + 1] - k0 + 1 : COND_PIECE;
          if (n_runs == run_cap) { run_cap = run_cap ? 2 * run_cap : 64; runs = fh_realloc(runs, sizeof *runs * (size_t)run_cap, "runs"); }
          runs[n_runs].chr = c; runs[n_runs].start_pos = (int)(s->chr_limits[c].start_pos + k0 * step);
          runs[n_runs].step = step; runs[n_runs].count = (int)cnt;
          n_runs++;
        }
      }
    }
    run_chr_first[s->n_chromosomes] = n_runs;
    fscl_amd_sites_free(&st);
    poff = fh_run_offsets(runs, n_runs);
    np = poff[n_runs];
    clip = fh_malloc(sizeof(int32_t) * 2 * (np ? np : 1), "clips");
    want = fh_malloc(sizeof(int32_t) * (np ? np : 1), "positions");
    pts = fh_malloc(sizeof *pts * (np ? np : 1), "conditional points");
    smv = fh_malloc(sizeof(double) * (np ? np : 1) * (size_t)n_la, "conditional values");
    cost = fh_malloc(sizeof(double) * (size_t)(n_runs ? n_runs : 1), "cost");
    lav = fh_malloc(sizeof(double) * (size_t)(n_runs ? n_runs : 1) * (size_t)n_la, "alphas");
    for (i = 0, off = 0; i < n_runs; i++) {
      memcpy(lav + (size_t)i * n_la, alphas, sizeof(double) * (size_t)n_la);
      cost[i] = fh_window_cost(runs[i].chr, eval_range) * runs[i].count * n_la;
      for (j = 0; j < runs[i].count; j++, off++) {
        int sp, a, b;
        fscl_amd_cond_clip(s, gv, ng, runs[i].chr, runs[i].start_pos + j * runs[i].step, &sp, &a, &b);
        want[off] = sp; clip[2 * off] = a; clip[2 * off + 1] = b;
      }
    }
    fh_local_shares(cost, n_runs, lo, hi);
    job.runs = runs; job.la = lav; job.n_la = n_la; job.eval_range = eval_range; job.poff = poff; job.clip = clip;
    job.pts = pts; job.val = smv;
    r = fh_run_on_devices("conditional", lo, hi, cond_submit, cond_wait, fsclg_cond_last_ms, &job, dev_ms, &out->n_terms);
    if (r == FSCLG_OK) {
      for (off = 0; off < np; off++)
        if (pts[off].sweep_pos != want[off])
          logmsg(MSG_FATAL, "fscl_amd: conditional scan: the device evaluated position %d where the clip was computed for %d",
                 pts[off].sweep_pos, want[off]);
      if (out->n_rows + np > rows_cap) {
        rows_cap = out->n_rows + np;
        out->rows = fh_realloc(out->rows, sizeof *out->rows * (rows_cap ? rows_cap : 1), "conditional rows");
      }
      t0 = fh_now();
      {
        fscl_amd_cond_row_t *rows = out->rows + out->n_rows;
        long long q, nq = (long long)np;
        for (q = 0; q < nq; q++) {
          const fsclg_point_t *p = pts + q;
          fscl_amd_cond_row_t *w = rows + q;
          int nt = 0;
          memset(w, 0, sizeof *w);
          w->pos = p->sweep_pos; w->lo = clip[2 * q]; w->hi = clip[2 * q + 1];
          w->lalpha = p->lalpha; w->v = p->sm_logl; w->null_logl = p->null_logl;
          w->base = fscl_amd_cond_base(g[p->chr], s->chr_limits[p->chr].start_index, w->lo, w->hi, p->window_start, p->window_end, &nt);
          w->n_terms = nt;
          w->cond_clr = 2.0 * ((w->v - w->null_logl) - w->base);
        }
      }
      out->fold_s += fh_now() - t0;
      for (c = 0; c < s->n_chromosomes; c++) { /* one block per chromosome with a given sweep */
        fscl_amd_cond_block_t *h;
        const size_t row0 = out->n_rows + poff[run_chr_first[c]], nrow = poff[run_chr_first[c + 1]] - poff[run_chr_first[c]];
        int best = -1, m = 0;
        if (!g[c]) continue;
        if (out->n_blocks == blk_cap) { blk_cap = blk_cap ? 2 * blk_cap : 16; out->blk = fh_realloc(out->blk, sizeof *out->blk * (size_t)blk_cap, "conditional blocks"); }
        h = out->blk + out->n_blocks++;
        memset(h, 0, sizeof *h);
        for (i = 0; i < ng; i++) m += gv[i].chr == c;
        if (out->n_given + (size_t)m > given_cap) {
          given_cap = 2 * (out->n_given + (size_t)m);
          out->given = fh_realloc(out->given, sizeof *out->given * given_cap, "given sweeps");
        }
        h->chr = c; h->round = round; h->n_pos = (int)nrow; h->n_given = m; h->row_off = row0; h->given_off = out->n_given;
        for (i = 0; i < ng; i++)
          if (gv[i].chr == c) out->given[out->n_given++] = gv[i];
        for (i = 0; i < (int)nrow; i++) { /* the first position of greatest cond_clr, never a NaN */
          const double v = out->rows[row0 + i].cond_clr;
          if (v == v && (best < 0 || v > out->rows[row0 + best].cond_clr)) best = i;
        }
        h->max_row = best;
        h->added = best >= 0 && out->rows[row0 + best].cond_clr > min_clr;
      }
      out->n_rows += np;
      for (i = blk0; i < out->n_blocks; i++) { /* the rounds' maxima join the given sweeps */
        const fscl_amd_cond_block_t *h = out->blk + i;
        if (!h->added) continue;
        gv[ng].chr = h->chr; gv[ng].pos = out->rows[h->row_off + h->max_row].pos;
        gv[ng].alpha = exp(out->rows[h->row_off + h->max_row].lalpha);
        ng++; added++;
      }
    }
    for (c = 0; c < s->n_chromosomes; c++) free(g[c]);
    free(g); free(run_chr_first); free(runs); free(poff); free(clip); free(want); free(pts); free(smv); free(cost); free(lav);
    if (!added) break;
  }
  g_cond_ms = fh_dev_ms_max(dev_ms); /* (a round after another on each device, the devices side by side) */
  free(gv);
  if (r != FSCLG_OK) fscl_amd_conditional_free(out);
  return r;
}

/* the test handle of fsclg_cond_submit / fsclg_cond_wait on the first device: fscl_amd_surface_runs with
   the positions' clips */
int fscl_amd_cond_runs(scan_t *s, sm_ptable_t *sm, const fsclg_run_t *runs, int n_runs, const double *la, int n_la,
                       const int32_t *clip, int eval_range, const uint32_t *rows, int batch, fsclg_point_t *pts,
                       double *smv) {
  int slot, r = fh_runs_handle_begin(s, sm, runs, n_runs, rows, &slot);
  if (r != FSCLG_OK) return r;
  g_cond_ms = 0.;
  r = fsclg_cond_submit(D.ctx[0], batch, slot, runs, n_runs, la, n_la, clip, eval_range);
  if (r != FSCLG_OK) return r;
  r = fsclg_cond_wait(D.ctx[0], batch, pts, smv);
  g_cond_ms = fsclg_cond_last_ms(D.ctx[0], batch);
  return r;
}

/* ------------------------------------------------------ block sums (delete-one-block jackknife)
   The surface's terms summed per genomic block (fsclg_blocks_submit) for surface requests, on the
   data as loaded.  The size checks come first, on the host; then a surface evaluation of the same
   requests gives every position's window, hence each request's blocks; then the block sums, one
   list length after another and the local devices side by side, as the surfaces. */
static double g_blocks_ms;
double fscl_amd_blocks_last_ms(void) { return g_blocks_ms; }

static int blocks_submit(int l, int lo, int hi, const dev_job_t *j) {
  return fsclg_blocks_submit(D.ctx[l], 0, 0, j->runs + lo, hi - lo, j->la + (size_t)lo * j->n_la, j->n_la, j->blk + lo,
                             j->eval_range);
}
static int blocks_wait(int k, int lo, const dev_job_t *j) {
  return fsclg_blocks_wait(D.ctx[k], 0, j->pts + j->poff[lo], j->val + j->coff[lo], j->cnt + j->coff[lo]);
}

int fscl_amd_scan_blocks(scan_t *s, sm_ptable_t *sm, int eval_range, const fscl_amd_surface_req_t *req, int n,
                         int block_bp, fscl_amd_blocks_t *out) {
  fscl_amd_surfaces_t sf;
  fsclg_run_t *runs;
  fsclg_blocks_t *blk;
  double *cost, dev_ms[FH_MAX_DEV] = {0.};
  int *idx, lo[FH_MAX_DEV], hi[FH_MAX_DEV], i, j, m, nla, r = FSCLG_OK;
  uint64_t po = 0, co = 0;
  if (!s || !sm || !out || n < 0 || (n && !req) || block_bp < 1 || eval_range < 0) return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  if (D.world > 1 && D.rank != 0) return FSCLG_OK; /* rank 0 alone evaluates, as the surfaces */
  runs = fh_malloc(sizeof(fsclg_run_t) * (n ? n : 1), "block runs");
  for (i = 0; i < n; i++) { /* every refusal before the first device call */
    int b0, nb;
    if (!surface_list_ok(req[i].la, req[i].n_la) || fscl_amd_surface_run(s, req + i, runs + i) != 0 ||
        fscl_amd_blocks_bound(s, runs + i, eval_range, block_bp, &b0, &nb) != 0) {
      free(runs);
      return FSCLG_E_ARG;
    }
    if (nb > FSCL_AMD_BLOCKS_MAX_NB) {
      logmsg(MSG_ERROR, "Error: the jackknife of the peak at %d needs %d blocks of %d bp (at most %d): raise --jackknife-block.\n",
             req[i].centre_pos, nb, block_bp, FSCL_AMD_BLOCKS_MAX_NB);
      free(runs);
      return FSCLG_E_ARG;
    }
    co += (uint64_t)runs[i].count * (uint64_t)nb * (uint64_t)req[i].n_la;
  }
  if (co * (sizeof(double) + sizeof(uint32_t)) > (uint64_t)fscl_amd_blocks_cap()) {
    logmsg(MSG_ERROR, "Error: the jackknife's block sums take %llu bytes (limit %llu, $FSCL_AMD_BLOCKS_CAP): raise --jackknife-block "
                      "or --jackknife-step, or lower --jackknife-top, --jackknife-halfwidth or the count of --jackknife-alphas.\n",
           (unsigned long long)(co * (sizeof(double) + sizeof(uint32_t))), (unsigned long long)fscl_amd_blocks_cap());
    free(runs);
    return FSCLG_E_ARG;
  }
  r = fscl_amd_scan_surface(s, sm, eval_range, req, n, &sf); /* the windows of the positions */
  if (r != FSCLG_OK) { free(runs); return r; }
  out->hdr = fh_calloc(n ? n : 1, sizeof *out->hdr, "block headers");
  blk = fh_calloc(n ? n : 1, sizeof *blk, "blocks");
  for (i = 0, co = 0; i < n; i++) {
    fscl_amd_blocks_hdr_t *h = out->hdr + i;
    const fsclg_point_t *pt = sf.pts + sf.hdr[i].pos_off;
    int ws = -1, we = -1;
    for (j = 0; j < runs[i].count; j++) {
      if (ws < 0 || pt[j].window_start < ws) ws = pt[j].window_start;
      if (we < 0 || pt[j].window_end > we) we = pt[j].window_end;
    }
    h->chr = req[i].chr; h->centre_pos = req[i].centre_pos; h->halfwidth = req[i].halfwidth; h->step = req[i].step;
    h->n_la = req[i].n_la; h->point = req[i].point; h->start_pos = runs[i].start_pos; h->n_pos = runs[i].count;
    memcpy(h->la, req[i].la, sizeof(double) * (size_t)h->n_la);
    h->block_bp = block_bp; h->b0 = 0; h->nb = 1;
    if (ws >= 0) {
      const int a = s->snps[ws].pos / block_bp, b = s->snps[we].pos / block_bp;
      h->b0 = a < 0 ? 0 : a;
      h->nb = b - h->b0 + 1 < 1 ? 1 : b - h->b0 + 1;
      if (h->nb > FSCL_AMD_BLOCKS_MAX_NB) h->nb = FSCL_AMD_BLOCKS_MAX_NB; /* (the bound above covers these windows) */
    }
    blk[i].block_bp = block_bp; blk[i].b0 = h->b0; blk[i].nb = h->nb;
    h->pos_off = po; h->cell_off = co;
    po += (uint64_t)h->n_pos; co += (uint64_t)h->n_pos * (uint64_t)h->nb * (uint64_t)h->n_la;
  }
  fscl_amd_surfaces_free(&sf);
  out->n = n; out->n_pos = (size_t)po; out->n_cells = (size_t)co;
  out->pts = fh_calloc(po ? po : 1, sizeof *out->pts, "block points");
  out->bs = fh_calloc(co ? co : 1, sizeof *out->bs, "block sums");
  out->cnt = fh_calloc(co ? co : 1, sizeof *out->cnt, "block counts");
  idx = fh_malloc(sizeof(int) * (n ? n : 1), "block requests");
  cost = fh_malloc(sizeof(double) * (n ? n : 1), "cost");
  for (nla = 1; nla <= FSCL_AMD_SURFACE_MAX_LA && r == FSCLG_OK; nla++) {
    dev_job_t job = {0};
    fsclg_run_t *gr;
    fsclg_blocks_t *gb;
    fsclg_point_t *gp;
    double *la, *gs;
    uint32_t *gc;
    size_t *poff, *coff, np, ncell;
    for (i = 0, m = 0; i < n; i++)
      if (req[i].n_la == nla) { idx[m] = i; cost[m] = fh_window_cost(req[i].chr, eval_range) * runs[i].count * nla; m++; }
    if (m == 0) continue;
    gr = fh_malloc(sizeof *gr * (size_t)m, "block runs");
    gb = fh_malloc(sizeof *gb * (size_t)m, "blocks");
    la = fh_malloc(sizeof(double) * (size_t)m * nla, "block alphas");
    for (j = 0; j < m; j++) { gr[j] = runs[idx[j]]; gb[j] = blk[idx[j]]; memcpy(la + (size_t)j * nla, req[idx[j]].la, sizeof(double) * (size_t)nla); }
    poff = fh_run_offsets(gr, m);
    coff = fh_malloc(sizeof(size_t) * ((size_t)m + 1), "run offsets"); /* the cells before run j: positions x blocks x alphas */
    for (j = 0, coff[0] = 0; j < m; j++) coff[j + 1] = coff[j] + (size_t)gr[j].count * gb[j].nb * nla;
    np = poff[m]; ncell = coff[m];
    gp = fh_malloc(sizeof *gp * (np ? np : 1), "block points");
    gs = fh_malloc(sizeof(double) * (ncell ? ncell : 1), "block sums");
    gc = fh_malloc(sizeof(uint32_t) * (ncell ? ncell : 1), "block counts");
    fh_local_shares(cost, m, lo, hi);
    job.runs = gr; job.la = la; job.n_la = nla; job.eval_range = eval_range; job.poff = poff; job.coff = coff; job.blk = gb;
    job.pts = gp; job.val = gs; job.cnt = gc;
    r = fh_run_on_devices("blocks", lo, hi, blocks_submit, blocks_wait, fsclg_blocks_last_ms, &job, dev_ms, &out->n_terms);
    for (j = 0; j < m && r == FSCLG_OK; j++) { /* back into request order */
      const fscl_amd_blocks_hdr_t *h = out->hdr + idx[j];
      const size_t nc = coff[j + 1] - coff[j];
      memcpy(out->pts + h->pos_off, gp + poff[j], sizeof *gp * (size_t)h->n_pos);
      memcpy(out->bs + h->cell_off, gs + coff[j], sizeof(double) * nc);
      memcpy(out->cnt + h->cell_off, gc + coff[j], sizeof(uint32_t) * nc);
    }
    free(gr); free(gb); free(la); free(poff); free(coff); free(gp); free(gs); free(gc);
  }
  g_blocks_ms = fh_dev_ms_max(dev_ms); /* (as the surfaces) */
  free(runs); free(blk); free(idx); free(cost);
  if (r != FSCLG_OK) fscl_amd_blocks_free(out);
  return r;
}

int fscl_amd_scan_point_jackknife(scan_t *s, sm_ptable_t *sm, int eval_range, int top, int halfwidth, int step,
                                  double la_lo, double la_hi, int n_grid, int block_bp, fscl_amd_blocks_t *out) {
  fscl_amd_surface_req_t *req;
  int n, r;
  if (!s || !sm || !out || (!s->scan_pts && s->n_scan_pts) || s->n_scan_pts < 0 || top < 0 || halfwidth < 0 || step < 1 ||
      block_bp < 1)
    return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  req = top_peak_requests(s, top, halfwidth, step, la_lo, la_hi, n_grid, &n); /* the --surface-top points */
  if (!req) return FSCLG_E_ARG;
  r = fscl_amd_scan_blocks(s, sm, eval_range, req, n, block_bp, out);
  free(req);
  return r;
}

/* the test handle of fsclg_blocks_submit / fsclg_blocks_wait on the first device, as fscl_amd_surface_runs */
int fscl_amd_blocks_runs(scan_t *s, sm_ptable_t *sm, const fsclg_run_t *runs, int n_runs, const double *la, int n_la,
                         const fsclg_blocks_t *blk, int eval_range, const uint32_t *rows, int batch, fsclg_point_t *pts,
                         double *bs, uint32_t *cnt) {
  int slot, r = fh_runs_handle_begin(s, sm, runs, n_runs, rows, &slot);
  if (r != FSCLG_OK) return r;
  g_blocks_ms = 0.;
  r = fsclg_blocks_submit(D.ctx[0], batch, slot, runs, n_runs, la, n_la, blk, eval_range);
  if (r != FSCLG_OK) return r;
  r = fsclg_blocks_wait(D.ctx[0], batch, pts, bs, cnt);
  g_blocks_ms = fsclg_blocks_last_ms(D.ctx[0], batch);
  return r;
}

/* ------------------------------------------------------ per-site likelihood terms
   The terms of single sm_likelihood walks (fsclg_sites_submit), on the data as loaded.  The local
   devices take contiguous shares of the requests balanced by window size; every device is
   submitted to before the first is waited for.  A first wait with no room sizes the terms (the
   batch stays submitted), a second one fills each device's part of the one array. */
static double g_sites_ms;
double fscl_amd_sites_last_ms(void) { return g_sites_ms; }

void fscl_amd_sites_free(fscl_amd_sites_t *r) {
  if (!r) return;
  free(r->point); free(r->hdr); free(r->terms);
  memset(r, 0, sizeof *r);
}

int fscl_amd_scan_sites(scan_t *s, sm_ptable_t *sm, int eval_range, const fsclg_site_req_t *req, int n,
                        fscl_amd_sites_t *out) {
  double *cost;
  size_t nt[FH_MAX_DEV], base[FH_MAX_DEV], total = 0;
  int lo[FH_MAX_DEV], hi[FH_MAX_DEV], i, l, k, r = FSCLG_OK;
  if (!s || !sm || !out || n < 0 || (n && !req)) return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  if (D.world > 1 && D.rank != 0) return FSCLG_OK; /* rank 0 alone evaluates, as the curves */
  fh_prepare(s, sm);
  for (i = 0; i < n; i++)
    if (req[i].chr < 0 || req[i].chr >= D.n_chr) return FSCLG_E_ARG;
  fh_set_original_rows();
  g_sites_ms = 0.;
  cost = fh_malloc(sizeof(double) * (n ? n : 1), "cost");
  for (i = 0; i < n; i++) cost[i] = fh_window_cost(req[i].chr, eval_range);
  fh_local_shares(cost, n, lo, hi);
  for (l = 0; l < D.n_dev; l++) nt[l] = 0;
  free(cost);
  out->hdr = fh_malloc(sizeof(fscl_amd_site_hdr_t) * (n ? n : 1), "site headers");
  for (l = 0; l < D.n_dev && r == FSCLG_OK; l++) {
    DBG("sites: device %d, requests [%d, %d)\n", D.dev[l], lo[l], hi[l]);
    r = fsclg_sites_submit(D.ctx[l], 0, 0, req + lo[l], hi[l] - lo[l], eval_range); /* (the requests are copied) */
  }
  if (r != FSCLG_OK) l--; /* the submit that failed left nothing to wait for */
  for (k = 0; k < l; k++) { /* the sizes (the headers are ready once this returns) */
    const int rw = fsclg_sites_wait(D.ctx[k], 0, out->hdr + lo[k], NULL, 0, &nt[k]);
    if (rw != FSCLG_OK && !(rw == FSCLG_E_ARG && nt[k] > 0)) { nt[k] = (size_t)-1; if (r == FSCLG_OK) r = rw; }
    else if (rw == FSCLG_OK) nt[k] = (size_t)-2; /* no terms: that wait ended the batch */
  }
  for (k = 0; k < l; k++) {
    base[k] = total;
    if (nt[k] < (size_t)-2) total += nt[k];
  }
  out->terms = fh_malloc(sizeof(double) * (total ? total : 1), "site terms");
  for (k = 0; k < l; k++) {
    double ms;
    if (nt[k] < (size_t)-2) {
      const int rw = fsclg_sites_wait(D.ctx[k], 0, out->hdr + lo[k], out->terms + base[k], nt[k], NULL);
      if (r == FSCLG_OK) r = rw;
    }
    for (i = lo[k]; i < hi[k]; i++) out->hdr[i].off += base[k];
    ms = fsclg_sites_last_ms(D.ctx[k], 0);
    if (ms > g_sites_ms) g_sites_ms = ms; /* the devices run side by side */
  }
  out->n = n; out->n_terms = total;
  if (r != FSCLG_OK) fscl_amd_sites_free(out);
  return r;
}

int fscl_amd_scan_point_sites(scan_t *s, sm_ptable_t *sm, int eval_range, int top_k, fscl_amd_sites_t *out) {
  fsclg_site_req_t *req;
  int *pick, i, j, n, m, r;
  if (!s || !sm || !out || (!s->scan_pts && s->n_scan_pts) || s->n_scan_pts < 0 || top_k < 0) return FSCLG_E_ARG;
  n = s->n_scan_pts;
  m = top_k == 0 || top_k > n ? n : top_k;
  /* the m points of greatest CLR, ties in scan order (a NaN CLR ranks last): insertion into a list
     kept in descending order, then back into scan order */
  pick = fh_malloc(sizeof(int) * (size_t)(m ? m : 1), "site points");
  for (i = 0; m == n && i < n; i++) pick[i] = i; /* every point */
  for (i = 0, j = 0; m < n && i < n; i++) {
    const double v = s->scan_pts[i].clr;
    int k = j;
    while (k > 0 && v == v && !(s->scan_pts[pick[k - 1]].clr >= v)) k--;
    if (k >= m) continue;
    if (j < m) j++;
    memmove(pick + k + 1, pick + k, sizeof(int) * (size_t)(j - k - 1));
    pick[k] = i;
  }
  for (i = 1; i < m; i++) { /* ascending index */
    const int v = pick[i];
    for (j = i; j > 0 && pick[j - 1] > v; j--) pick[j] = pick[j - 1];
    pick[j] = v;
  }
  req = fh_malloc(sizeof(fsclg_site_req_t) * (size_t)(m ? m : 1), "site requests");
  for (i = 0; i < m; i++) {
    const scan_pt_t *q = s->scan_pts + pick[i];
    req[i].chr = q->chr; req[i].pos = q->sweep_pos; req[i].lalpha = q->lalpha;
  }
  r = fscl_amd_scan_sites(s, sm, eval_range, req, m, out);
  free(req);
  if (r == FSCLG_OK && out->hdr) out->point = pick; /* (not rank 0: nothing was evaluated) */
  else free(pick);
  return r;
}

/* term k of a walk belongs to site walk_site(h, k); site i of the walk holds term walk_term(h, i) */
static int walk_site(const fscl_amd_site_hdr_t *h, int k) {
  return k == 0 ? h->pt.nearest_snp : (k <= h->nl ? h->pt.nearest_snp - k : h->pt.nearest_snp + (k - h->nl));
}
static int walk_term(const fscl_amd_site_hdr_t *h, int i) {
  return i == h->pt.nearest_snp ? 0 : (i < h->pt.nearest_snp ? h->pt.nearest_snp - i : h->nl + (i - h->pt.nearest_snp));
}

typedef struct { double t; int k; } site_term_t;
static int site_term_cmp(const void *va, const void *vb) { /* descending term, then walk order */
  const site_term_t *a = va, *b = vb;
  if (a->t != b->t) return a->t > b->t ? -1 : 1;
  return a->k - b->k;
}

void fscl_amd_sites_summary(const scan_t *s, const fscl_amd_sites_t *r, fscl_amd_sites_summary_t *out) {
  int i, k;
  if (!s || !r || !out) return;
  for (i = 0; i < r->n; i++) {
    const fscl_amd_site_hdr_t *h = r->hdr + i;
    const double *t = r->terms + h->off;
    fscl_amd_sites_summary_t *o = out + i;
    double nan_ = 0.0, sum = 0.0, acc = 0.0;
    int top = -1, np = 0;
    nan_ = nan_ / nan_;
    memset(o, 0, sizeof *o);
    o->n_sites = h->len;
    o->first_pos = o->last_pos = o->top_pos = -1;
    o->top_term = o->top_share = nan_;
    if (h->len <= 0) continue;
    o->first_pos = s->snps[h->pt.nearest_snp - h->nl].pos;
    o->last_pos = s->snps[h->pt.nearest_snp + h->nr].pos;
    for (k = 0; k < h->len; k++) {
      if (t[k] > 0.0) o->n_pos++;
      if (t[k] < 0.0) o->n_neg++;
      if (t[k] == t[k] && (top < 0 || t[k] > t[top])) top = k; /* strict: the first in walk order wins; never a NaN */
    }
    if (top >= 0) {
      o->top_pos = s->snps[walk_site(h, top)].pos;
      o->top_term = t[top];
      if (h->pt.clr > 0.0) o->top_share = 2.0 * t[top] / h->pt.clr;
    }
    /* n_half: the positive terms in descending order (ties in walk order), summed one by one in
       that order; then the least count whose running sum, formed the same way, reaches half of it */
    if (o->n_pos > 0) {
      site_term_t *v = fh_malloc(sizeof *v * (size_t)o->n_pos, "positive terms");
      for (k = 0; k < h->len; k++)
        if (t[k] > 0.0) { v[np].t = t[k]; v[np].k = k; np++; }
      qsort(v, (size_t)np, sizeof *v, site_term_cmp);
      for (k = 0; k < np; k++) sum += v[k].t;
      for (k = 0; k < np; k++) {
        acc += v[k].t;
        if (acc >= 0.5 * sum) break;
      }
      o->n_half = k + 1;
      free(v);
    }
  }
}

/* sm-search.c:40-46 */
static double sites_logt(long long d) {
  if (d < 0) d = -d;
  if (d > 0xFFFFFF) return 11.783502069519070 + fh_log_table()[d >> 16];
  if (d > 0xFFFF) return 5.545177444479562 + fh_log_table()[d >> 8];
  return fh_log_table()[d];
}

void fscl_amd_sites_output(const char *fname, const scan_t *s, const fscl_amd_sites_t *r, const char *label) {
  FILE *f = stdout;
  fscl_amd_sites_summary_t *sum;
  int i, j;
  if (!r || !s) return;
  if (D.world > 1 && D.rank != 0) return; /* one writer */
  init_log_table();
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open site term file \"%s\" (%s)", fname, strerror(errno)); return; }
  }
  sum = fh_malloc(sizeof *sum * (size_t)(r->n > 0 ? r->n : 1), "site summaries");
  fscl_amd_sites_summary(s, r, sum);
  for (i = 0; i < r->n; i++) {
    const fscl_amd_site_hdr_t *h = r->hdr + i;
    const fscl_amd_sites_summary_t *o = sum + i;
    const char *name = s->chr_limits[h->pt.chr].name;
    for (j = h->pt.nearest_snp - h->nl; h->len > 0 && j <= h->pt.nearest_snp + h->nr; j++) {
      const snp_t *p = s->snps + j;
      if (label) fprintf(f, "%s\t", label);
      fprintf(f, "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%1.4f\t%1.4f\n", name, h->pt.sweep_pos, p->pos, p->pos - h->pt.sweep_pos,
              p->obs_freq, s->sample_depths[p->depth_p], p->folded,
              sites_logt((long long)h->pt.sweep_pos - p->pos) + h->pt.lalpha, r->terms[h->off + walk_term(h, j)]);
    }
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\tsummary\t%d\t", name, h->pt.sweep_pos, o->n_sites);
    if (h->len > 0) fprintf(f, "%d\t%d\t%d\t%d\t", o->first_pos, o->last_pos, o->n_pos, o->n_neg);
    else fprintf(f, "NA\tNA\t0\t0\t");
    if (o->top_pos >= 0) fprintf(f, "%d\t%1.4f\t", o->top_pos, o->top_term);
    else fprintf(f, "NA\tNA\t");
    if (o->top_share == o->top_share) fprintf(f, "%1.4f\t", o->top_share);
    else fprintf(f, "NA\t");
    fprintf(f, "%d\n", o->n_half);
  }
  free(sum);
  if (fname) fclose(f);
}

/* ------------------------------------------------------ sweep-model simulation, bootstrap
   fscl_amd_simulate draws one replicate on the first device (fsclg_sample_submit); the
   sampler's tables are kept per tables hash.  The host-only pieces are in simulate.c. */
static double g_sample_ms;
static double g_boot_s[5];
double fscl_amd_simulate_last_ms(void) { return g_sample_ms; }
void fscl_amd_bootstrap_times(double out[5]) { memcpy(out, g_boot_s, sizeof g_boot_s); }

/* the first device holds these positions and chromosome limits already (a replicate's are its
   original's): the sampler reads nothing else of the sites */
static int same_geometry(const scan_t *s) {
  int i;
  if (!D.n_dev || !D.snp_key || D.n_snps_key != s->n_snps || D.n_chr != s->n_chromosomes) return 0;
  for (i = 0; i < D.n_chr; i++)
    if (D.chr_start[i] != s->chr_limits[i].start_index || D.chr_n[i] != s->chr_limits[i].n_snps) return 0;
  for (i = 0; i < s->n_snps; i++)
    if (D.pos[i] != s->snps[i].pos) return 0;
  return 1;
}

/* the first device holds the sampler's tables of sm (kept per tables hash) */
static int sampler_tables(const scan_t *s, const sm_ptable_t *sm) {
  const uint64_t h = fh_tables_hash(sm, s->n_depths);
  int i, r;
  if (SMP.ctx != D.ctx[0] || SMP.hash != h || SMP.n_depths != s->n_depths) {
    double *coef_t, *neutral;
    int32_t *dn = fh_malloc(sizeof(int32_t) * (size_t)s->n_depths, "depths");
    int n_iv;
    fscl_amd_sample_tables_build(sm, s->n_depths, &coef_t, &neutral, dn, &n_iv);
    for (i = 0; i < s->n_depths; i++)
      if (dn[i] != s->sample_depths[i])
        logmsg(MSG_FATAL, "fscl_amd: sweep-model table %d is for depth %d, data has %d", i, dn[i], s->sample_depths[i]);
    SMP.ctx = NULL;
    r = fsclg_sample_tables(D.ctx[0], coef_t, neutral, dn, s->n_depths, n_iv, (LOG_AD_MAX - LOG_AD_MIN) / (n_iv + 1.));
    free(coef_t); free(neutral); free(dn);
    if (r != FSCLG_OK) return r;
    SMP.ctx = D.ctx[0]; SMP.hash = h; SMP.n_depths = s->n_depths; SMP.gen++;
  }
  return FSCLG_OK;
}

int fscl_amd_simulate(scan_t *s, sm_ptable_t *sm, const fscl_amd_sweep_t *sweeps, int n_sweeps,
                      unsigned long long seed, int rep, int *freq_out, unsigned long long *n_degenerate) {
  fsclg_sweep_t *sw;
  int32_t *depth;
  int i, r;
  if (!s || !sm || !freq_out || n_sweeps < 0 || (n_sweeps && !sweeps)) return FSCLG_E_ARG;
  for (i = 0; i < n_sweeps; i++)
    if (sweeps[i].chr < 0 || sweeps[i].chr >= s->n_chromosomes || !(sweeps[i].alpha > 0.0) ||
        sweeps[i].alpha > 1.7976931348623157e308)
      return FSCLG_E_ARG;
  if (n_degenerate) *n_degenerate = 0;
  if (D.world > 1 && D.rank != 0) return FSCLG_OK; /* rank 0 alone evaluates, as the other diagnostics */
  if (!same_geometry(s)) fh_prepare(s, sm);
  if ((r = sampler_tables(s, sm)) != FSCLG_OK) return r;
  depth = fh_malloc(sizeof(int32_t) * (size_t)(s->n_snps ? s->n_snps : 1), "site depths");
  sw = fh_malloc(sizeof(fsclg_sweep_t) * (size_t)(n_sweeps ? n_sweeps : 1), "sweeps");
  for (i = 0; i < s->n_snps; i++) depth[i] = s->snps[i].depth_p;
  for (i = 0; i < n_sweeps; i++) { sw[i].chr = sweeps[i].chr; sw[i].pos = sweeps[i].pos; sw[i].lalpha = log(sweeps[i].alpha); }
  r = fsclg_sample_submit(D.ctx[0], 0, depth, sw, n_sweeps, seed, rep);
  if (r == FSCLG_OK) {
    int32_t *f = fh_malloc(sizeof(int32_t) * (size_t)(s->n_snps ? s->n_snps : 1), "drawn counts");
    unsigned long long deg = 0;
    r = fsclg_sample_wait(D.ctx[0], 0, f, &deg);
    /* a degenerate site keeps its observed count */
    for (i = 0; r == FSCLG_OK && i < s->n_snps; i++) freq_out[i] = f[i] < 0 ? s->snps[i].obs_freq : f[i];
    if (r == FSCLG_OK && n_degenerate) *n_degenerate = deg;
    g_sample_ms = fsclg_sample_last_ms(D.ctx[0], 0);
    free(f);
  }
  free(depth); free(sw);
  return r;
}

int fscl_amd_bootstrap(scan_t *s, sm_ptable_t *sm, double **fsp, const fscl_amd_sweep_t *sweeps, int n_sweeps,
                       int reps, unsigned long long seed, int window_bp, int eval_range, int bp_resl, int large_grid_sp,
                       fscl_amd_boot_t *out) {
  const double t_all = fh_now();
  double nan_ = 0.0;
  int *freq;
  int rep, k, i, r = FSCLG_OK;
  if (!s || !sm || !fsp || n_sweeps < 0 || reps < 0 || (n_sweeps && !sweeps) || (n_sweeps && reps && !out))
    return FSCLG_E_ARG;
  if (D.world > 1) return FSCLG_E_STATE;
  nan_ = nan_ / nan_;
  memset(g_boot_s, 0, sizeof g_boot_s);
  freq = fh_malloc(sizeof(int) * (size_t)(s->n_snps ? s->n_snps : 1), "drawn counts");
  for (rep = 0; rep < reps && r == FSCLG_OK; rep++) {
    scan_t *q;
    double t0 = fh_now(), t1;
    r = fscl_amd_simulate(s, sm, sweeps, n_sweeps, seed, rep, freq, NULL);
    t1 = fh_now(); g_boot_s[1] += t1 - t0; t0 = t1;
    if (r != FSCLG_OK) break;
    q = fscl_amd_simulate_scan(s, freq);
    compute_snp_null_model(q, fsp);
    t1 = fh_now(); g_boot_s[2] += t1 - t0; t0 = t1;
    fh_prepare(q, sm); /* (timed on its own; scan_chromosome finds the replicate uploaded) */
    t1 = fh_now(); g_boot_s[3] += t1 - t0; t0 = t1;
    scan_chromosome(q, sm, eval_range, bp_resl, large_grid_sp, 1);
    g_boot_s[4] += fh_now() - t0;
    for (k = 0; k < n_sweeps; k++) {
      fscl_amd_boot_t *b = out + (size_t)k * (size_t)reps + rep;
      const scan_pt_t *best = NULL;
      for (i = 0; i < q->n_scan_pts; i++) {
        const scan_pt_t *p = q->scan_pts + i;
        long long d = (long long)p->sweep_pos - sweeps[k].pos;
        if (d < 0) d = -d;
        if (p->chr != sweeps[k].chr || d > window_bp) continue;
        if (!best || p->clr > best->clr) best = p; /* the first point wins a tie */
      }
      memset(b, 0, sizeof *b);
      b->sweep = k; b->rep = rep; b->chr = sweeps[k].chr; b->planted_pos = sweeps[k].pos;
      b->planted_alpha = sweeps[k].alpha;
      b->est_pos = best ? best->sweep_pos : -1;
      b->est_lalpha = best ? best->lalpha : nan_;
      b->clr = best ? best->clr : nan_;
    }
    fscl_amd_scan_free(q);
  }
  free(freq);
  g_boot_s[0] = fh_now() - t_all;
  return r;
}

/* ------------------------------------------------------ expected terms under the model (--expect-file)
   fscl_amd_scan_expect evaluates every (request, alpha) as one task of fsclg_expect_submit on the
   first device, on the data as loaded (slot 0).  The expect tables are kept per upload of the scan
   (prepare's key), of the sampler's tables and of the background spectra.  The host-only pieces
   are in expect.c. */
static double g_expect_ms;
static struct {
  fsclg_ctx *ctx;
  uint64_t key, fsp_hash;
  unsigned long long smp_gen;
} EXP;
double fscl_amd_expect_last_ms(void) { return g_expect_ms; }

static int expect_tables(const scan_t *s, const sm_ptable_t *sm, double **fsp) {
  double *fcoef, *neutral, *nu, *nf;
  int32_t *dn;
  uint32_t *cls;
  uint64_t fh = 1469598103934665603ull;
  int d, r, n_iv;
  if ((r = sampler_tables(s, sm)) != FSCLG_OK) return r;
  for (d = 0; d < s->n_depths; d++) fh = fh_hash_words(fsp[d], sizeof(double) * (size_t)(s->sample_depths[d] + 1), fh);
  if (EXP.ctx == D.ctx[0] && EXP.key == D.key && EXP.smp_gen == SMP.gen && EXP.fsp_hash == fh) return FSCLG_OK;
  dn = fh_malloc(sizeof(int32_t) * (size_t)s->n_depths, "depths");
  fscl_amd_expect_tables_build(sm, fsp, s->n_depths, &fcoef, &neutral, &nu, &nf, dn, &n_iv);
  /* the class of every device row: the depth of the sites that carry it, bit 31 for a folded row */
  cls = fh_calloc((size_t)D.rm.n_dev_rows, sizeof(uint32_t), "row classes");
  for (d = 0; d < D.rm.n_depths; d++) {
    const int n = D.rm.depth_n[d];
    for (r = 0; r <= n + n / 2 + 1; r++) {
      const int dr = D.rm.dev_row[D.rm.row_base[d] + r];
      if (dr >= 0) cls[dr] = (uint32_t)d | (r > n ? 0x80000000u : 0u);
    }
  }
  EXP.ctx = NULL;
  r = fsclg_expect_tables(D.ctx[0], fcoef, neutral, nu, nf, dn, s->n_depths, n_iv, (LOG_AD_MAX - LOG_AD_MIN) / (n_iv + 1.), cls,
                          D.rm.n_dev_rows);
  free(fcoef); free(neutral); free(nu); free(nf); free(dn); free(cls);
  if (r != FSCLG_OK) return r;
  EXP.ctx = D.ctx[0]; EXP.key = D.key; EXP.smp_gen = SMP.gen; EXP.fsp_hash = fh;
  return FSCLG_OK;
}

/* the test handle of fsclg_expect_submit / fsclg_expect_count / fsclg_expect_wait on the first device, for
   any batch: on the uploaded rows (slot 0).  *sites_out is malloc'd (n_sites records) when not NULL */
int fscl_amd_expect_runs(scan_t *s, sm_ptable_t *sm, double **fsp, const fsclg_site_req_t *req, int n_req, const double *la,
                         int n_la, int n_bins, int eval_range, int batch, fsclg_expect_tot_t *tot, fsclg_site_hdr_t *hdr,
                         fsclg_expect_site_t **sites_out, size_t *n_sites) {
  size_t ns = 0;
  fsclg_expect_site_t *sites = NULL;
  int r;
  if (!s || !sm || !fsp || n_req < 0) return FSCLG_E_ARG;
  if (sites_out) *sites_out = NULL;
  if (n_sites) *n_sites = 0;
  fh_prepare(s, sm);
  fh_set_original_rows();
  if ((r = expect_tables(s, sm, fsp)) != FSCLG_OK) return r;
  if ((r = fsclg_expect_submit(D.ctx[0], batch, 0, req, n_req, la, n_la, n_bins, eval_range)) != FSCLG_OK) return r;
  if ((r = fsclg_expect_count(D.ctx[0], batch, &ns)) != FSCLG_OK) return r;
  if (sites_out) sites = fh_malloc(sizeof *sites * (ns ? ns : 1), "expect site records");
  r = fsclg_expect_wait(D.ctx[0], batch, tot, hdr, sites, ns);
  g_expect_ms = fsclg_expect_last_ms(D.ctx[0], batch);
  if (r != FSCLG_OK) { free(sites); return r; }
  if (sites_out) *sites_out = sites;
  if (n_sites) *n_sites = ns;
  return FSCLG_OK;
}

int fscl_amd_scan_expect(scan_t *s, sm_ptable_t *sm, double **fsp, int eval_range, const fsclg_site_req_t *req, int n,
                         const double *la, int n_la, int n_bins, fscl_amd_expect_t *out) {
  fsclg_site_req_t *fr;
  double *fl;
  int i, k, r, nt = 0;
  if (!out) return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  if (fscl_amd_expect_check(s, req, n, la, n_la, n_bins) != 0) return FSCLG_E_ARG; /* (before any device work) */
  if (!sm || !fsp || eval_range < 0) return FSCLG_E_ARG;
  if (D.world > 1 && D.rank != 0) return FSCLG_OK; /* rank 0 alone evaluates, as the sampler */
  /* every request's own list: the shared one with the request's alpha inserted in order */
  out->n = n; out->n_bins = n_bins;
  out->req = fh_malloc(sizeof *out->req * (size_t)(n ? n : 1), "expect requests");
  out->first = fh_malloc(sizeof(int) * (size_t)(n + 1), "expect requests");
  out->own = fh_malloc(sizeof(int) * (size_t)(n ? n : 1), "expect requests");
  out->la = fh_malloc(sizeof(double) * (size_t)(n ? n : 1) * (size_t)(n_la + 1), "expect alphas");
  for (i = 0; i < n; i++) {
    int placed = 0;
    out->req[i] = req[i];
    out->first[i] = nt;
    for (k = 0; k < n_la; k++) {
      if (!placed && req[i].lalpha <= la[k]) {
        out->own[i] = nt - out->first[i];
        if (req[i].lalpha < la[k]) out->la[nt++] = req[i].lalpha;
        placed = 1;
      }
      out->la[nt++] = la[k];
    }
    if (!placed) { out->own[i] = nt - out->first[i]; out->la[nt++] = req[i].lalpha; }
  }
  out->first[n] = nt;
  out->n_tasks = nt;
  out->hdr = fh_malloc(sizeof *out->hdr * (size_t)(nt ? nt : 1), "expect headers");
  out->tot = fh_malloc(sizeof *out->tot * (size_t)(nt ? nt : 1) * (size_t)(n_bins + 1), "expect totals");
  fr = fh_malloc(sizeof *fr * (size_t)(nt ? nt : 1), "expect tasks");
  fl = out->la;
  for (i = 0; i < n; i++)
    for (k = out->first[i]; k < out->first[i + 1]; k++) { fr[k].chr = req[i].chr; fr[k].pos = req[i].pos; fr[k].lalpha = fl[k]; }
  fh_prepare(s, sm);
  fh_set_original_rows();
  g_expect_ms = 0.;
  r = expect_tables(s, sm, fsp);
  if (r == FSCLG_OK) r = fsclg_expect_submit(D.ctx[0], 0, 0, fr, nt, fl, 1, n_bins, eval_range);
  if (r == FSCLG_OK) {
    r = fsclg_expect_wait(D.ctx[0], 0, out->tot, out->hdr, NULL, 0);
    g_expect_ms = fsclg_expect_last_ms(D.ctx[0], 0);
  }
  out->kernel_ms = g_expect_ms;
  free(fr);
  if (r != FSCLG_OK) fscl_amd_expect_free(out);
  return r;
}

static int lalpha_in_range(const scan_pt_t *p) { return p->lalpha >= LOG_AD_MIN && p->lalpha <= LOG_AD_MAX; }

int fscl_amd_scan_point_expect(scan_t *s, sm_ptable_t *sm, double **fsp, int eval_range, int top, int spacing, const double *la,
                               int n_la, int n_bins, fscl_amd_expect_t *out) {
  fsclg_site_req_t *req;
  int *point;
  int n, k, r;
  if (!out) return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  if (!s || !sm || (!s->scan_pts && s->n_scan_pts) || s->n_scan_pts < 0 || top < 0 || spacing < 0) return FSCLG_E_ARG;
  req = fh_calloc(top ? top : 1, sizeof *req, "expect requests");
  point = fh_calloc(top ? top : 1, sizeof *point, "expect requests");
  n = fscl_amd_top_points(s, top, spacing, lalpha_in_range, point); /* --surface-top's rule, a fitted alpha the tables hold */
  for (k = 0; k < n; k++) {
    const int best = point[k];
    req[k].chr = s->scan_pts[best].chr; req[k].pos = s->scan_pts[best].sweep_pos; req[k].lalpha = s->scan_pts[best].lalpha;
  }
  r = fscl_amd_scan_expect(s, sm, fsp, eval_range, req, n, la, n_la, n_bins, out);
  free(req);
  if (r == FSCLG_OK && out->hdr) out->point = point;
  else free(point);
  return r;
}

/* ------------------------------------------------------ projected p-values (--tail-file)
   The device side of the noncentral chi-square fit: the points' records go to the first device
   chunk by chunk (fsclg_tail_submit).  The host-only pieces are in tail.c. */
static double g_tail_ms;
double fscl_amd_tail_last_ms(void) { return g_tail_ms; }

static int tail_drive(const float *const *src, const int32_t *counts, const double *x0, int n_points, int df, int min_n,
                      fsclg_tail_t *out) {
  const char *e = getenv("FSCL_AMD_TAIL_CAP");
  size_t cap = e && atof(e) >= 1.0 ? (size_t)atof(e) : (size_t)1 << 24, need = 1;
  unsigned long long *off;
  float *buf;
  int first = 0, r = FSCLG_OK, p;
  g_tail_ms = 0.0;
  if (df < 2 || (df & 1)) return FSCLG_E_ARG;
  if (n_points <= 0) return FSCLG_OK;
  fh_dev_open();
  if (cap > 0x7fffffffu) cap = 0x7fffffffu;
  for (p = 0; p < n_points; p++) { /* (a point larger than the cap is a chunk of its own) */
    if (counts[p] < 0) return FSCLG_E_ARG;
    if ((size_t)counts[p] > need) need = (size_t)counts[p];
  }
  buf = fh_malloc(sizeof(float) * (need > cap ? need : cap), "tail samples");
  off = fh_malloc(sizeof *off * (size_t)n_points, "tail offsets");
  while (first < n_points && r == FSCLG_OK) {
    const int n = fscl_amd_tail_chunk(counts, n_points, first, cap);
    const size_t tot = fscl_amd_tail_pack(src, counts, first, n, buf, off);
    r = fsclg_tail_submit(D.ctx[0], 0, buf, tot, off, counts + first, x0 + first, n, df, min_n);
    if (r == FSCLG_OK) r = fsclg_tail_wait(D.ctx[0], 0, out + first);
    g_tail_ms += fsclg_tail_last_ms(D.ctx[0], 0);
    first += n;
  }
  free(buf); free(off);
  return r;
}

int fscl_amd_tail_runs(const float *samples, size_t n_samples, const unsigned long long *offsets, const int32_t *counts,
                       const double *x0, int n_points, int df, int min_n, fsclg_tail_t *out) {
  const float **src;
  int p, r;
  if (n_points < 0 || (n_points && (!offsets || !counts || !x0 || !out)) || (n_samples && !samples)) return FSCLG_E_ARG;
  for (p = 0; p < n_points; p++)
    if (counts[p] < 0 || offsets[p] > n_samples || (size_t)counts[p] > n_samples - offsets[p]) return FSCLG_E_ARG;
  src = fh_malloc(sizeof *src * (size_t)(n_points ? n_points : 1), "tail records");
  for (p = 0; p < n_points; p++) src[p] = samples + offsets[p];
  r = tail_drive(src, counts, x0, n_points, df, min_n, out);
  free(src);
  return r;
}

int fscl_amd_tail_fit(scan_t *s, int df, int min_n, fscl_amd_tail_t *out) {
  const double t0 = fh_now();
  const float **src;
  int32_t *counts;
  double *x0;
  int i, r, n;
  if (!s || !out) return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  if (df < 2 || (df & 1)) return FSCLG_E_ARG;
  if (D.world > 1) return FSCLG_E_STATE;
  n = s->n_scan_pts > 0 ? s->n_scan_pts : 0;
  out->n = n; out->df = df; out->min_n = min_n;
  out->pt = fh_calloc((size_t)(n ? n : 1), sizeof *out->pt, "tail rows");
  src = fh_malloc(sizeof *src * (size_t)(n ? n : 1), "tail records");
  counts = fh_malloc(sizeof *counts * (size_t)(n ? n : 1), "tail counts");
  x0 = fh_malloc(sizeof *x0 * (size_t)(n ? n : 1), "tail observed");
  for (i = 0; i < n; i++) {
    src[i] = s->scan_pts[i].permute_clr;
    counts[i] = fscl_amd_tail_count(s->scan_pts + i);
    x0[i] = s->scan_pts[i].clr;
  }
  r = tail_drive(src, counts, x0, n, df, min_n, out->pt);
  free(src); free(counts); free(x0);
  out->kernel_ms = g_tail_ms;
  if (r == FSCLG_OK) fscl_amd_tail_summary(s, out);
  else fscl_amd_tail_free(out);
  out->wall_s = fh_now() - t0;
  return r;
}
