/* familywise.c -- the host-only side of the family-wise adjusted p-values (--familywise-file,
 * include/fscl_amd.h): the rank order of the observed CLRs, the chunk of trials under a byte cap,
 * the combine of the exceedance counts into p-values, the thresholds and the two writers.  Nothing
 * here touches the device; fscl_amd_familywise and fscl_amd_familywise_runs are in trials.c;
 * tools/familywise_host_check.c builds this file alone under the sanitizers. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fscl_host.h"

static char g_fw_err[256];
const char *fscl_amd_familywise_error(void) { return g_fw_err; }
void fh_familywise_set_error(const char *msg) { snprintf(g_fw_err, sizeof g_fw_err, "%s", msg ? msg : ""); }

size_t fscl_amd_familywise_cap(void) {
  const char *e = getenv("FSCL_AMD_FWER_CAP");
  return e && atof(e) >= 1.0 ? (size_t)atof(e) : (size_t)1 << 28;
}

int fscl_amd_familywise_check(const scan_t *s, int large_grid_sp, int trials) {
  long long n = 0;
  int c;
  g_fw_err[0] = 0;
  if (!s) { fh_familywise_set_error("a NULL argument"); return -1; }
  if (trials < 1) { fh_familywise_set_error("--familywise-trials must be at least 1"); return -1; }
  if (large_grid_sp < 1) { fh_familywise_set_error("the coarse grid spacing must be positive"); return -1; }
  if (s->n_chromosomes > FSCLG_MAXT_MAX_GROUPS) {
    snprintf(g_fw_err, sizeof g_fw_err, "%d chromosomes: more than the %d the family-wise maxima take", s->n_chromosomes,
             FSCLG_MAXT_MAX_GROUPS);
    return -1;
  }
  for (c = 0; c < s->n_chromosomes; c++) { /* the scan's cells (scan_cells): one point each */
    const long long len = (long long)s->chr_limits[c].bp_length - (long long)s->chr_limits[c].start_pos;
    if (len > 0) n += (len + large_grid_sp - 1) / large_grid_sp;
  }
  if (n > 0x7fffffff || fscl_amd_familywise_chunk((int)n, trials, fscl_amd_familywise_cap()) < 1) {
    snprintf(g_fw_err, sizeof g_fw_err, "one trial of %lld points does not fit in FSCL_AMD_FWER_CAP=%zu bytes", n,
             fscl_amd_familywise_cap());
    return -1;
  }
  return 0;
}

void fscl_amd_familywise_free(fscl_amd_familywise_t *f) {
  if (!f) return;
  free(f->order); free(f->c_single); free(f->c_chr); free(f->c_step);
  free(f->gmax); free(f->garg); free(f->chr_max); free(f->chr_arg); free(f->matrix);
  memset(f, 0, sizeof *f);
}

/* observed CLR descending, ties by index ascending; a NaN after every number */
typedef struct { double v; int32_t i; } fw_key_t;
static int fw_key_cmp(const void *va, const void *vb) {
  const fw_key_t *a = va, *b = vb;
  const int an = a->v != a->v, bn = b->v != b->v;
  if (an != bn) return an - bn;
  if (!an && a->v != b->v) return a->v > b->v ? -1 : 1;
  return (a->i > b->i) - (a->i < b->i);
}

void fscl_amd_familywise_order(const double *obs, int n, int32_t *order) {
  fw_key_t *k;
  int i;
  if (n <= 0 || !obs || !order) return;
  k = fh_malloc(sizeof *k * (size_t)n, "familywise order");
  for (i = 0; i < n; i++) { k[i].v = obs[i]; k[i].i = i; }
  qsort(k, (size_t)n, sizeof *k, fw_key_cmp);
  for (i = 0; i < n; i++) order[i] = k[i].i;
  free(k);
}

int fscl_amd_familywise_chunk(int n, int trials, size_t cap_bytes) {
  const size_t row = sizeof(double) * (size_t)(n > 0 ? n : 1), b = cap_bytes / row;
  if (trials < 1) return 0;
  return b > (size_t)trials ? trials : (int)b;
}

void fscl_amd_familywise_combine(const int32_t *c_single, const int32_t *c_chr, const int32_t *c_step, const int32_t *order,
                                 int n, int trials, int32_t *rank, double *p_single, double *p_chr, double *p_step) {
  const double d = (double)trials + 1.0;
  int32_t run = 0;
  int j;
  for (j = 0; j < n; j++) { /* in rank order: the step-down value never falls */
    const int i = order[j];
    if (j == 0 || c_step[i] > run) run = c_step[i];
    if (rank) rank[i] = j + 1;
    if (p_single) p_single[i] = (1.0 + c_single[i]) / d;
    if (p_chr) p_chr[i] = (1.0 + c_chr[i]) / d;
    if (p_step) p_step[i] = (1.0 + run) / d;
  }
}

static int dbl_desc(const void *va, const void *vb) {
  const double a = *(const double *)va, b = *(const double *)vb;
  return (a < b) - (a > b);
}

/* k = floor(level (M + 1)): the most exceedances + 1 a significant point may have.  The product is
   nudged up by 1e-9 so that a level such as 0.05, whose double lies a hair off the decimal, keeps
   the k of the decimal when level (M + 1) is a whole number */
static int fw_k(int trials, double level) {
  const double x = floor(level * ((double)trials + 1.0) + 1e-9);
  if (!(x >= 1.0)) return 0;
  return x >= (double)trials ? trials : (int)x;
}

int fscl_amd_familywise_threshold(const double *maxima, int trials, double level, double *thr) {
  const int k = trials > 0 && maxima ? fw_k(trials, level) : 0;
  if (thr) *thr = NAN;
  if (k > 0 && thr) {
    double *d = fh_malloc(sizeof(double) * (size_t)trials, "familywise maxima");
    memcpy(d, maxima, sizeof(double) * (size_t)trials);
    qsort(d, (size_t)trials, sizeof(double), dbl_desc);
    *thr = d[k - 1];
    free(d);
  }
  return k;
}

static void put_num(FILE *f, double v, const char *fmt, const char *end) {
  if (v != v || fabs(v) > 1.7976931348623157e308) fprintf(f, "NA%s", end);
  else { fprintf(f, fmt, v); fputs(end, f); }
}

/* one summary row: the median and the thresholds of maxima[M] (stride apart), and the counts */
static void summary_row(FILE *f, const char *label, const char *name, const double *maxima, int stride, int M, int n_points,
                        int n05, int n01) {
  static const double LEVEL[3] = {0.10, 0.05, 0.01};
  double *d = fh_malloc(sizeof(double) * (size_t)(M > 0 ? M : 1), "familywise maxima"), q50 = NAN;
  int t, a;
  for (t = 0; t < M; t++) d[t] = maxima[(size_t)t * (size_t)stride];
  qsort(d, (size_t)M, sizeof(double), dbl_desc);
  if (M > 0) q50 = M & 1 ? d[M / 2] : 0.5 * (d[M / 2 - 1] + d[M / 2]);
  if (label) fprintf(f, "%s\t", label);
  fprintf(f, "%s\tsummary\t%d\t%d\t", name, M, n_points);
  put_num(f, q50, "%1.2f", "\t");
  for (a = 0; a < 3; a++) {
    const int k = M > 0 ? fw_k(M, LEVEL[a]) : 0;
    put_num(f, k > 0 ? d[k - 1] : NAN, "%1.2f", "\t");
  }
  fprintf(f, "%d\t%d\n", n05, n01);
  free(d);
}

static int fw_ok(const scan_t *s, const fscl_amd_familywise_t *r) {
  return s && r && r->n == s->n_scan_pts && r->n_groups == s->n_chromosomes && r->trials >= 1 &&
         (r->n == 0 || (r->order && r->c_single && r->c_chr && r->c_step)) && r->gmax && r->garg &&
         (r->n_groups == 0 || (r->chr_max && r->chr_arg));
}

int fscl_amd_familywise_output(const char *fname, const scan_t *s, const fscl_amd_familywise_t *r, const char *label) {
  FILE *f = stdout;
  const int n = r ? r->n : 0, M = r ? r->trials : 0;
  int32_t *rank, *mono;
  int *n_pts, *n05, *n01;
  int i, j, c, g05 = 0, g01 = 0, k05, k01;
  if (!fw_ok(s, r)) return -1;
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open familywise file \"%s\" (%s)\n", fname, strerror(errno)); return -1; }
  }
  rank = fh_malloc(sizeof *rank * (size_t)(n ? n : 1), "familywise ranks");
  mono = fh_malloc(sizeof *mono * (size_t)(n ? n : 1), "familywise ranks");
  n_pts = fh_calloc((size_t)(r->n_groups ? r->n_groups : 1) * 3, sizeof *n_pts, "familywise summary");
  n05 = n_pts + (r->n_groups ? r->n_groups : 1);
  n01 = n05 + (r->n_groups ? r->n_groups : 1);
  k05 = fw_k(M, 0.05); k01 = fw_k(M, 0.01);
  for (j = 0; j < n; j++) { /* the step-down counts, never falling in rank order */
    i = r->order[j];
    rank[i] = j + 1;
    mono[i] = j > 0 && mono[r->order[j - 1]] > r->c_step[i] ? mono[r->order[j - 1]] : r->c_step[i];
  }
  for (i = 0; i < n; i++) {
    const scan_pt_t *q = s->scan_pts + i;
    const double d = (double)M + 1.0, ps = (1.0 + mono[i]) / d;
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\t%1.2f\t%1.3e\t%d\t%1.3e\t%1.3e\t%1.3e\t%1.3f\n", s->chr_limits[q->chr].name, q->sweep_pos, q->clr,
            exp(q->lalpha), rank[i], (1.0 + r->c_chr[i]) / d, (1.0 + r->c_single[i]) / d, ps, 0.0 - log10(ps));
    /* p <= a exactly when 1 + c <= k (integers) */
    c = q->chr >= 0 && q->chr < r->n_groups ? q->chr : 0;
    n_pts[c]++;
    n05[c] += 1 + r->c_chr[i] <= k05; n01[c] += 1 + r->c_chr[i] <= k01;
    g05 += 1 + mono[i] <= k05; g01 += 1 + mono[i] <= k01;
  }
  for (c = 0; c < r->n_groups; c++)
    summary_row(f, label, s->chr_limits[c].name, r->chr_max + c, r->n_groups, M, n_pts[c], n05[c], n01[c]);
  summary_row(f, label, "genome", r->gmax, 1, M, n, g05, g01);
  free(rank); free(mono); free(n_pts);
  if (fname && fclose(f) != 0) return -1;
  return 0;
}

int fscl_amd_familywise_null_output(const char *fname, const scan_t *s, const fscl_amd_familywise_t *r, const char *label) {
  FILE *f = stdout;
  int t, c;
  if (!fw_ok(s, r)) return -1;
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open familywise null file \"%s\" (%s)\n", fname, strerror(errno)); return -1; }
  }
  for (t = 0; t < r->trials; t++) {
    const int a = r->garg[t];
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%d\t", t);
    put_num(f, r->gmax[t], "%1.4f", "\t");
    if (a >= 0 && a < r->n) fprintf(f, "%s\t%d", s->chr_limits[s->scan_pts[a].chr].name, s->scan_pts[a].sweep_pos);
    else fprintf(f, "NA\tNA");
    for (c = 0; c < r->n_groups; c++) {
      fputc('\t', f);
      put_num(f, r->chr_max[(size_t)t * (size_t)r->n_groups + c], "%1.4f", "");
    }
    fputc('\n', f);
  }
  if (fname && fclose(f) != 0) return -1;
  return 0;
}
