/* tail.c -- the host-only side of the projected p-values (include/fscl_amd.h): the used prefix of
 * every point's null record, the chunks of a launch, the packing of one chunk, the summary with its
 * calibration figure and the --tail-file writer.  Nothing here touches the device;
 * fscl_amd_tail_fit and fscl_amd_tail_runs are in analyses.c. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fscl_host.h"

int fscl_amd_tail_count(const scan_pt_t *p) {
  if (!p || !p->permute_clr || p->permute_n <= 0) return 0;
  return p->permute_n < FSCL_AMD_TAIL_SAVE ? p->permute_n : FSCL_AMD_TAIL_SAVE;
}

int fscl_amd_tail_chunk(const int32_t *counts, int n_points, int first, size_t cap) {
  size_t tot = 0;
  int n = 0;
  if (!counts || first < 0 || first >= n_points) return 0;
  while (first + n < n_points) {
    const size_t c = counts[first + n] > 0 ? (size_t)counts[first + n] : 0;
    if (n > 0 && (c > cap || tot > cap - c)) break;
    tot += c;
    n++;
  }
  return n;
}

size_t fscl_amd_tail_pack(const float *const *src, const int32_t *counts, int first, int n, float *buf,
                          unsigned long long *offsets) {
  size_t at = 0;
  int k;
  for (k = 0; k < n; k++) {
    const size_t c = counts[first + k] > 0 ? (size_t)counts[first + k] : 0;
    offsets[k] = at;
    if (c) memcpy(buf + at, src[first + k], sizeof(float) * c); /* in the record's own order */
    at += c;
  }
  return at;
}

/* the -o column's p-value (scan_output) */
static double p_empirical(const scan_pt_t *q) {
  return q->permute_p < 2 ? 1.0 / q->permute_n : (q->permute_p - 1.0) / (double)(q->permute_n - 1.0);
}

double fscl_amd_tail_log10p(const fsclg_tail_t *t) {
  if (!t || t->flag == FSCLG_TAIL_NOFIT || t->m <= 0) return NAN;
  return log10((double)t->m_pos / (double)t->m) + t->log10_q;
}

static int dbl_cmp(const void *va, const void *vb) {
  const double a = *(const double *)va, b = *(const double *)vb;
  return (a > b) - (a < b);
}

void fscl_amd_tail_summary(const scan_t *s, fscl_amd_tail_t *t) {
  double *d;
  int i, n = 0;
  if (!t) return;
  t->n_fit = t->n_central = t->n_nofit = 0;
  t->calibration = NAN; t->n_calibration = 0;
  if (!s || t->n <= 0 || !t->pt) return;
  d = fh_malloc(sizeof(double) * (size_t)t->n, "tail calibration");
  for (i = 0; i < t->n; i++) {
    const fsclg_tail_t *r = t->pt + i;
    const scan_pt_t *q = s->scan_pts + i;
    if (r->flag == FSCLG_TAIL_FIT) t->n_fit++;
    else if (r->flag == FSCLG_TAIL_CENTRAL) t->n_central++;
    else t->n_nofit++;
    if (r->flag != FSCLG_TAIL_NOFIT && q->permute_p >= 5 && q->permute_n > 1) {
      const double v = fscl_amd_tail_log10p(r) - log10(p_empirical(q));
      if (v == v && fabs(v) <= 1.7976931348623157e308) d[n++] = v;
    }
  }
  if (n) {
    qsort(d, (size_t)n, sizeof(double), dbl_cmp);
    t->calibration = n & 1 ? d[n / 2] : 0.5 * (d[n / 2 - 1] + d[n / 2]);
  }
  t->n_calibration = n;
  free(d);
}

void fscl_amd_tail_free(fscl_amd_tail_t *t) {
  if (!t) return;
  free(t->pt);
  memset(t, 0, sizeof *t);
}

int fscl_amd_tail_output(const char *fname, const scan_t *s, const fscl_amd_tail_t *t, const char *label) {
  static const char *const FLAG[3] = {"fit", "central", "nofit"};
  FILE *f = stdout;
  int i;
  if (!s || !t || t->n != s->n_scan_pts || (t->n && !t->pt)) return -1;
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open tail file \"%s\" (%s)\n", fname, strerror(errno)); return -1; }
  }
  for (i = 0; i < t->n; i++) {
    const scan_pt_t *q = s->scan_pts + i;
    const fsclg_tail_t *r = t->pt + i;
    const int fl = r->flag == FSCLG_TAIL_FIT || r->flag == FSCLG_TAIL_CENTRAL ? r->flag : FSCLG_TAIL_NOFIT;
    const double vr = r->variance / (2.0 * (t->df + 2.0 * r->lambda));
    const double lp = fscl_amd_tail_log10p(r);
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\t%1.2f\t%d\t%d\t%d\t", s->chr_limits[q->chr].name, q->sweep_pos, q->clr, q->permute_p, q->permute_n,
            r->m_pos);
    if (fl == FSCLG_TAIL_NOFIT || r->lambda != r->lambda) fprintf(f, "NA\tNA\t");
    else if (vr != vr || fabs(vr) > 1.7976931348623157e308) fprintf(f, "%1.4f\tNA\t", r->lambda);
    else fprintf(f, "%1.4f\t%1.3f\t", r->lambda, vr);
    if (q->permute_n > 0) fprintf(f, "%1.3f\t", -log10(p_empirical(q))); /* the -o column's expression */
    else fprintf(f, "NA\t");
    if (fl == FSCLG_TAIL_NOFIT || lp != lp) fprintf(f, "NA\t");
    else fprintf(f, "%1.3f\t", 0.0 - lp);
    fprintf(f, "%s\n", FLAG[fl]);
  }
  if (fname && fclose(f) != 0) return -1;
  return 0;
}
