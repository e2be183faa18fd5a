/* surface.c -- the host-only side of the position-by-alpha likelihood surfaces (--surface-file):
   the alpha list of a request, its positions, the region summary and the writer.  No device call
   is made here (fscl_amd_scan_surface, analyses.c, evaluates); tools/surface_host_check.c builds this
   file alone under the sanitizers. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fscl_host.h"

int fscl_amd_surface_alphas(double lo, double hi, int n, double fitted, double *out) {
  int i, m = 0, placed = 0;
  if (!out || n < 1 || n > FSCL_AMD_SURFACE_MAX_LA - 1) return -1;
  if (!(lo >= LOG_AD_MIN && hi <= LOG_AD_MAX && lo <= hi)) return -1; /* (a NaN fails) */
  if (n > 1 && !(lo < hi)) return -1;
  if (n == 1 && lo != hi) return -1;
  if (!(fitted >= LOG_AD_MIN && fitted <= LOG_AD_MAX)) placed = 1; /* NaN or outside the range: nothing to insert */
  for (i = 0; i < n; i++) {
    const double g = i == n - 1 ? hi : lo + (double)i * ((hi - lo) / (double)(n - 1));
    if (!placed && fitted <= g) {
      if (fitted < g) out[m++] = fitted;
      placed = 1;
    }
    out[m++] = g;
  }
  if (!placed) out[m++] = fitted; /* above the grid */
  for (i = 1; i < m; i++)
    if (!(out[i] > out[i - 1])) return -1; /* a grid too fine for double */
  return m;
}

int fscl_amd_surface_run(const scan_t *s, const fscl_amd_surface_req_t *q, fsclg_run_t *run) {
  long long lo, hi, K, k0, k1;
  if (!s || !q || !run || q->chr < 0 || q->chr >= s->n_chromosomes || q->step < 1 || q->halfwidth < 0) return -1;
  lo = s->chr_limits[q->chr].start_pos;
  hi = s->chr_limits[q->chr].bp_length; /* the last cell's clipped end, as the profile's grid */
  K = q->halfwidth / q->step;
  /* the k with lo <= centre + k step <= hi (floor / ceiling divisions of either sign) */
  k0 = lo - q->centre_pos; k0 = k0 >= 0 ? (k0 + q->step - 1) / q->step : -((-k0) / q->step);
  k1 = hi - q->centre_pos; k1 = k1 >= 0 ? k1 / q->step : -((-k1 + q->step - 1) / q->step);
  if (k0 < -K) k0 = -K;
  if (k1 > K) k1 = K;
  run->chr = q->chr; run->step = q->step;
  run->count = k1 >= k0 ? (int)(k1 - k0 + 1) : 0;
  run->start_pos = run->count ? (int)(q->centre_pos + k0 * q->step) : q->centre_pos;
  return 0;
}

/* the peak selection of --surface-top, --jackknife-top, --expect-top and --bootstrap-top */
int fscl_amd_top_points(const scan_t *s, int top, int spacing, int (*accept)(const scan_pt_t *), int *idx_out) {
  char *used;
  int n = 0, i, k;
  if (!s || (!s->scan_pts && s->n_scan_pts > 0) || (top > 0 && !idx_out)) return -1;
  used = fh_calloc(s->n_scan_pts > 0 ? s->n_scan_pts : 1, 1, "top points");
  while (n < top) {
    int best = -1;
    for (i = 0; i < s->n_scan_pts; i++)
      if (!used[i] && s->scan_pts[i].clr == s->scan_pts[i].clr && (best < 0 || s->scan_pts[i].clr > s->scan_pts[best].clr))
        best = i;
    if (best < 0) break;
    used[best] = 1;
    for (k = 0; k < n; k++) {
      long long d = (long long)s->scan_pts[best].sweep_pos - s->scan_pts[idx_out[k]].sweep_pos;
      if (s->scan_pts[idx_out[k]].chr == s->scan_pts[best].chr && (d < 0 ? -d : d) <= spacing) break;
    }
    if (k < n) continue;
    if (accept && !accept(s->scan_pts + best)) continue;
    idx_out[n++] = best;
  }
  free(used);
  return n;
}

void fscl_amd_surfaces_free(fscl_amd_surfaces_t *r) {
  if (!r) return;
  free(r->hdr); free(r->pts); free(r->sm);
  memset(r, 0, sizeof *r);
}

/* V of cell (p, k); NaN where sm or the null sum is */
static double cell_v(const double *sm, const double *nul, int n_la, int p, int k) { return sm[(size_t)p * n_la + k] - nul[p]; }

int fscl_amd_surface_region(const double *sm, const double *null_logl, int n_pos, int n_la, double drop,
                            fscl_amd_surface_region_t *out, unsigned char *mark) {
  int p, k, bp = -1, bk = -1, top = 0, a, b, *stack;
  double M = 0.0, cut;
  unsigned char *in;
  if (!out) return -1;
  memset(out, 0, sizeof *out);
  out->max_ipos = out->max_ila = out->ipos_lo = out->ipos_hi = out->ila_lo = out->ila_hi = -1;
  out->max_v = NAN;
  if (!sm || !null_logl || n_pos < 1 || n_la < 1 || !(drop >= 0.0)) return -1;
  out->n_pos = n_pos; out->n_la = n_la;
  if (mark) memset(mark, 0, (size_t)n_pos * n_la);
  for (p = 0; p < n_pos; p++) /* the first maximum in position order, then alpha order */
    for (k = 0; k < n_la; k++) {
      const double v = cell_v(sm, null_logl, n_la, p, k);
      if (v == v && (bp < 0 || v > M)) { M = v; bp = p; bk = k; }
    }
  if (bp < 0) return 0; /* every cell NaN */
  cut = M - drop;
  out->max_ipos = bp; out->max_ila = bk; out->max_v = M;
  /* the 4-connected component of the cells at or above the cut that holds the argmax */
  in = mark ? mark : fh_calloc((size_t)n_pos * n_la, 1, "surface region");
  stack = fh_malloc(sizeof(int) * (size_t)n_pos * n_la, "surface region");
  in[(size_t)bp * n_la + bk] = 1;
  stack[top++] = bp * n_la + bk;
  while (top > 0) {
    static const int dp[4] = {-1, 1, 0, 0}, dk[4] = {0, 0, -1, 1};
    const int c = stack[--top], cp = c / n_la, ck = c % n_la;
    int d;
    out->n_region++;
    for (d = 0; d < 4; d++) {
      const int qp = cp + dp[d], qk = ck + dk[d];
      if (qp < 0 || qp >= n_pos || qk < 0 || qk >= n_la || in[(size_t)qp * n_la + qk]) continue;
      if (!(cell_v(sm, null_logl, n_la, qp, qk) >= cut)) continue; /* (a NaN fails the comparison) */
      in[(size_t)qp * n_la + qk] = 1;
      stack[top++] = qp * n_la + qk;
    }
  }
  free(stack);
  if (mark) mark[(size_t)bp * n_la + bk] = 2;
  else free(in);
  /* the run of positions (columns: alphas) around the argmax whose row (column) maximum reaches the cut */
  for (a = bp; a > 0; a--) {
    for (k = 0; k < n_la && !(cell_v(sm, null_logl, n_la, a - 1, k) >= cut); k++) {}
    if (k == n_la) break;
  }
  for (b = bp; b < n_pos - 1; b++) {
    for (k = 0; k < n_la && !(cell_v(sm, null_logl, n_la, b + 1, k) >= cut); k++) {}
    if (k == n_la) break;
  }
  out->ipos_lo = a; out->ipos_hi = b; out->open_pos_lo = a == 0; out->open_pos_hi = b == n_pos - 1;
  for (a = bk; a > 0; a--) {
    for (p = 0; p < n_pos && !(cell_v(sm, null_logl, n_la, p, a - 1) >= cut); p++) {}
    if (p == n_pos) break;
  }
  for (b = bk; b < n_la - 1; b++) {
    for (p = 0; p < n_pos && !(cell_v(sm, null_logl, n_la, p, b + 1) >= cut); p++) {}
    if (p == n_pos) break;
  }
  out->ila_lo = a; out->ila_hi = b; out->open_la_lo = a == 0; out->open_la_hi = b == n_la - 1;
  return 1;
}

int fscl_amd_surface_output(const char *fname, const scan_t *s, const fscl_amd_surfaces_t *r, double drop,
                            const char *label) {
  FILE *f = stdout;
  int i, p, k;
  if (!r || !s || !(drop >= 0.0)) return -1;
  for (i = 0; i < r->n; i++) { /* before anything is written */
    const fscl_amd_surface_hdr_t *h = r->hdr + i;
    if (h->chr < 0 || h->chr >= s->n_chromosomes || h->n_pos < 0 || h->n_la < 1 || h->n_la > FSCL_AMD_SURFACE_MAX_LA ||
        h->pos_off + (uint64_t)h->n_pos > r->n_pos || h->cell_off + (uint64_t)h->n_pos * (uint64_t)h->n_la > r->n_cells)
      return -1;
  }
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open surface file \"%s\" (%s)", fname, strerror(errno)); return -1; }
  }
  for (i = 0; i < r->n; i++) {
    const fscl_amd_surface_hdr_t *h = r->hdr + i;
    const char *name = s->chr_limits[h->chr].name;
    const fsclg_point_t *pts = r->pts + h->pos_off;
    const double *sm = r->sm + h->cell_off;
    const size_t nc = (size_t)h->n_pos * h->n_la;
    double *nul = fh_malloc(sizeof(double) * (h->n_pos ? h->n_pos : 1), "surface output");
    unsigned char *mark = fh_calloc(nc ? nc : 1, 1, "surface output");
    fscl_amd_surface_region_t g;
    int have;
    for (p = 0; p < h->n_pos; p++) nul[p] = pts[p].null_logl;
    have = fscl_amd_surface_region(sm, nul, h->n_pos, h->n_la, drop, &g, mark);
    for (p = 0; p < h->n_pos; p++)
      for (k = 0; k < h->n_la; k++) {
        const unsigned char m = mark[(size_t)p * h->n_la + k];
        if (label) fprintf(f, "%s\t", label);
        fprintf(f, "%s\t%d\t%d\t%1.3e\t%1.2f\t%s\n", name, h->centre_pos, pts[p].sweep_pos, exp(h->la[k]),
                2.0 * (sm[(size_t)p * h->n_la + k] - nul[p]), m == 2 ? "*" : (m ? "+" : "-"));
      }
    if (label) fprintf(f, "%s\t", label);
    if (have == 1)
      fprintf(f, "%s\t%d\tsummary\t%d\t%d\t%d\t%1.3e\t%1.2f\t%d\t%d\t%d\t%d\t%1.3e\t%1.3e\t%d\t%d\t%d\n", name, h->centre_pos,
              h->n_pos, h->n_la, pts[g.max_ipos].sweep_pos, exp(h->la[g.max_ila]), 2.0 * g.max_v, pts[g.ipos_lo].sweep_pos,
              pts[g.ipos_hi].sweep_pos, g.open_pos_lo, g.open_pos_hi, exp(h->la[g.ila_lo]), exp(h->la[g.ila_hi]),
              g.open_la_lo, g.open_la_hi, g.n_region);
    else
      fprintf(f, "%s\t%d\tsummary\t%d\t%d\tNA\tNA\tNA\tNA\tNA\t0\t0\tNA\tNA\t0\t0\t0\n", name, h->centre_pos, h->n_pos,
              h->n_la);
    free(nul); free(mark);
  }
  if (fname) fclose(f);
  return 0;
}
