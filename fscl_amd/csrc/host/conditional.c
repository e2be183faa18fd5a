/* conditional.c -- the host-only side of the conditional sweep scan (--conditional-file): the
   sites a candidate sweep owns, the given sweeps' terms per site, the base fold, the size limit
   and the writer.  No device call is made here (fscl_amd_scan_conditional, analyses.c, evaluates);
   tools/conditional_host_check.c builds this file alone under the sanitizers. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fscl_host.h"

void fscl_amd_conditional_free(fscl_amd_conditional_t *r) {
  if (!r) return;
  free(r->blk); free(r->rows); free(r->given);
  memset(r, 0, sizeof *r);
}

size_t fscl_amd_conditional_cap(void) {
  const char *e = getenv("FSCL_AMD_COND_CAP");
  char *end = NULL;
  unsigned long long v;
  if (!e || !*e) return (size_t)1 << 30;
  v = strtoull(e, &end, 10);
  if (end == e || *end || v < 1) return (size_t)1 << 30;
  return (size_t)v;
}

static char g_cond_err[256];
const char *fscl_amd_conditional_error(void) { return g_cond_err; }

static int cond_refuse(const char *msg) {
  snprintf(g_cond_err, sizeof g_cond_err, "%s", msg);
  return -1;
}

int fscl_amd_conditional_check(const scan_t *s, const fscl_amd_sweep_t *given, int n_given, int halfwidth, int step,
                               const double *alphas, int n_la, int rounds, double min_clr) {
  double bytes = 0.;
  int *per_chr, i, c, round;
  g_cond_err[0] = 0;
  if (!s || n_given < 0 || (n_given && !given)) return cond_refuse("a NULL argument");
  if (step < 1) return cond_refuse("--conditional-step must be at least 1");
  if (halfwidth < 0) return cond_refuse("--conditional-halfwidth must be >= 0");
  if (rounds < 1 || rounds > FSCL_AMD_COND_MAX_ROUNDS) return cond_refuse("--conditional-rounds must be 1 .. 8");
  if (!(min_clr == min_clr)) return cond_refuse("--conditional-min-clr must be a number");
  if (!alphas || n_la < 1 || n_la > FSCL_AMD_SURFACE_MAX_LA)
    return cond_refuse("--conditional-alphas: 1 .. 64 ascending natural-log alphas within [-20, 4]");
  for (i = 0; i < n_la; i++)
    if (!(alphas[i] >= LOG_AD_MIN && alphas[i] <= LOG_AD_MAX) || (i && !(alphas[i] > alphas[i - 1])))
      return cond_refuse("--conditional-alphas: 1 .. 64 ascending natural-log alphas within [-20, 4]");
  per_chr = calloc((size_t)(s->n_chromosomes > 0 ? s->n_chromosomes : 1), sizeof *per_chr);
  if (!per_chr) return cond_refuse("out of memory");
  for (i = 0; i < n_given; i++) {
    const double la = given[i].alpha > 0.0 ? log(given[i].alpha) : NAN;
    if (given[i].chr < 0 || given[i].chr >= s->n_chromosomes) { free(per_chr); return cond_refuse("--given-sweep: unknown chromosome"); }
    if (!(la >= LOG_AD_MIN && la <= LOG_AD_MAX)) {
      free(per_chr);
      return cond_refuse("--given-sweep: alpha must be positive with its natural log within [-20, 4]");
    }
    if (++per_chr[given[i].chr] > FSCL_AMD_COND_MAX_GIVEN) {
      free(per_chr);
      return cond_refuse("--given-sweep: more than 64 given sweeps on one chromosome");
    }
  }
  for (c = 0; c < s->n_chromosomes; c++) { /* an upper bound of the result: every round's rows */
    const double whole = ((double)s->chr_limits[c].bp_length - s->chr_limits[c].start_pos) / step + 1.;
    if (!per_chr[c]) continue;
    for (round = 0; round < rounds; round++) {
      /* an interval of 2 halfwidth bp holds at most 2 halfwidth / step + 1 grid positions */
      const double near = (per_chr[c] + round) * (2. * (double)halfwidth / step + 1.);
      const double m = halfwidth > 0 && near < whole ? near : whole;
      if (m > 0.) bytes += m * (double)sizeof(fscl_amd_cond_row_t);
    }
    if ((double)s->chr_limits[c].bp_length > 2147483647. - 64.) {
      free(per_chr);
      return cond_refuse("--conditional-file: a position past the int range");
    }
  }
  free(per_chr);
  if (bytes > (double)fscl_amd_conditional_cap())
    return cond_refuse("--conditional-file: the result would exceed FSCL_AMD_COND_CAP bytes (raise --conditional-step or set "
                       "--conditional-halfwidth)");
  return 0;
}

/* search_snppos (scan-chromosome.c:39-56) on a chromosome's n sites */
static int nearest_site(const snp_t *a, int n, int pos) {
  int i = 0, j = n, m;
  while (j - i > 1) {
    m = (i + j) / 2;
    if (a[m].pos < pos) i = m; else j = m;
  }
  if (j == n) return n - 1;
  if ((long long)pos - a[i].pos < (long long)a[j].pos - pos) return i;
  return j;
}

/* the first index in [0, n) of a site with 2 * pos > twice (n: none) */
static int first_above(const snp_t *a, int n, long long twice) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = lo + (hi - lo) / 2;
    if (2 * (long long)a[m].pos > twice) hi = m; else lo = m + 1;
  }
  return lo;
}

int fscl_amd_cond_clip(const scan_t *s, const fscl_amd_sweep_t *given, int n_given, int chr, int pos, int *sweep_pos,
                       int *lo, int *hi) {
  const chr_limits_t *c;
  const snp_t *a;
  long long ql = 0, qr = 0;
  int i, near, n, has_l = 0, has_r = 0, same = 0;
  if (!s || !sweep_pos || !lo || !hi || n_given < 0 || (n_given && !given) || chr < 0 || chr >= s->n_chromosomes) return -1;
  c = s->chr_limits + chr;
  a = s->snps + c->start_index; n = c->n_snps;
  *lo = c->start_index; *hi = c->start_index + n - 1;
  if (n > 0) {
    near = c->start_index + nearest_site(a, n, pos);
    /* Q3: the de-collision compares a global index with the chromosome's count (scan-chromosome.c:58-101) */
    for (i = near; i < n && s->snps[i].pos == pos; i++) pos++;
  }
  *sweep_pos = pos;
  for (i = 0; i < n_given; i++) { /* the nearest given sweep on either side */
    const long long q = given[i].pos;
    if (given[i].chr != chr) continue;
    if (q == pos) same = 1;
    else if (q > pos) { if (!has_r || q < qr) { qr = q; has_r = 1; } }
    else if (!has_l || q > ql) { ql = q; has_l = 1; }
  }
  if (same || n <= 0) { *lo = c->start_index + 1; *hi = c->start_index; return 0; }
  if (has_r) *hi = c->start_index + first_above(a, n, (long long)pos + qr) - 1; /* 2x <= s + q */
  if (has_l) *lo = c->start_index + first_above(a, n, (long long)pos + ql);     /* 2x > s + q */
  return 0;
}

/* the given sweep that owns a site at pos: fscl_amd_nearest_sweep's rule (least distance, a tie to the
   lower position, then to the first listed), restated so that this file links alone */
static int owner_of(const fscl_amd_sweep_t *sw, int n, int chr, int pos) {
  long long bd = -1;
  int best = -1, k;
  for (k = 0; k < n; k++) {
    long long d;
    if (sw[k].chr != chr) continue;
    d = (long long)pos - sw[k].pos;
    if (d < 0) d = -d;
    if (best < 0 || d < bd || (d == bd && sw[k].pos < sw[best].pos)) { bd = d; best = k; }
  }
  return best;
}

int fscl_amd_cond_given_terms(const scan_t *s, const fscl_amd_sweep_t *given, int n_given, int chr,
                              const fscl_amd_site_hdr_t *hdr, const double *terms, double *g) {
  const chr_limits_t *c;
  int i;
  if (!s || !g || n_given < 0 || (n_given && (!given || !hdr)) || chr < 0 || chr >= s->n_chromosomes) return -1;
  c = s->chr_limits + chr;
  for (i = 0; i < c->n_snps; i++) {
    const int gi = c->start_index + i;
    const int q = owner_of(given, n_given, chr, s->snps[gi].pos);
    g[i] = 0.0;
    if (q < 0) continue;
    {
      const fscl_amd_site_hdr_t *h = hdr + q;
      const int near = h->pt.nearest_snp;
      if (h->len <= 0 || gi < near - h->nl || gi > near + h->nr) continue;
      if (!terms) return -1;
      g[i] = terms[h->off + (uint64_t)(gi == near ? 0 : (gi < near ? near - gi : h->nl + (gi - near)))];
    }
  }
  return 0;
}

double fscl_amd_cond_base(const double *g, int chr_start_index, int lo, int hi, int window_start, int window_end,
                          int *n_terms) {
  double acc = 0.0;
  int i;
  if (lo < window_start) lo = window_start;
  if (hi > window_end) hi = window_end;
  if (n_terms) *n_terms = hi >= lo ? hi - lo + 1 : 0;
  if (!g) return acc;
  for (i = lo; i <= hi; i++) {
    const double t = g[i - chr_start_index];
    if (t == 0.0) continue; /* a sum started at +0.0 is never -0.0: adding a zero changes nothing */
    acc = acc + t;
  }
  return acc;
}

static void put_pos(FILE *f, const scan_t *s, int site) {
  if (site < 0 || site >= s->n_snps) fprintf(f, "\tNA");
  else fprintf(f, "\t%d", s->snps[site].pos);
}

int fscl_amd_conditional_output(const char *fname, const scan_t *s, const fscl_amd_conditional_t *r, const char *label) {
  FILE *f = stdout;
  int b, p, k;
  if (!r || !s || r->n_blocks < 0 || (r->n_blocks && !r->blk)) return -1;
  for (b = 0; b < r->n_blocks; b++) { /* before anything is written */
    const fscl_amd_cond_block_t *h = r->blk + b;
    if (h->chr < 0 || h->chr >= s->n_chromosomes || h->n_pos < 0 || h->n_given < 0 || h->max_row >= h->n_pos ||
        h->row_off + (uint64_t)h->n_pos > r->n_rows || h->given_off + (uint64_t)h->n_given > r->n_given ||
        (h->n_pos && !r->rows) || (h->n_given && !r->given))
      return -1;
  }
  if (fname && !(f = fopen(fname, "w"))) return -1;
  for (b = 0; b < r->n_blocks; b++) {
    const fscl_amd_cond_block_t *h = r->blk + b;
    const char *name = s->chr_limits[h->chr].name;
    for (p = 0; p < h->n_pos; p++) {
      const fscl_amd_cond_row_t *q = r->rows + h->row_off + p;
      if (label) fprintf(f, "%s\t", label);
      fprintf(f, "%s\t%d\t%d\t%1.3e\t%1.2f", name, h->round, q->pos, exp(q->lalpha), q->cond_clr);
      if (q->lo > q->hi) fprintf(f, "\tNA\tNA");
      else { put_pos(f, s, q->lo); put_pos(f, s, q->hi); }
      fprintf(f, "\t%d\t%1.4f\n", q->n_terms, q->base);
    }
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\tsummary\t%d\t%d\t", name, h->round, h->n_pos, h->n_given);
    for (k = 0; k < h->n_given; k++) {
      const fscl_amd_sweep_t *w = r->given + h->given_off + k;
      fprintf(f, "%s%d:%1.3e", k ? "," : "", w->pos, w->alpha);
    }
    if (h->n_given == 0) fprintf(f, "NA");
    if (h->max_row < 0) fprintf(f, "\tNA\tNA\tNA");
    else {
      const fscl_amd_cond_row_t *q = r->rows + h->row_off + h->max_row;
      fprintf(f, "\t%d\t%1.3e\t%1.2f", q->pos, exp(q->lalpha), q->cond_clr);
    }
    fprintf(f, "\t%d\n", h->added ? 1 : 0);
  }
  if (fname && fclose(f) != 0) return -1;
  return 0;
}
