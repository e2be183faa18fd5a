/* expect.c -- the host-only side of the expected terms under the model (--expect-file): the tables
   the sampler's lack (folded rows, null values per class), the refusals, the size limit and the
   writer.  No device call is made here (fscl_amd_scan_expect, analyses.c, evaluates);
   tools/expect_host_check.c builds this file alone under the sanitizers. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fscl_host.h"

void fscl_amd_expect_free(fscl_amd_expect_t *r) {
  if (!r) return;
  free(r->req); free(r->first); free(r->own); free(r->la); free(r->hdr); free(r->tot); free(r->point);
  memset(r, 0, sizeof *r);
}

size_t fscl_amd_expect_cap(void) {
  const char *e = getenv("FSCL_AMD_EXPECT_CAP");
  char *end = NULL;
  unsigned long long v;
  if (!e || !*e) return (size_t)1 << 30;
  v = strtoull(e, &end, 10);
  if (end == e || *end || v < 1) return (size_t)1 << 30;
  return (size_t)v;
}

static char g_expect_err[256];
const char *fscl_amd_expect_error(void) { return g_expect_err; }

static int expect_refuse(const char *msg) {
  snprintf(g_expect_err, sizeof g_expect_err, "%s", msg);
  return -1;
}

int fscl_amd_expect_check(const scan_t *s, const fsclg_site_req_t *req, int n, const double *la, int n_la, int n_bins) {
  double bytes;
  int i;
  g_expect_err[0] = 0;
  if (!s || n < 0 || (n && !req)) return expect_refuse("a NULL argument");
  if (n_bins < 1 || n_bins > FSCL_AMD_EXPECT_MAX_BINS) return expect_refuse("--expect-bins must be 1 .. 64");
  if (!la || n_la < 1 || n_la > FSCL_AMD_EXPECT_MAX_LA)
    return expect_refuse("--expect-alphas: 1 .. 64 ascending natural-log alphas within [-20, 4]");
  for (i = 0; i < n_la; i++)
    if (!(la[i] >= LOG_AD_MIN && la[i] <= LOG_AD_MAX) || (i && !(la[i] > la[i - 1])))
      return expect_refuse("--expect-alphas: 1 .. 64 ascending natural-log alphas within [-20, 4]");
  for (i = 0; i < n; i++) {
    if (req[i].chr < 0 || req[i].chr >= s->n_chromosomes) return expect_refuse("--expect-sweep: unknown chromosome");
    if (!(req[i].lalpha >= LOG_AD_MIN && req[i].lalpha <= LOG_AD_MAX))
      return expect_refuse("--expect-sweep: alpha must be positive with its natural log within [-20, 4]");
    if (req[i].pos > 2147483647 - 64) return expect_refuse("--expect-sweep: a position past the int range");
  }
  /* the result: per (request, alpha) a header and n_bins + 1 totals */
  bytes = (double)n * (double)(n_la + 1) *
          ((double)sizeof(fsclg_site_hdr_t) + (double)(n_bins + 1) * (double)sizeof(fsclg_expect_tot_t));
  if (bytes > (double)fscl_amd_expect_cap() || (double)n * (double)(n_la + 1) > 65535.)
    return expect_refuse("--expect-file: the result would exceed FSCL_AMD_EXPECT_CAP bytes (or 65535 walks): fewer sweeps, "
                         "alphas or bins");
  return 0;
}

void fscl_amd_expect_tables_build(const sm_ptable_t *sm, double **fsp, int n_depths, double **fcoef_out, double **neutral_out,
                                  double **null_unf_out, double **null_fold_out, int32_t *depth_n, int *n_iv_out) {
  const int n_iv = sm[0].spline_func[0]->n;
  size_t n_fold = 0, n_unf = 0, n_nf = 0, fo = 0, uo = 0, no = 0;
  double *fc, *ne, *nu, *nf;
  int d, f, iv;
  for (d = 0; d < n_depths; d++) {
    const int n = sm[d].sample_size;
    n_fold += (size_t)n_iv * (size_t)(n / 2) * 4;
    n_unf += (size_t)(n > 1 ? n - 1 : 0);
    n_nf += (size_t)(n / 2);
  }
  fc = fh_malloc(sizeof(double) * (n_fold ? n_fold : 1), "expect tables");
  ne = fh_malloc(sizeof(double) * (n_unf ? n_unf : 1), "expect tables");
  nu = fh_malloc(sizeof(double) * (n_unf ? n_unf : 1), "expect tables");
  nf = fh_malloc(sizeof(double) * (n_nf ? n_nf : 1), "expect tables");
  for (d = 0; d < n_depths; d++) {
    const int n = sm[d].sample_size, nh = n / 2;
    depth_n[d] = n;
    for (f = 1; f < n; f++) {
      ne[uo + (size_t)(f - 1)] = sm[d].fsp[f];
      nu[uo + (size_t)(f - 1)] = log(fsp[d][f]); /* compute_snp_null_model's unfolded branch */
    }
    for (f = 1; f <= nh; f++) {
      const spline_t *sp = sm[d].fspline_func[f];
      if (sp->n != n_iv) logmsg(MSG_FATAL, "fscl_amd: splines with different knot counts");
      for (iv = 0; iv < n_iv; iv++)
        memcpy(fc + fo + ((size_t)iv * (size_t)nh + (size_t)(f - 1)) * 4, sp->coef[iv], sizeof(double) * 4);
      /* compute_snp_null_model's folded branch */
      nf[no + (size_t)(f - 1)] = f != n - f ? log(fsp[d][f] + fsp[d][n - f]) : log(fsp[d][f]);
    }
    fo += (size_t)n_iv * (size_t)nh * 4;
    if (n > 1) uo += (size_t)(n - 1);
    no += (size_t)nh;
  }
  *fcoef_out = fc; *neutral_out = ne; *null_unf_out = nu; *null_fold_out = nf; *n_iv_out = n_iv;
}

int fscl_amd_expect_bin(double x, int n_bins) {
  int b;
  if (!(x >= LOG_AD_MIN)) return 0;
  if (x >= LOG_AD_MAX) return n_bins - 1; /* (no walk holds a site past the range; the cast below stays in range) */
  b = (int)(((x - LOG_AD_MIN) * (double)n_bins) / (LOG_AD_MAX - LOG_AD_MIN));
  return b < n_bins - 1 ? b : n_bins - 1;
}

static void put_num(FILE *f, const char *fmt, double v, int ok) {
  if (ok && v == v) fprintf(f, fmt, v);
  else fputs("NA", f);
}

int fscl_amd_expect_output(const char *fname, const scan_t *s, const fscl_amd_expect_t *r, const char *label) {
  FILE *f = stdout;
  int i, k, b;
  if (!r || !s) return -1;
  if (!r->hdr) return 0; /* (not rank 0: nothing was evaluated) */
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open expectation file \"%s\" (%s)", fname, strerror(errno)); return -1; }
  }
  for (i = 0; i < r->n; i++) {
    const int t0 = r->first[i], own = t0 + r->own[i], nb1 = r->n_bins + 1;
    const fsclg_site_hdr_t *h = r->hdr + own;
    const char *name = s->chr_limits[h->pt.chr].name;
    const double alpha = exp(r->req[i].lalpha), w = (LOG_AD_MAX - LOG_AD_MIN) / r->n_bins;
    const fsclg_expect_tot_t *T = r->tot + (size_t)own * (size_t)nb1 + r->n_bins;
    for (b = 0; b < nb1; b++) {
      const fsclg_expect_tot_t *o = r->tot + (size_t)own * (size_t)nb1 + b;
      const double obs = 2. * o->obs, es = 2. * o->e_s, ss = 2. * sqrt(o->v_s), e0 = 2. * o->e_0, s0 = 2. * sqrt(o->v_0);
      if (b < r->n_bins && o->n_sites == 0) continue; /* bins without sites are left out */
      if (b == r->n_bins) { /* the curve rows stand between the bins and the summary */
        for (k = t0; k < r->first[i + 1]; k++) {
          const fsclg_expect_tot_t *c = r->tot + (size_t)k * (size_t)nb1 + r->n_bins;
          const double ces = 2. * c->e_s, css = 2. * sqrt(c->v_s), ce0 = 2. * c->e_0, cs0 = 2. * sqrt(c->v_0);
          const double pooled = sqrt((css * css + cs0 * cs0) / 2.);
          if (label) fprintf(f, "%s\t", label);
          fprintf(f, "%s\t%d\t%1.3e\tcurve\t%1.3e\t%u\t%1.4f\t%1.4f\t%1.4f\t%1.4f\t", name, h->pt.sweep_pos, alpha,
                  exp(r->la[k]), c->n_sites, ces, css, ce0, cs0);
          put_num(f, "%1.4f", (ces - ce0) / pooled, pooled > 0.);
          fputc('\n', f);
        }
      }
      if (label) fprintf(f, "%s\t", label);
      fprintf(f, "%s\t%d\t%1.3e\t", name, h->pt.sweep_pos, alpha);
      if (b < r->n_bins) fprintf(f, "bin\t%1.4f\t%1.4f\t%u\t", LOG_AD_MIN + b * w, b == r->n_bins - 1 ? LOG_AD_MAX : LOG_AD_MIN + (b + 1) * w, o->n_sites);
      else fprintf(f, "summary\t%u\t%u\t", T->n_sites, T->n_degenerate);
      fprintf(f, "%1.4f\t%1.4f\t%1.4f\t", obs, es, ss);
      put_num(f, "%1.4f", (obs - es) / ss, ss > 0.);
      fprintf(f, "\t%1.4f\t%1.4f\t", e0, s0);
      put_num(f, "%1.4f", (obs - e0) / s0, s0 > 0.);
      if (b == r->n_bins) fprintf(f, "\t%1.3e\t%1.3e", T->max_lost_s, T->max_lost_0);
      fputc('\n', f);
    }
  }
  if (fname && fclose(f) != 0) return -1;
  return 0;
}
