/* simulate.c -- the host-only side of the sweep-model simulation and the parametric bootstrap
 * (include/fscl_amd.h): sweep parsing, the nearest-sweep rule, the sampler's table layout, the
 * replicate scan_t, the SNP-format writer and the bootstrap's quantile summary.  Nothing here
 * touches the device; fscl_amd_simulate and fscl_amd_bootstrap are in analyses.c. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fscl_host.h"

int fscl_amd_parse_sweep(const scan_t *s, const char *text, fscl_amd_sweep_t *out) {
  const char *c2, *c1;
  char *end;
  long pos;
  double alpha;
  int i;
  if (!s || !text || !out) return -1;
  c2 = strrchr(text, ':');
  if (!c2 || c2 == text) return -1;
  for (c1 = c2 - 1; c1 > text && *c1 != ':'; c1--) {}
  if (*c1 != ':' || c1 == text) return -1; /* (an empty name is malformed too) */
  errno = 0;
  pos = strtol(c1 + 1, &end, 10);
  if (end == c1 + 1 || end != c2 || errno || pos < -2147483647L || pos > 2147483647L) return -1;
  alpha = strtod(c2 + 1, &end);
  if (end == c2 + 1 || *end) return -1;
  for (i = 0; i < s->n_chromosomes; i++) {
    const char *nm = s->chr_limits[i].name;
    if (nm && strlen(nm) == (size_t)(c1 - text) && strncmp(nm, text, (size_t)(c1 - text)) == 0) break;
  }
  if (i == s->n_chromosomes) return -2;
  if (!(alpha > 0.0) || alpha > 1.7976931348623157e308) return -3;
  out->chr = i; out->pos = (int)pos; out->alpha = alpha;
  return 0;
}

int fscl_amd_nearest_sweep(const fscl_amd_sweep_t *sw, int n, int chr, int pos) {
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

void fscl_amd_sample_tables_build(const sm_ptable_t *sm, int n_depths, double **coef_t, double **neutral,
                                  int32_t *depth_n, int *n_iv_out) {
  const int n_iv = sm[0].spline_func[0]->n;
  size_t n_coef = 0, n_neut = 0, co = 0, no = 0;
  double *coef, *neut;
  int d, f, iv;
  for (d = 0; d < n_depths; d++) {
    const int m = sm[d].sample_size - 1;
    n_coef += (size_t)n_iv * (size_t)(m > 0 ? m : 0) * 4;
    n_neut += (size_t)(m > 0 ? m : 0);
  }
  coef = fh_malloc(sizeof(double) * (n_coef ? n_coef : 1), "sampler tables");
  neut = fh_malloc(sizeof(double) * (n_neut ? n_neut : 1), "sampler tables");
  for (d = 0; d < n_depths; d++) {
    const int n = sm[d].sample_size, m = n - 1;
    depth_n[d] = n;
    for (f = 1; f < n; f++) {
      const spline_t *sp = sm[d].spline_func[f];
      if (sp->n != n_iv) logmsg(MSG_FATAL, "fscl_amd: splines with different knot counts");
      for (iv = 0; iv < n_iv; iv++)
        memcpy(coef + co + ((size_t)iv * (size_t)m + (size_t)(f - 1)) * 4, sp->coef[iv], sizeof(double) * 4);
      neut[no + (size_t)(f - 1)] = sm[d].fsp[f];
    }
    if (m > 0) { co += (size_t)n_iv * (size_t)m * 4; no += (size_t)m; }
  }
  *coef_t = coef; *neutral = neut; *n_iv_out = n_iv;
}

scan_t *fscl_amd_simulate_scan(const scan_t *s, const int *freq) {
  scan_t *r;
  int i;
  if (!s || !freq) return NULL;
  r = fh_calloc(1, sizeof *r, "scan_t");
  r->n_snps = s->n_snps;
  r->snps = fh_malloc(sizeof(snp_t) * (size_t)(s->n_snps ? s->n_snps : 1), "snps");
  r->n_depths = s->n_depths;
  r->sample_depths = fh_malloc(sizeof(int) * (size_t)(s->n_depths ? s->n_depths : 1), "sample depths");
  memcpy(r->sample_depths, s->sample_depths, sizeof(int) * (size_t)s->n_depths);
  r->n_chromosomes = s->n_chromosomes;
  r->chr_limits = fh_calloc((size_t)(s->n_chromosomes ? s->n_chromosomes : 1), sizeof(chr_limits_t), "chr_limits");
  for (i = 0; i < s->n_chromosomes; i++) {
    r->chr_limits[i] = s->chr_limits[i];
    r->chr_limits[i].name = s->chr_limits[i].name ? strdup(s->chr_limits[i].name) : NULL;
  }
  for (i = 0; i < s->n_snps; i++) {
    const int n = s->sample_depths[s->snps[i].depth_p];
    snp_t *p = r->snps + i;
    *p = s->snps[i];
    p->null_logl = 0.0;
    p->obs_freq = p->folded && freq[i] > n - freq[i] ? n - freq[i] : freq[i];
  }
  return r;
}

void fscl_amd_scan_free(scan_t *s) {
  int i;
  if (!s) return;
  for (i = 0; s->scan_pts && i < s->n_scan_pts; i++) free(s->scan_pts[i].permute_clr);
  free(s->scan_pts);
  for (i = 0; s->chr_limits && i < s->n_chromosomes; i++) free(s->chr_limits[i].name);
  free(s->chr_limits);
  free(s->sample_depths);
  free(s->snps);
  free(s);
}

int fscl_amd_simulate_output(const char *fname, const scan_t *s) {
  FILE *f = stdout;
  int c, i;
  if (!s) return -1;
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open simulation file \"%s\" (%s)\n", fname, strerror(errno)); return -1; }
  }
  for (c = 0; c < s->n_chromosomes; c++) { /* snp-input.c:55: chr pos derived_count sample_size folded */
    const chr_limits_t *l = s->chr_limits + c;
    for (i = l->start_index; i < l->start_index + l->n_snps; i++) {
      const snp_t *p = s->snps + i;
      fprintf(f, "%s %d %d %d %d\n", l->name, p->pos, p->obs_freq, s->sample_depths[p->depth_p], p->folded);
    }
  }
  if (fname && fclose(f) != 0) return -1;
  return 0;
}

static int dbl_cmp(const void *va, const void *vb) {
  const double a = *(const double *)va, b = *(const double *)vb;
  return (a > b) - (a < b);
}

/* sorted[floor(q * (n - 1))] of n > 0 values (v is sorted in place) */
static double quantile(double *v, int n, double q) { return v[(int)floor(q * (double)(n - 1))]; }

void fscl_amd_bootstrap_output(const char *fname, const scan_t *s, const fscl_amd_sweep_t *sw, int n_sweeps, int reps,
                               const fscl_amd_boot_t *out, const char *label) {
  static const double Q[3] = {0.025, 0.5, 0.975};
  FILE *f = stdout;
  double *pos, *alpha, *clr;
  int k, r, q;
  if (!s || n_sweeps < 0 || reps < 0 || (n_sweeps && (!sw || (reps && !out)))) return;
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open bootstrap file \"%s\" (%s)\n", fname, strerror(errno)); return; }
  }
  pos = fh_malloc(sizeof(double) * 3 * (size_t)(reps ? reps : 1), "bootstrap summary");
  alpha = pos + (reps ? reps : 1);
  clr = alpha + (reps ? reps : 1);
  for (k = 0; k < n_sweeps; k++) {
    const char *name = s->chr_limits[sw[k].chr].name;
    int nf = 0;
    for (r = 0; r < reps; r++) {
      const fscl_amd_boot_t *b = out + (size_t)k * (size_t)reps + r;
      if (label) fprintf(f, "%s\t", label);
      fprintf(f, "%s\t%d\t%1.3e\t%d\t", name, sw[k].pos, sw[k].alpha, r);
      if (b->est_pos < 0) { fprintf(f, "NA\tNA\tNA\n"); continue; }
      fprintf(f, "%d\t%1.3e\t%1.2f\n", b->est_pos, exp(b->est_lalpha), b->clr);
      pos[nf] = b->est_pos; alpha[nf] = exp(b->est_lalpha); clr[nf] = b->clr;
      nf++;
    }
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\tsummary\t%d\t%d", name, sw[k].pos, reps, nf);
    if (nf == 0) { fprintf(f, "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"); continue; }
    qsort(pos, (size_t)nf, sizeof(double), dbl_cmp);
    qsort(alpha, (size_t)nf, sizeof(double), dbl_cmp);
    qsort(clr, (size_t)nf, sizeof(double), dbl_cmp);
    for (q = 0; q < 3; q++) fprintf(f, "\t%d", (int)quantile(pos, nf, Q[q]));
    for (q = 0; q < 3; q++) fprintf(f, "\t%1.3e", quantile(alpha, nf, Q[q]));
    fprintf(f, "\t%1.2f\n", quantile(clr, nf, 0.5));
  }
  free(pos);
  if (fname) fclose(f);
}
