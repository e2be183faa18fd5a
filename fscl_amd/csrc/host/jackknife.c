/* jackknife.c -- the host-only side of the delete-one-block jackknife of sweep peaks
   (--jackknife-file): the blocks a request needs, the size limits, the combination of the block
   sums into delete-one estimates and the writer.  No device call is made here
   (fscl_amd_scan_blocks, analyses.c, evaluates); tools/jackknife_host_check.c builds this file alone
   under the sanitizers. */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fscl_host.h"

void fscl_amd_blocks_free(fscl_amd_blocks_t *r) {
  if (!r) return;
  free(r->hdr); free(r->pts); free(r->bs); free(r->cnt);
  memset(r, 0, sizeof *r);
}

size_t fscl_amd_blocks_cap(void) {
  const char *e = getenv("FSCL_AMD_BLOCKS_CAP");
  char *end = NULL;
  unsigned long long v;
  if (!e || !*e) return (size_t)1 << 30;
  v = strtoull(e, &end, 10);
  if (end == e || *end || v < 1) return (size_t)1 << 30;
  return (size_t)v;
}

/* the first index in [0, n) of a site at or past pos (n: none) */
static int lower_site(const snp_t *a, int n, long long pos) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = lo + (hi - lo) / 2;
    if ((long long)a[m].pos < pos) lo = m + 1; else hi = m;
  }
  return lo;
}

int fscl_amd_blocks_bound(const scan_t *s, const fsclg_run_t *run, int eval_range, int block_bp, int *b0, int *nb) {
  const chr_limits_t *c;
  const snp_t *a;
  long long first, last, lo, hi, ws, we, er = eval_range;
  int n;
  if (!s || !run || !b0 || !nb || block_bp < 1 || eval_range < 0 || run->chr < 0 || run->chr >= s->n_chromosomes || run->step < 1)
    return -1;
  c = s->chr_limits + run->chr;
  a = s->snps + c->start_index; n = c->n_snps;
  *b0 = 0; *nb = 1;
  if (run->count <= 0 || n <= 0) return 0;
  first = run->start_pos; last = first + (long long)(run->count - 1) * run->step;
  /* init_scan_result's nearest SNP of a position is the first site at or past it or the one before
     (the de-collision moves the position, by 64 at most as the device's run check allows, never the
     SNP); its window is nearest -/+ eval_range, shifted to stay inside the chromosome */
  lo = (long long)lower_site(a, n, first) - 1; if (lo < 0) lo = 0;
  hi = lower_site(a, n, last); if (hi > n - 1) hi = n - 1;
  ws = lo - er; if (ws > (long long)n - 1 - 2 * er) ws = (long long)n - 1 - 2 * er; if (ws < 0) ws = 0;
  we = hi + er; if (we < 2 * er) we = 2 * er; if (we > n - 1) we = n - 1;
  lo = a[ws].pos / block_bp; hi = a[we].pos / block_bp;
  if (lo < 0) lo = 0;
  if (hi < lo) hi = lo;
  *b0 = (int)lo;
  if (hi - lo + 1 > 0x7FFFFFFFll) return -1;
  *nb = (int)(hi - lo + 1);
  return 0;
}

/* the first strict maximum of v[n_pos][n_la] in position order, then alpha order; a NaN never wins */
static void first_max(const double *v, int n_pos, int n_la, int *ip, int *ik, double *m) {
  int p, k;
  *ip = -1; *ik = -1; *m = NAN;
  for (p = 0; p < n_pos; p++)
    for (k = 0; k < n_la; k++) {
      const double x = v[(size_t)p * n_la + k];
      if (x == x && (*ip < 0 || x > *m)) { *m = x; *ip = p; *ik = k; }
    }
}

int fscl_amd_jackknife_combine(const double *bs, const uint32_t *cnt, int n_pos, int nb, int n_la, const int32_t *pos,
                               const double *la, fscl_amd_jack_block_t *blocks, fscl_amd_jack_summary_t *out) {
  const size_t nc = (size_t)(n_pos > 0 ? n_pos : 0) * (size_t)(n_la > 0 ? n_la : 0);
  double *pre, *v, sum[3] = {0., 0., 0.}, ss[3] = {0., 0., 0.}, full[3], dmax = -1., lmax = 0.;
  int b, j, p, k, g = 0, na = 0, have_loss = 0;
  if (!out) return -1;
  memset(out, 0, sizeof *out);
  out->ipos = out->ila = out->top_shift = out->top_loss = -1;
  out->v = out->se_pos = out->se_la = out->se_clr = out->bias_pos = out->bias_la = out->bias_clr = NAN;
  if (!bs || !cnt || !pos || !la || !blocks || n_pos < 1 || nb < 1 || n_la < 1) return -1;
  out->n_pos = n_pos; out->n_la = n_la; out->nb = nb;
  pre = fh_calloc(nc, sizeof *pre, "jackknife"); /* the fold of the blocks before b, from +0.0 */
  v = fh_malloc(sizeof *v * nc, "jackknife");
  for (b = 0; b < nb; b++) {
    fscl_amd_jack_block_t *o = blocks + b;
    memset(o, 0, sizeof *o);
    o->block = b; o->ipos = o->ila = -1; o->v = NAN;
    for (p = 0; p < n_pos && !o->has_terms; p++)
      for (k = 0; k < n_la; k++)
        if (cnt[((size_t)p * nb + b) * n_la + k]) { o->has_terms = 1; break; }
    if (o->has_terms) { /* V_b: the blocks j != b in ascending j */
      memcpy(v, pre, sizeof *v * nc);
      for (p = 0; p < n_pos; p++)
        for (j = b + 1; j < nb; j++)
          for (k = 0; k < n_la; k++) v[(size_t)p * n_la + k] = v[(size_t)p * n_la + k] + bs[((size_t)p * nb + j) * n_la + k];
      first_max(v, n_pos, n_la, &o->ipos, &o->ila, &o->v);
      g++;
    }
    for (p = 0; p < n_pos; p++)
      for (k = 0; k < n_la; k++) pre[(size_t)p * n_la + k] = pre[(size_t)p * n_la + k] + bs[((size_t)p * nb + b) * n_la + k];
  }
  first_max(pre, n_pos, n_la, &out->ipos, &out->ila, &out->v); /* the full estimate: every block */
  free(v); free(pre);
  out->g = g;
  if (out->ipos < 0) return 0; /* every cell NaN */
  full[0] = (double)pos[out->ipos]; full[1] = la[out->ila]; full[2] = 2.0 * out->v;
  for (b = 0; b < nb; b++) {
    fscl_amd_jack_block_t *o = blocks + b;
    double d, l;
    o->n_terms = cnt[((size_t)out->ipos * nb + b) * n_la + out->ila];
    if (!o->has_terms) continue;
    if (o->ipos < 0) { na++; continue; }
    sum[0] += (double)pos[o->ipos]; sum[1] += la[o->ila]; sum[2] += 2.0 * o->v;
    d = fabs((double)pos[o->ipos] - full[0]);
    l = full[2] - 2.0 * o->v;
    if (d > dmax) { dmax = d; out->top_shift = b; }
    if (!have_loss || l > lmax) { lmax = l; out->top_loss = b; have_loss = 1; }
    if (o->ipos == 0 || o->ipos == n_pos - 1) out->n_edge_pos++;
    if (o->ila == 0 || o->ila == n_la - 1) out->n_edge_la++;
  }
  if (g >= 2 && na == 0) { /* (a delete-one surface of NaN alone has no estimate: no spread is reported) */
    double mean[3], *se[3] = {&out->se_pos, &out->se_la, &out->se_clr}, *bias[3] = {&out->bias_pos, &out->bias_la, &out->bias_clr};
    for (k = 0; k < 3; k++) mean[k] = sum[k] / (double)g;
    for (b = 0; b < nb; b++) {
      const fscl_amd_jack_block_t *o = blocks + b;
      double th[3];
      if (!o->has_terms) continue;
      th[0] = (double)pos[o->ipos]; th[1] = la[o->ila]; th[2] = 2.0 * o->v;
      for (k = 0; k < 3; k++) ss[k] += (th[k] - mean[k]) * (th[k] - mean[k]);
    }
    for (k = 0; k < 3; k++) {
      *se[k] = sqrt(((double)(g - 1) / (double)g) * ss[k]);
      *bias[k] = (double)(g - 1) * (mean[k] - full[k]);
    }
  }
  return 1;
}

static void put_num(FILE *f, const char *fmt, double x) {
  if (x == x) fprintf(f, fmt, x); else fprintf(f, "\tNA");
}

int fscl_amd_jackknife_output(const char *fname, const scan_t *s, const fscl_amd_blocks_t *r, const char *label) {
  FILE *f = stdout;
  int i, b, p;
  if (!r || !s) return -1;
  for (i = 0; i < r->n; i++) { /* before anything is written */
    const fscl_amd_blocks_hdr_t *h = r->hdr + i;
    if (h->chr < 0 || h->chr >= s->n_chromosomes || h->n_pos < 0 || h->n_la < 1 || h->n_la > FSCL_AMD_SURFACE_MAX_LA ||
        h->nb < 1 || h->nb > FSCL_AMD_BLOCKS_MAX_NB || h->block_bp < 1 || h->b0 < 0 || h->pos_off + (uint64_t)h->n_pos > r->n_pos ||
        h->cell_off + (uint64_t)h->n_pos * (uint64_t)h->nb * (uint64_t)h->n_la > r->n_cells)
      return -1;
  }
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open jackknife file \"%s\" (%s)", fname, strerror(errno)); return -1; }
  }
  for (i = 0; i < r->n; i++) {
    const fscl_amd_blocks_hdr_t *h = r->hdr + i;
    const char *name = s->chr_limits[h->chr].name;
    fscl_amd_jack_block_t *blk = fh_calloc((size_t)h->nb, sizeof *blk, "jackknife output");
    int32_t *pos = fh_malloc(sizeof *pos * (h->n_pos ? h->n_pos : 1), "jackknife output");
    fscl_amd_jack_summary_t g;
    int have = 0;
    for (p = 0; p < h->n_pos; p++) pos[p] = r->pts[h->pos_off + p].sweep_pos;
    if (h->n_pos > 0)
      have = fscl_amd_jackknife_combine(r->bs + h->cell_off, r->cnt + h->cell_off, h->n_pos, h->nb, h->n_la, pos, h->la, blk, &g);
    else { memset(&g, 0, sizeof g); g.n_la = h->n_la; g.nb = h->nb; }
    for (b = 0; have == 1 && b < h->nb; b++) {
      const fscl_amd_jack_block_t *o = blk + b;
      const long long bstart = ((long long)h->b0 + b) * h->block_bp;
      if (!o->has_terms) continue;
      if (label) fprintf(f, "%s\t", label);
      fprintf(f, "%s\t%d\t%lld\t%lld\t%u", name, h->centre_pos, bstart, bstart + h->block_bp - 1, o->n_terms);
      if (o->ipos >= 0)
        fprintf(f, "\t%d\t%1.3e\t%1.2f\t%d\t%1.4f\t%1.2f\n", pos[o->ipos], exp(h->la[o->ila]), 2.0 * o->v, pos[o->ipos] - pos[g.ipos],
                h->la[o->ila] - h->la[g.ila], 2.0 * o->v - 2.0 * g.v);
      else
        fprintf(f, "\tNA\tNA\tNA\tNA\tNA\tNA\n");
    }
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\tsummary\t%d\t%d\t%d", name, h->centre_pos, h->n_pos, h->n_la, g.g);
    if (have == 1) {
      fprintf(f, "\t%d\t%1.3e\t%1.2f", pos[g.ipos], exp(h->la[g.ila]), 2.0 * g.v);
      put_num(f, "\t%1.1f", g.se_pos); put_num(f, "\t%1.4f", g.se_la); put_num(f, "\t%1.2f", g.se_clr);
      put_num(f, "\t%1.1f", g.bias_pos); put_num(f, "\t%1.4f", g.bias_la);
      if (g.top_shift >= 0) fprintf(f, "\t%lld", ((long long)h->b0 + g.top_shift) * h->block_bp); else fprintf(f, "\tNA");
      if (g.top_loss >= 0) fprintf(f, "\t%lld", ((long long)h->b0 + g.top_loss) * h->block_bp); else fprintf(f, "\tNA");
      fprintf(f, "\t%d\t%d\n", g.n_edge_pos, g.n_edge_la);
    } else {
      fprintf(f, "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\t0\t0\n");
    }
    free(blk); free(pos);
  }
  if (fname) fclose(f);
  return 0;
}
