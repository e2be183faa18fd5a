/* conditional_host_check.c -- a stand-alone exercise of the host-only side of the conditional sweep scan
 * (fscl_amd/csrc/host/conditional.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/conditional_host_check.c fscl_amd/csrc/host/conditional.c fscl_amd/csrc/host/util.c -lm \
 *       -o /tmp/conditional_host_check && /tmp/conditional_host_check /tmp
 *
 * It needs no GPU and no device library: the sites a candidate owns (the tie rule, the de-collision and its
 * comparison of a global index with the chromosome's count), the given sweeps' terms per site, the base
 * fold with NaN and zero entries, and the --conditional-file writer, all on exact-size heap arrays.  Exit
 * status 0 and "ok" when every check holds. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fscl_amd/csrc/host/fscl_host.h"

char *prepend_label, *output_fname;
int spline_pts, n_permute;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

int main(int argc, char **argv) {
  /* chromosome A: sites 0 .. 5 at 100, 200, 300, 400, 500, 600; chromosome B: sites 6 .. 9 at 100, 101, 102, 900 */
  static const int posv[10] = {100, 200, 300, 400, 500, 600, 100, 101, 102, 900};
  char nameA[] = "chrA", nameB[] = "chrB";
  chr_limits_t *lim = calloc(2, sizeof *lim);
  snp_t *snps = calloc(10, sizeof *snps);
  fscl_amd_sweep_t *gv = calloc(3, sizeof *gv);
  fscl_amd_site_hdr_t *hdr = calloc(3, sizeof *hdr);
  fscl_amd_conditional_t r;
  scan_t s;
  double *terms, *g;
  char path[4096], line[512];
  const char *dir = argc > 1 ? argv[1] : ".";
  int i, n, sp, lo, hi, nt;
  FILE *fp;

  configure_logmsg(1);
  CHECK(lim && snps && gv && hdr);
  memset(&s, 0, sizeof s);
  for (i = 0; i < 10; i++) { snps[i].pos = posv[i]; snps[i].chr = i >= 6; }
  lim[0].name = nameA; lim[0].start_index = 0; lim[0].n_snps = 6; lim[0].start_pos = 100; lim[0].bp_length = 600;
  lim[1].chr = 1; lim[1].name = nameB; lim[1].start_index = 6; lim[1].n_snps = 4; lim[1].start_pos = 100; lim[1].bp_length = 900;
  s.snps = snps; s.n_snps = 10; s.chr_limits = lim; s.n_chromosomes = 2;

  /* no given sweep: the whole chromosome; a candidate on a site is de-collided on the first chromosome */
  CHECK(fscl_amd_cond_clip(&s, NULL, 0, 0, 250, &sp, &lo, &hi) == 0 && sp == 250 && lo == 0 && hi == 5);
  CHECK(fscl_amd_cond_clip(&s, NULL, 0, 0, 300, &sp, &lo, &hi) == 0 && sp == 301 && lo == 0 && hi == 5);
  /* Q3: on a later chromosome the global index is never below the count: no de-collision (100 stays 100) */
  CHECK(fscl_amd_cond_clip(&s, NULL, 0, 1, 100, &sp, &lo, &hi) == 0 && sp == 100 && lo == 6 && hi == 9);
  /* the tie rule: s + q even (s 250, q 350: the site at 300 ties and goes to the lower position, the candidate) */
  gv[0].chr = 0; gv[0].pos = 350; gv[0].alpha = 1e-3;
  CHECK(fscl_amd_cond_clip(&s, gv, 1, 0, 250, &sp, &lo, &hi) == 0 && lo == 0 && hi == 2);
  /* q below s (q 350, s 450: the site at 400 ties and stays with the given sweep) */
  CHECK(fscl_amd_cond_clip(&s, gv, 1, 0, 450, &sp, &lo, &hi) == 0 && lo == 4 && hi == 5);
  /* s + q odd (s 251: 2x <= 601 keeps 300) */
  CHECK(fscl_amd_cond_clip(&s, gv, 1, 0, 251, &sp, &lo, &hi) == 0 && lo == 0 && hi == 2);
  CHECK(fscl_amd_cond_clip(&s, gv, 1, 0, 249, &sp, &lo, &hi) == 0 && lo == 0 && hi == 1);
  /* q = s: nothing */
  CHECK(fscl_amd_cond_clip(&s, gv, 1, 0, 350, &sp, &lo, &hi) == 0 && sp == 350 && lo > hi);
  /* a sweep on either side, and one of another chromosome that is skipped */
  gv[1].chr = 0; gv[1].pos = 150; gv[1].alpha = 1e-2;
  gv[2].chr = 1; gv[2].pos = 260; gv[2].alpha = 1e-2;
  CHECK(fscl_amd_cond_clip(&s, gv, 3, 0, 260, &sp, &lo, &hi) == 0 && lo == 2 && hi == 2);
  /* squeezed between two given sweeps with no site of its own */
  gv[1].pos = 310;
  CHECK(fscl_amd_cond_clip(&s, gv, 3, 0, 330, &sp, &lo, &hi) == 0 && lo > hi);
  /* a candidate whose nearest SNP lies beyond q (s 320, q 310 < s: nearest 300 belongs to q) */
  CHECK(fscl_amd_cond_clip(&s, gv, 2, 0, 320, &sp, &lo, &hi) == 0 && lo > hi);
  gv[1].pos = 150;
  CHECK(fscl_amd_cond_clip(&s, gv, 3, 2, 260, &sp, &lo, &hi) == -1 && fscl_amd_cond_clip(&s, gv, 3, -1, 260, &sp, &lo, &hi) == -1);
  CHECK(fscl_amd_cond_clip(&s, gv, 3, 0, 260, NULL, &lo, &hi) == -1);

  /* the given sweeps' terms: walks of gv[0] (nearest 3, one site left, two right) and gv[1] (nearest 0, one right) */
  terms = malloc(sizeof(double) * 6);
  g = malloc(sizeof(double) * 6);
  CHECK(terms && g);
  hdr[0].pt.nearest_snp = 3; hdr[0].nl = 1; hdr[0].nr = 2; hdr[0].len = 4; hdr[0].off = 0;
  terms[0] = 3.5; terms[1] = 2.5; terms[2] = 4.5; terms[3] = NAN;
  hdr[1].pt.nearest_snp = 0; hdr[1].nl = 0; hdr[1].nr = 1; hdr[1].len = 2; hdr[1].off = 4;
  terms[4] = -1.0; terms[5] = -2.0;
  CHECK(fscl_amd_cond_given_terms(&s, gv, 3, 0, hdr, terms, g) == 0);
  /* sites 0, 1 belong to gv[1] (150), sites 2 .. 5 to gv[0] (350; 250 would tie, there is no site there) */
  CHECK(g[0] == -1.0 && g[1] == -2.0 && g[2] == 2.5 && g[3] == 3.5 && g[4] == 4.5 && isnan(g[5]));
  hdr[0].len = 0; /* an empty walk: +0.0 everywhere it owns */
  CHECK(fscl_amd_cond_given_terms(&s, gv, 3, 0, hdr, terms, g) == 0 && g[2] == 0.0 && !signbit(g[2]) && g[5] == 0.0);
  hdr[0].len = 4;
  CHECK(fscl_amd_cond_given_terms(&s, gv, 3, 0, hdr, terms, g) == 0);
  CHECK(fscl_amd_cond_given_terms(&s, gv, 3, 5, hdr, terms, g) == -1 && fscl_amd_cond_given_terms(&s, gv, 3, 0, hdr, terms, NULL) == -1);

  /* the base fold: ascending from +0.0, cut to the window, zeros skipped, a NaN confined to the folds that reach it */
  CHECK(fscl_amd_cond_base(g, 0, 0, 4, 0, 5, &nt) == ((((-1.0 + -2.0) + 2.5) + 3.5) + 4.5) && nt == 5);
  CHECK(fscl_amd_cond_base(g, 0, 0, 5, 1, 3, &nt) == ((-2.0 + 2.5) + 3.5) && nt == 3);
  CHECK(isnan(fscl_amd_cond_base(g, 0, 2, 5, 0, 5, &nt)) && nt == 4);
  CHECK(fscl_amd_cond_base(g, 0, 3, 2, 0, 5, &nt) == 0.0 && nt == 0 && !signbit(fscl_amd_cond_base(g, 0, 3, 2, 0, 5, NULL)));
  g[0] = -0.0; g[1] = 0.0;
  CHECK(fscl_amd_cond_base(g, 0, 0, 1, 0, 5, &nt) == 0.0 && !signbit(fscl_amd_cond_base(g, 0, 0, 1, 0, 5, &nt)) && nt == 2);
  CHECK(fscl_amd_cond_base(g + 2, 2, -100, 100, 2, 4, &nt) == (2.5 + 3.5) + 4.5 && nt == 3);
  free(terms); free(g);

  /* the writer: two blocks, the second with an empty interval and no maximum */
  memset(&r, 0, sizeof r);
  r.n_blocks = 2; r.n_rows = 3; r.n_given = 3;
  r.blk = calloc(2, sizeof *r.blk); r.rows = calloc(3, sizeof *r.rows); r.given = calloc(3, sizeof *r.given);
  CHECK(r.blk && r.rows && r.given);
  r.given[0] = gv[0]; r.given[1] = gv[1]; r.given[2] = gv[2];
  r.blk[0].chr = 0; r.blk[0].round = 1; r.blk[0].n_pos = 2; r.blk[0].n_given = 2; r.blk[0].max_row = 1; r.blk[0].added = 1;
  r.blk[1].chr = 1; r.blk[1].round = 2; r.blk[1].n_pos = 1; r.blk[1].n_given = 1; r.blk[1].row_off = 2; r.blk[1].given_off = 2;
  r.blk[1].max_row = -1;
  r.rows[0].pos = 250; r.rows[0].lo = 2; r.rows[0].hi = 2; r.rows[0].n_terms = 1; r.rows[0].lalpha = log(1e-4); r.rows[0].cond_clr = -1.25;
  r.rows[0].base = 2.5;
  r.rows[1].pos = 450; r.rows[1].lo = 4; r.rows[1].hi = 5; r.rows[1].n_terms = 2; r.rows[1].lalpha = log(1e-2); r.rows[1].cond_clr = 12.5;
  r.rows[1].base = -0.75;
  r.rows[2].pos = 260; r.rows[2].lo = 8; r.rows[2].hi = 7; r.rows[2].lalpha = 4.0; r.rows[2].cond_clr = NAN;
  snprintf(path, sizeof path, "%s/conditional_host_check.txt", dir);
  CHECK(fscl_amd_conditional_output(path, &s, &r, "lab") == 0);
  CHECK(fscl_amd_conditional_output("/nonexistent-directory/x.txt", &s, &r, NULL) == -1);
  CHECK(fscl_amd_conditional_output(path, NULL, &r, NULL) == -1);
  fp = fopen(path, "r");
  CHECK(fp != NULL);
  for (n = 0; fgets(line, sizeof line, fp);) {
    n++;
    if (n == 1) CHECK(!strcmp(line, "lab\tchrA\t1\t250\t1.000e-04\t-1.25\t300\t300\t1\t2.5000\n"));
    if (n == 2) CHECK(!strcmp(line, "lab\tchrA\t1\t450\t1.000e-02\t12.50\t500\t600\t2\t-0.7500\n"));
    if (n == 3) CHECK(!strcmp(line, "lab\tchrA\t1\tsummary\t2\t2\t350:1.000e-03,150:1.000e-02\t450\t1.000e-02\t12.50\t1\n"));
    if (n == 4) CHECK(!strcmp(line, "lab\tchrB\t2\t260\t5.460e+01\tnan\tNA\tNA\t0\t0.0000\n") ||
                      !strcmp(line, "lab\tchrB\t2\t260\t5.460e+01\t-nan\tNA\tNA\t0\t0.0000\n"));
    if (n == 5) CHECK(!strcmp(line, "lab\tchrB\t2\tsummary\t1\t1\t260:1.000e-02\tNA\tNA\tNA\t0\n"));
  }
  CHECK(n == 5);
  fclose(fp);
  remove(path);
  r.blk[1].row_off = 3; /* a block past the arrays */
  CHECK(fscl_amd_conditional_output(path, &s, &r, NULL) == -1);
  r.blk[1].row_off = 2; r.blk[1].max_row = 1; /* a maximum past the block */
  CHECK(fscl_amd_conditional_output(path, &s, &r, NULL) == -1);
  fscl_amd_conditional_free(&r);
  CHECK(r.blk == NULL && r.n_blocks == 0);
  fscl_amd_conditional_free(&r);
  CHECK(fscl_amd_conditional_cap() >= 1);
  free(lim); free(snps); free(gv); free(hdr);
  printf("ok\n");
  return 0;
}
