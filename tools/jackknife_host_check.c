/* jackknife_host_check.c -- a stand-alone exercise of the host-only side of the delete-one-block
 * jackknife (fscl_amd/csrc/host/jackknife.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/jackknife_host_check.c fscl_amd/csrc/host/jackknife.c fscl_amd/csrc/host/util.c -lm \
 *       -o /tmp/jackknife_host_check && /tmp/jackknife_host_check /tmp
 *
 * It needs no GPU and no device library: the block bound of a run, the combination of hand-made
 * block sums into delete-one estimates and the --jackknife-file writer.  Exit status 0 and "ok"
 * when every check holds. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fscl_amd/csrc/host/fscl_host.h"

char *prepend_label, *output_fname;
int spline_pts, n_permute;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

int main(int argc, char **argv) {
  char name0[] = "chrA";
  chr_limits_t lim[1];
  snp_t *snps;
  scan_t s;
  fsclg_run_t run;
  fscl_amd_jack_block_t *blk;
  fscl_amd_jack_summary_t g;
  fscl_amd_blocks_t r;
  char path[4096], line[512];
  const char *dir = argc > 1 ? argv[1] : ".";
  int i, n, b0, nb;
  FILE *fp;

  configure_logmsg(1);
  memset(&s, 0, sizeof s);
  memset(lim, 0, sizeof lim);
  snps = calloc(100, sizeof *snps); /* sites at 1000, 1100, ..., 10900 */
  for (i = 0; i < 100; i++) snps[i].pos = 1000 + 100 * i;
  lim[0].name = name0; lim[0].start_pos = 1000; lim[0].bp_length = 10900; lim[0].start_index = 0; lim[0].n_snps = 100;
  s.chr_limits = lim; s.n_chromosomes = 1; s.snps = snps; s.n_snps = 100;

  /* the block bound: positions 5000 .. 5200, windows of +-10 sites: sites 29 .. 52 at the widest */
  run.chr = 0; run.start_pos = 5000; run.step = 100; run.count = 3;
  CHECK(fscl_amd_blocks_bound(&s, &run, 10, 1000, &b0, &nb) == 0 && b0 == 3 && nb == 4);  /* 3900 .. 6200 */
  CHECK(fscl_amd_blocks_bound(&s, &run, 1000, 1000, &b0, &nb) == 0 && b0 == 1 && nb == 10); /* the whole chromosome */
  CHECK(fscl_amd_blocks_bound(&s, &run, 10, 1, &b0, &nb) == 0 && nb == 2301);
  run.start_pos = 0; run.count = 1; /* left of every site: the window is pushed right */
  CHECK(fscl_amd_blocks_bound(&s, &run, 10, 1000, &b0, &nb) == 0 && b0 == 1 && nb == 3);   /* sites 0 .. 20 */
  run.start_pos = 50000;
  CHECK(fscl_amd_blocks_bound(&s, &run, 10, 1000, &b0, &nb) == 0 && b0 == 8 && nb == 3);   /* sites 79 .. 99 */
  run.count = 0;
  CHECK(fscl_amd_blocks_bound(&s, &run, 10, 1000, &b0, &nb) == 0 && b0 == 0 && nb == 1);
  CHECK(fscl_amd_blocks_bound(&s, &run, 10, 0, &b0, &nb) == -1);
  run.chr = 1; CHECK(fscl_amd_blocks_bound(&s, &run, 10, 1000, &b0, &nb) == -1);
  CHECK(fscl_amd_blocks_cap() >= 1);

  /* the combination: 3 positions x 4 blocks x 2 alphas on the heap at their exact sizes.  Block 1 carries the
     peak at position 1; without it position 2 wins; block 3 holds no term */
  {
    const int32_t pos[3] = {2000, 3000, 4000};
    const double la[2] = {-3., -1.};
    double *bs = calloc(24, sizeof *bs);
    uint32_t *cnt = calloc(24, sizeof *cnt);
#define CELL(p, j, k) (((p) * 4 + (j)) * 2 + (k))
    for (i = 0; i < 3; i++) { bs[CELL(i, 0, 0)] = 1.; cnt[CELL(i, 0, 0)] = 2; bs[CELL(i, 2, 0)] = 1.; cnt[CELL(i, 2, 0)] = 1; }
    bs[CELL(1, 1, 0)] = 10.; cnt[CELL(1, 1, 0)] = 5;
    bs[CELL(2, 2, 0)] = 1.5;
    blk = malloc(sizeof *blk * 4);
    CHECK(fscl_amd_jackknife_combine(bs, cnt, 3, 4, 2, pos, la, blk, &g) == 1);
    CHECK(g.ipos == 1 && g.ila == 0 && g.v == 12. && g.g == 3 && g.nb == 4);
    CHECK(blk[0].has_terms && blk[0].ipos == 1 && blk[0].v == 11. && blk[0].n_terms == 2);
    CHECK(blk[1].has_terms && blk[1].ipos == 2 && blk[1].ila == 0 && blk[1].v == 2.5 && blk[1].n_terms == 5);
    CHECK(blk[2].has_terms && blk[2].ipos == 1 && blk[2].v == 11. && blk[2].n_terms == 1);
    CHECK(!blk[3].has_terms && blk[3].ipos == -1 && blk[3].n_terms == 0);
    CHECK(g.top_shift == 1 && g.top_loss == 1 && g.n_edge_pos == 1 && g.n_edge_la == 3);
    /* theta_b = 3000, 4000, 3000: mean 10000/3, se^2 = 2/3 * (2 (1000/3)^2 + (2000/3)^2) */
    CHECK(fabs(g.se_pos - sqrt(2. / 3. * (2. * (1000. / 3.) * (1000. / 3.) + (2000. / 3.) * (2000. / 3.)))) < 1e-9);
    CHECK(fabs(g.bias_pos - 2. * (10000. / 3. - 3000.)) < 1e-9 && g.se_la == 0. && g.bias_la == 0.);
    /* a NaN cell never wins; a surface of NaN alone has no estimate */
    bs[CELL(1, 1, 0)] = NAN;
    CHECK(fscl_amd_jackknife_combine(bs, cnt, 3, 4, 2, pos, la, blk, &g) == 1 && g.ipos == 2 && g.v == 2.5);
    for (i = 0; i < 24; i++) bs[i] = NAN;
    CHECK(fscl_amd_jackknife_combine(bs, cnt, 3, 4, 2, pos, la, blk, &g) == 0 && g.ipos == -1 && isnan(g.se_pos) && g.g == 3);
    /* one block with terms: no spread */
    memset(bs, 0, sizeof *bs * 24); memset(cnt, 0, sizeof *cnt * 24);
    bs[CELL(0, 2, 1)] = 3.; cnt[CELL(0, 2, 1)] = 1;
    CHECK(fscl_amd_jackknife_combine(bs, cnt, 3, 4, 2, pos, la, blk, &g) == 1 && g.g == 1 && isnan(g.se_pos) && isnan(g.bias_la));
    CHECK(g.ipos == 0 && g.ila == 1 && blk[2].ipos == 0 && blk[2].ila == 0 && blk[2].v == 0.); /* all ties: the first cell */
    CHECK(fscl_amd_jackknife_combine(NULL, cnt, 3, 4, 2, pos, la, blk, &g) == -1);
    CHECK(fscl_amd_jackknife_combine(bs, cnt, 0, 4, 2, pos, la, blk, &g) == -1);
    free(blk);

    /* the writer: the first peak above, a second one of NaN alone */
    memset(&r, 0, sizeof r);
    r.n = 2; r.n_pos = 4; r.n_cells = 24 + 2;
    r.hdr = calloc(2, sizeof *r.hdr); r.pts = calloc(4, sizeof *r.pts);
    r.bs = calloc(26, sizeof *r.bs); r.cnt = calloc(26, sizeof *r.cnt);
    for (i = 0; i < 3; i++) { r.bs[CELL(i, 0, 0)] = 1.; r.cnt[CELL(i, 0, 0)] = 2; r.bs[CELL(i, 2, 0)] = 1.; r.cnt[CELL(i, 2, 0)] = 1; }
    r.bs[CELL(1, 1, 0)] = 10.; r.cnt[CELL(1, 1, 0)] = 5; r.bs[CELL(2, 2, 0)] = 1.5;
    r.bs[24] = NAN; r.bs[25] = NAN; r.cnt[24] = 1;
    for (i = 0; i < 4; i++) r.pts[i].sweep_pos = 2000 + 1000 * i;
    r.hdr[0].centre_pos = 3000; r.hdr[0].n_pos = 3; r.hdr[0].n_la = 2; r.hdr[0].nb = 4; r.hdr[0].b0 = 1; r.hdr[0].block_bp = 1000;
    r.hdr[0].la[0] = log(1e-4); r.hdr[0].la[1] = log(1e-3);
    r.hdr[1].centre_pos = 5000; r.hdr[1].n_pos = 1; r.hdr[1].n_la = 1; r.hdr[1].nb = 2; r.hdr[1].block_bp = 500;
    r.hdr[1].pos_off = 3; r.hdr[1].cell_off = 24;
    free(bs); free(cnt);
  }
  snprintf(path, sizeof path, "%s/jackknife_host_check.txt", dir);
  CHECK(fscl_amd_jackknife_output(path, &s, &r, "lab") == 0);
  CHECK(fscl_amd_jackknife_output("/nonexistent-directory/x.txt", &s, &r, NULL) == -1);
  fp = fopen(path, "r");
  CHECK(fp != NULL);
  for (n = 0; fgets(line, sizeof line, fp);) {
    n++;
    if (n == 1) CHECK(!strcmp(line, "lab\tchrA\t3000\t1000\t1999\t2\t3000\t1.000e-04\t22.00\t0\t0.0000\t-2.00\n"));
    if (n == 2) CHECK(!strcmp(line, "lab\tchrA\t3000\t2000\t2999\t5\t4000\t1.000e-04\t5.00\t1000\t0.0000\t-19.00\n"));
    if (n == 4) CHECK(!strcmp(line, "lab\tchrA\t3000\tsummary\t3\t2\t3\t3000\t1.000e-04\t24.00\t666.7\t0.0000\t11.33\t666.7\t0.0000\t2000\t2000\t1\t3\n"));
    if (n == 5) CHECK(!strcmp(line, "lab\tchrA\t5000\tsummary\t1\t1\t1\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\t0\t0\n"));
  }
  CHECK(n == 5);
  fclose(fp);
  remove(path);
  r.hdr[1].cell_off = 25; /* a header past the arrays */
  CHECK(fscl_amd_jackknife_output(path, &s, &r, NULL) == -1);
  fscl_amd_blocks_free(&r);
  CHECK(r.hdr == NULL && r.n == 0);
  fscl_amd_blocks_free(&r);
  free(snps);
  printf("ok\n");
  return 0;
}
