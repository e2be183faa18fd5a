/* tail_host_check.c -- a stand-alone exercise of the host-only side of the projected p-values
 * (fscl_amd/csrc/host/tail.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/tail_host_check.c fscl_amd/csrc/host/tail.c fscl_amd/csrc/host/util.c -lm \
 *       -o /tmp/tail_host_check && /tmp/tail_host_check /tmp
 *
 * It needs no GPU and no device library: the used prefix of a point's record, the chunks of a
 * launch under a cap, the packing of a chunk, the summary with its calibration figure and the
 * --tail-file writer.  Exit status 0 and "ok" when every check holds. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fscl_amd/csrc/host/fscl_host.h"

char *prepend_label, *output_fname;
int spline_pts, n_permute;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

enum { NP = 6 };

int main(int argc, char **argv) {
  static const int pn[NP] = {0, 3, 20, 10000, 25000, 7};
  static const int pp[NP] = {0, 1, 20, 6, 0, 5};
  char name0[] = "chrA", name1[] = "x:1";
  chr_limits_t lim[2] = {{0, name0, 0, 0, 0, 0}, {1, name1, 0, 0, 0, 0}};
  scan_pt_t pts[NP];
  scan_t s;
  const float *src[NP];
  int32_t counts[NP];
  unsigned long long off[NP];
  fscl_amd_tail_t t;
  float *buf;
  char path[4096];
  int i, k, first, n;
  size_t tot;
  const char *dir = argc > 1 ? argv[1] : ".";

  configure_logmsg(1);
  memset(pts, 0, sizeof pts);
  memset(&s, 0, sizeof s);
  for (i = 0; i < NP; i++) {
    pts[i].chr = i < 4 ? 0 : 1; pts[i].sweep_pos = 1000 * (i + 1); pts[i].clr = 2.5 * i;
    pts[i].permute_n = pn[i]; pts[i].permute_p = pp[i];
    pts[i].permute_clr = i == 0 ? NULL : malloc(sizeof(float) * FSCL_AMD_TAIL_SAVE); /* the record's full size, as scan_permute */
    for (k = 0; pts[i].permute_clr && k < FSCL_AMD_TAIL_SAVE; k++) pts[i].permute_clr[k] = (float)(i * 100000 + k);
  }
  s.n_scan_pts = NP; s.scan_pts = pts; s.chr_limits = lim; s.n_chromosomes = 2;

  /* the used prefix */
  CHECK(fscl_amd_tail_count(pts + 0) == 0 && fscl_amd_tail_count(pts + 1) == 3 && fscl_amd_tail_count(pts + 3) == 10000);
  CHECK(fscl_amd_tail_count(pts + 4) == 10000 && fscl_amd_tail_count(NULL) == 0);
  for (i = 0; i < NP; i++) { counts[i] = fscl_amd_tail_count(pts + i); src[i] = pts[i].permute_clr; }

  /* the chunks: whole points, at most cap floats, at least one point */
  CHECK(fscl_amd_tail_chunk(counts, NP, 0, 1u << 24) == NP);
  CHECK(fscl_amd_tail_chunk(counts, NP, 0, 23) == 3);       /* 0 + 3 + 20 */
  CHECK(fscl_amd_tail_chunk(counts, NP, 0, 22) == 2);
  CHECK(fscl_amd_tail_chunk(counts, NP, 3, 5) == 1);        /* a point above the cap goes alone */
  CHECK(fscl_amd_tail_chunk(counts, NP, 3, 20000) == 2 && fscl_amd_tail_chunk(counts, NP, 3, 19999) == 1);
  CHECK(fscl_amd_tail_chunk(counts, NP, 5, 0) == 1 && fscl_amd_tail_chunk(counts, NP, NP, 100) == 0);
  CHECK(fscl_amd_tail_chunk(counts, NP, -1, 100) == 0 && fscl_amd_tail_chunk(NULL, NP, 0, 100) == 0);
  for (first = 0, n = 0; first < NP; first += k, n++) { k = fscl_amd_tail_chunk(counts, NP, first, 10007); CHECK(k >= 1); }
  CHECK(n == 3);                                            /* {0,3,20}, {10000}, {10000,7} */

  /* the packing of every chunk, into a buffer of exactly the chunk's size */
  for (first = 0; first < NP; first += n) {
    size_t need = 0;
    n = fscl_amd_tail_chunk(counts, NP, first, 10007);
    for (k = 0; k < n; k++) need += (size_t)counts[first + k];
    buf = malloc(sizeof(float) * (need ? need : 1));
    tot = fscl_amd_tail_pack(src, counts, first, n, buf, off);
    CHECK(tot == need);
    for (k = 0; k < n; k++) {
      CHECK(off[k] + (size_t)counts[first + k] <= tot && (k == 0 || off[k] == off[k - 1] + (size_t)counts[first + k - 1]));
      for (i = 0; i < counts[first + k]; i++) CHECK(buf[off[k] + i] == (float)((first + k) * 100000 + i));
    }
    free(buf);
  }

  /* the summary and the writer */
  memset(&t, 0, sizeof t);
  t.n = NP; t.df = 2; t.min_n = 20;
  t.pt = calloc(NP, sizeof *t.pt);
  for (i = 0; i < NP; i++) {
    fsclg_tail_t *r = t.pt + i;
    r->m = counts[i]; r->m_pos = counts[i] - counts[i] / 4;
    r->flag = r->m_pos < 20 ? FSCLG_TAIL_NOFIT : i == 2 ? FSCLG_TAIL_CENTRAL : FSCLG_TAIL_FIT;
    r->mean = 3.0 + i; r->variance = i == 3 ? NAN : 20.0 + i;
    r->lambda = r->flag == FSCLG_TAIL_NOFIT ? NAN : r->flag == FSCLG_TAIL_CENTRAL ? 0.0 : 1.5 * i;
    r->logl = r->flag == FSCLG_TAIL_NOFIT ? NAN : -100.0 * i;
    r->log10_q = r->flag == FSCLG_TAIL_NOFIT ? NAN : -0.75 * i;
  }
  fscl_amd_tail_summary(&s, &t);
  CHECK(t.n_fit == 2 && t.n_central == 0 && t.n_nofit == 4);   /* point 2 has 15 positive samples */
  CHECK(t.n_calibration == 1);                                  /* point 3 alone: fitted, permute_p >= 5 */
  CHECK(fabs(t.calibration - (log10(7500. / 10000.) - 2.25 - log10(5. / 9999.))) < 1e-12);
  CHECK(isnan(fscl_amd_tail_log10p(t.pt + 0)) && isnan(fscl_amd_tail_log10p(NULL)));
  snprintf(path, sizeof path, "%s/tail_host_check.txt", dir);
  CHECK(fscl_amd_tail_output(path, &s, &t, "lab") == 0);
  CHECK(fscl_amd_tail_output("/nonexistent-directory/x.txt", &s, &t, NULL) == -1);
  {
    FILE *fp = fopen(path, "r");
    char line[512];
    n = 0;
    CHECK(fp != NULL);
    while (fgets(line, sizeof line, fp)) {
      n++;
      if (n == 1) CHECK(!strcmp(line, "lab\tchrA\t1000\t0.00\t0\t0\t0\tNA\tNA\tNA\tNA\tnofit\n"));
      if (n == 4) CHECK(!strcmp(line, "lab\tchrA\t4000\t7.50\t6\t10000\t7500\t4.5000\tNA\t3.301\t2.375\tfit\n"));
      if (n == 5) CHECK(!strcmp(line, "lab\tx:1\t5000\t10.00\t0\t25000\t7500\t6.0000\t0.857\t4.398\t3.125\tfit\n"));
    }
    CHECK(n == NP);
    fclose(fp);
  }
  remove(path);
  t.n = NP - 1;
  CHECK(fscl_amd_tail_output(path, &s, &t, NULL) == -1);   /* not one row per scan point */
  t.n = NP;
  fscl_amd_tail_free(&t);
  CHECK(t.pt == NULL && t.n == 0);
  fscl_amd_tail_free(&t);
  fscl_amd_tail_summary(&s, &t);                           /* nothing to summarise */
  CHECK(t.n_fit == 0 && isnan(t.calibration));
  for (i = 0; i < NP; i++) free(pts[i].permute_clr);
  printf("ok\n");
  return 0;
}
