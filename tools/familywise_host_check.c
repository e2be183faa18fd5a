/* familywise_host_check.c -- a stand-alone exercise of the host-only side of the family-wise
 * adjusted p-values (fscl_amd/csrc/host/familywise.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/familywise_host_check.c fscl_amd/csrc/host/familywise.c fscl_amd/csrc/host/util.c -lm \
 *       -o /tmp/familywise_host_check && /tmp/familywise_host_check /tmp
 *
 * It needs no GPU and no device library: the rank order, the chunk under a cap, the refusals before
 * any device work, the combine, the thresholds and both writers.  Exit status 0 and "ok" when every
 * check holds. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fscl_amd/csrc/host/fscl_host.h"

char *prepend_label, *output_fname;
int spline_pts, n_permute;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

enum { NP = 5, M = 19, NG = 2 };

static int line_is(const char *path, int want_line, const char *text) {
  FILE *fp = fopen(path, "r");
  char line[1024];
  int n = 0, ok = 0;
  if (!fp) return 0;
  while (fgets(line, sizeof line, fp))
    if (++n == want_line) ok = !strcmp(line, text);
  fclose(fp);
  return ok;
}

int main(int argc, char **argv) {
  static const double clr[NP] = {3.0, 12.5, 3.0, 0.0, 40.0};
  static const int chr[NP] = {0, 0, 0, 1, 1};
  char name0[] = "chrA", name1[] = "x:1";
  chr_limits_t lim[NG];
  scan_pt_t pts[NP];
  scan_t s;
  fscl_amd_familywise_t f;
  int32_t order[NP], rank[NP];
  double ps[NP], pc[NP], pt[NP], thr, obs_nan[4] = {1.0, NAN, 2.0, 2.0};
  int32_t o4[4];
  char path[4096];
  int i, t;
  const char *dir = argc > 1 ? argv[1] : ".";

  configure_logmsg(1);
  memset(pts, 0, sizeof pts);
  memset(&s, 0, sizeof s);
  memset(lim, 0, sizeof lim);
  lim[0].chr = 0; lim[0].name = name0; lim[0].start_pos = 0; lim[0].bp_length = 250000;
  lim[1].chr = 1; lim[1].name = name1; lim[1].start_pos = 1000; lim[1].bp_length = 101000;
  for (i = 0; i < NP; i++) { pts[i].chr = chr[i]; pts[i].sweep_pos = 1000 * (i + 1); pts[i].clr = clr[i]; pts[i].lalpha = log(0.001 * (i + 1)); }
  s.n_scan_pts = NP; s.scan_pts = pts; s.chr_limits = lim; s.n_chromosomes = NG;

  /* the rank order: descending, ties by index, a NaN last */
  fscl_amd_familywise_order(clr, NP, order);
  CHECK(order[0] == 4 && order[1] == 1 && order[2] == 0 && order[3] == 2 && order[4] == 3);
  fscl_amd_familywise_order(obs_nan, 4, o4);
  CHECK(o4[0] == 2 && o4[1] == 3 && o4[2] == 0 && o4[3] == 1);
  fscl_amd_familywise_order(NULL, 0, NULL);

  /* the chunk and the refusals */
  CHECK(fscl_amd_familywise_chunk(10, 5, 80) == 1 && fscl_amd_familywise_chunk(10, 5, 79) == 0);
  CHECK(fscl_amd_familywise_chunk(10, 5, 1000) == 5 && fscl_amd_familywise_chunk(0, 7, 8) == 1 && fscl_amd_familywise_chunk(3, 0, 800) == 0);
  unsetenv("FSCL_AMD_FWER_CAP");
  CHECK(fscl_amd_familywise_cap() == (size_t)1 << 28);
  CHECK(fscl_amd_familywise_check(&s, 100000, 10) == 0 && fscl_amd_familywise_error()[0] == 0);   /* 3 + 1 cells */
  CHECK(fscl_amd_familywise_check(&s, 100000, 0) == -1 && strstr(fscl_amd_familywise_error(), "--familywise-trials"));
  CHECK(fscl_amd_familywise_check(NULL, 100000, 1) == -1);
  setenv("FSCL_AMD_FWER_CAP", "31", 1);
  CHECK(fscl_amd_familywise_cap() == 31);
  CHECK(fscl_amd_familywise_check(&s, 100000, 10) == -1 && strstr(fscl_amd_familywise_error(), "FSCL_AMD_FWER_CAP=31"));
  setenv("FSCL_AMD_FWER_CAP", "32", 1);
  CHECK(fscl_amd_familywise_check(&s, 100000, 10) == 0);
  unsetenv("FSCL_AMD_FWER_CAP");

  /* the combine, the thresholds and the writers on M = 19 trials: k = 2, 1, 0 at levels .10, .05, .01 */
  memset(&f, 0, sizeof f);
  f.n = NP; f.n_groups = NG; f.trials = M; f.seed = 7;
  f.order = malloc(sizeof order); memcpy(f.order, order, sizeof order);
  f.c_single = calloc(NP, sizeof(int32_t)); f.c_chr = calloc(NP, sizeof(int32_t)); f.c_step = calloc(NP, sizeof(int32_t));
  f.gmax = malloc(sizeof(double) * M); f.garg = malloc(sizeof(int32_t) * M);
  f.chr_max = malloc(sizeof(double) * M * NG); f.chr_arg = malloc(sizeof(int32_t) * M * NG);
  for (t = 0; t < M; t++) {
    f.gmax[t] = t == 4 ? 30.0 : (double)t; f.garg[t] = t == 3 ? -1 : t % NP;   /* maxima 30, 18, 17, ... */
    f.chr_max[t * NG] = (double)t; f.chr_arg[t * NG] = 0;
    f.chr_max[t * NG + 1] = t == 3 ? -INFINITY : 0.5 * t; f.chr_arg[t * NG + 1] = t == 3 ? -1 : 3;
  }
  { /* c_step in rank order 0, 2, 1, 5, 19: the third rank is lifted to the second's value */
    static const int32_t cs[NP] = {17, 7, 17, 19, 0}, cc[NP] = {16, 6, 16, 19, 0}, ct[NP] = {1, 2, 5, 19, 0};
    memcpy(f.c_single, cs, sizeof cs); memcpy(f.c_chr, cc, sizeof cc); memcpy(f.c_step, ct, sizeof ct);
  }
  fscl_amd_familywise_combine(f.c_single, f.c_chr, f.c_step, f.order, NP, M, rank, ps, pc, pt);
  CHECK(rank[4] == 1 && rank[1] == 2 && rank[0] == 3 && rank[2] == 4 && rank[3] == 5);
  CHECK(ps[4] == 1.0 / 20 && ps[1] == 8.0 / 20 && pc[0] == 17.0 / 20 && ps[3] == 1.0);
  CHECK(pt[4] == 1.0 / 20 && pt[1] == 3.0 / 20 && pt[0] == 3.0 / 20 && pt[2] == 6.0 / 20 && pt[3] == 1.0);
  fscl_amd_familywise_combine(f.c_single, f.c_chr, f.c_step, f.order, NP, M, NULL, NULL, NULL, NULL);
  CHECK(fscl_amd_familywise_threshold(f.gmax, M, 0.10, &thr) == 2 && thr == 18.0);
  CHECK(fscl_amd_familywise_threshold(f.gmax, M, 0.05, &thr) == 1 && thr == 30.0);
  CHECK(fscl_amd_familywise_threshold(f.gmax, M, 0.01, &thr) == 0 && isnan(thr));
  CHECK(fscl_amd_familywise_threshold(f.gmax, M, 0.05, NULL) == 1 && fscl_amd_familywise_threshold(NULL, 0, 0.05, &thr) == 0);
  for (i = 0; i < NP; i++) { /* strictly above the threshold exactly when p_single <= a (counts consistent with the maxima) */
    int c = 0;
    for (t = 0; t < M; t++) c += f.gmax[t] >= clr[i];
    fscl_amd_familywise_threshold(f.gmax, M, 0.05, &thr);
    CHECK((clr[i] > thr) == ((1.0 + c) / (M + 1.0) <= 0.05));
    fscl_amd_familywise_threshold(f.gmax, M, 0.10, &thr);
    CHECK((clr[i] > thr) == ((1.0 + c) / (M + 1.0) <= 0.10));
  }
  snprintf(path, sizeof path, "%s/familywise_host_check.txt", dir);
  CHECK(fscl_amd_familywise_output(path, &s, &f, "lab") == 0);
  CHECK(fscl_amd_familywise_output("/nonexistent-directory/x.txt", &s, &f, NULL) == -1);
  CHECK(line_is(path, 1, "lab\tchrA\t1000\t3.00\t1.000e-03\t3\t8.500e-01\t9.000e-01\t1.500e-01\t0.824\n"));
  CHECK(line_is(path, 5, "lab\tx:1\t5000\t40.00\t5.000e-03\t1\t5.000e-02\t5.000e-02\t5.000e-02\t1.301\n"));
  CHECK(line_is(path, 6, "lab\tchrA\tsummary\t19\t3\t9.00\t17.00\t18.00\tNA\t0\t0\n"));
  CHECK(line_is(path, 7, "lab\tx:1\tsummary\t19\t2\t4.50\t8.50\t9.00\tNA\t1\t0\n"));
  CHECK(line_is(path, 8, "lab\tgenome\tsummary\t19\t5\t10.00\t18.00\t30.00\tNA\t1\t0\n"));
  CHECK(!line_is(path, 9, "") && fscl_amd_familywise_output(NULL, &s, &f, NULL) == 0);
  remove(path);
  snprintf(path, sizeof path, "%s/familywise_host_check_null.txt", dir);
  CHECK(fscl_amd_familywise_null_output(path, &s, &f, NULL) == 0);
  CHECK(line_is(path, 1, "0\t0.0000\tchrA\t1000\t0.0000\t0.0000\n"));
  CHECK(line_is(path, 4, "3\t3.0000\tNA\tNA\t3.0000\tNA\n"));
  CHECK(line_is(path, 5, "4\t30.0000\tx:1\t5000\t4.0000\t2.0000\n"));
  remove(path);
  f.n = NP - 1;
  CHECK(fscl_amd_familywise_output(path, &s, &f, NULL) == -1);   /* not one row per scan point */
  f.n = NP;
  fscl_amd_familywise_free(&f);
  CHECK(f.order == NULL && f.n == 0);
  fscl_amd_familywise_free(&f);
  fscl_amd_familywise_free(NULL);
  printf("ok\n");
  return 0;
}
