/* simulate_host_check.c -- a stand-alone exercise of the host-only side of the simulation and the
 * bootstrap (fscl_amd/csrc/host/simulate.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/simulate_host_check.c fscl_amd/csrc/host/simulate.c fscl_amd/csrc/host/input.c \
 *       fscl_amd/csrc/host/util.c -lm -o /tmp/simulate_host_check && /tmp/simulate_host_check /tmp
 *
 * It needs no GPU and no device library: sweep parsing, the nearest-sweep rule, the sampler's
 * table transposition, the replicate scan with its folding, the SNP-format writer read back by
 * load_snp_input, and the bootstrap's quantile summary.  Exit status 0 and "ok" when every check
 * holds. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fscl_amd/csrc/host/fscl_host.h"

char *prepend_label, *output_fname;
int spline_pts, n_permute;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

enum { NS = 12, N_IV = 5 };

static spline_t *make_spline(int depth, int f) {
  spline_t *sp = malloc(sizeof *sp);
  double *flat = malloc(sizeof(double) * N_IV * 4);
  int iv, k;
  sp->n = N_IV;
  sp->knot_points = NULL;
  sp->coef = malloc(sizeof(double *) * N_IV);
  for (iv = 0; iv < N_IV; iv++) {
    sp->coef[iv] = flat + iv * 4;
    for (k = 0; k < 4; k++) sp->coef[iv][k] = 1000. * depth + 100. * f + 10. * iv + k;
  }
  return sp;
}

int main(int argc, char **argv) {
  static const int pos[NS] = {10, 20, 30, 40, 50, 60, 5, 15, 25, 35, 45, 55};
  static const int dp[NS] = {0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 1};
  static const int fo[NS] = {0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 1};
  static const int freq[NS] = {7, 5, 6, 1, 1, 4, 2, 3, 5, 2, 7, 3};
  int depths[2] = {8, 6};
  char name0[] = "chrA", name1[] = "x:1";
  chr_limits_t lim[2] = {{0, name0, 0, 6, 10, 60}, {1, name1, 6, 6, 5, 55}};
  snp_t snps[NS];
  scan_t s = {NS, snps, 2, depths, 0, NULL, lim, 2}, *r, *back;
  sm_ptable_t sm[2];
  fscl_amd_sweep_t sw[4], one;
  fscl_amd_boot_t bt[2 * 5];
  double *coef_t, *neutral, fsp0[9], fsp1[7];
  int32_t dn[2];
  char path[4096];
  int i, d, f, iv, k, n_iv;
  const char *dir = argc > 1 ? argv[1] : ".";

  configure_logmsg(1);
  for (i = 0; i < NS; i++) {
    snps[i].chr = i < 6 ? 0 : 1; snps[i].pos = pos[i]; snps[i].null_logl = -2.5;
    snps[i].obs_freq = 1; snps[i].depth_p = dp[i]; snps[i].folded = fo[i];
  }

  /* sweep parsing */
  CHECK(fscl_amd_parse_sweep(&s, "chrA:35:1e-4", &one) == 0 && one.chr == 0 && one.pos == 35 && one.alpha == 1e-4);
  CHECK(fscl_amd_parse_sweep(&s, "x:1:-7:2.5", &one) == 0 && one.chr == 1 && one.pos == -7 && one.alpha == 2.5);
  CHECK(fscl_amd_parse_sweep(&s, "chrB:35:1e-4", &one) == -2);
  CHECK(fscl_amd_parse_sweep(&s, "chrA:35:0", &one) == -3 && fscl_amd_parse_sweep(&s, "chrA:35:-1", &one) == -3);
  CHECK(fscl_amd_parse_sweep(&s, "chrA:35:nan", &one) == -3 && fscl_amd_parse_sweep(&s, "chrA:35:inf", &one) == -3);
  CHECK(fscl_amd_parse_sweep(&s, "chrA:35", &one) == -1 && fscl_amd_parse_sweep(&s, "", &one) == -1);
  CHECK(fscl_amd_parse_sweep(&s, ":", &one) == -1 && fscl_amd_parse_sweep(&s, "::", &one) == -1);
  CHECK(fscl_amd_parse_sweep(&s, "chrA:3x:1", &one) == -1 && fscl_amd_parse_sweep(&s, "chrA:35:1z", &one) == -1);
  CHECK(fscl_amd_parse_sweep(&s, "chrA:99999999999:1", &one) == -1);

  /* the nearest sweep */
  sw[0] = (fscl_amd_sweep_t){0, 40, 1e-3}; sw[1] = (fscl_amd_sweep_t){0, 20, 2e-3};
  sw[2] = (fscl_amd_sweep_t){0, 40, 3e-3}; sw[3] = (fscl_amd_sweep_t){0, 2147483647, 1e-3};
  CHECK(fscl_amd_nearest_sweep(sw, 4, 0, 30) == 1);   /* equidistant: the lower position */
  CHECK(fscl_amd_nearest_sweep(sw, 4, 0, 31) == 0);   /* two sweeps on one position: the first */
  CHECK(fscl_amd_nearest_sweep(sw, 4, 0, -2147483647) == 1 && fscl_amd_nearest_sweep(sw, 4, 0, 2147483647) == 3);
  CHECK(fscl_amd_nearest_sweep(sw, 4, 1, 30) == -1 && fscl_amd_nearest_sweep(NULL, 0, 0, 30) == -1);

  /* the sampler's tables: [depth][interval][f][c0..c3], and fsp[1 .. n-1] */
  for (d = 0; d < 2; d++) {
    const int n = depths[d];
    sm[d].sample_size = n;
    sm[d].spline_func = malloc(sizeof(spline_t *) * (n + 1));
    sm[d].fspline_func = NULL; sm[d].pbk = NULL;
    sm[d].fsp = d ? fsp1 : fsp0;
    for (f = 0; f <= n; f++) { sm[d].spline_func[f] = make_spline(d, f); sm[d].fsp[f] = d + f / 16.; }
  }
  fscl_amd_sample_tables_build(sm, 2, &coef_t, &neutral, dn, &n_iv);
  CHECK(n_iv == N_IV && dn[0] == 8 && dn[1] == 6);
  for (d = 0; d < 2; d++) {
    const int m = depths[d] - 1;
    const double *c = coef_t + (d ? (size_t)N_IV * 7 * 4 : 0), *q = neutral + (d ? 7 : 0);
    for (f = 1; f <= m; f++) {
      CHECK(q[f - 1] == d + f / 16.);
      for (iv = 0; iv < N_IV; iv++)
        for (k = 0; k < 4; k++) CHECK(c[((size_t)iv * m + (f - 1)) * 4 + k] == 1000. * d + 100. * f + 10. * iv + k);
    }
  }
  free(coef_t); free(neutral);

  /* the replicate: folded, independent, written and read back */
  r = fscl_amd_simulate_scan(&s, freq);
  CHECK(r && r->n_snps == NS && r->snps != snps && r->chr_limits != lim && r->chr_limits[1].name != name1);
  CHECK(r->n_scan_pts == 0 && r->scan_pts == NULL && !strcmp(r->chr_limits[1].name, "x:1"));
  for (i = 0; i < NS; i++) {
    const int n = depths[dp[i]], want = fo[i] && freq[i] > n - freq[i] ? n - freq[i] : freq[i];
    CHECK(r->snps[i].obs_freq == want && r->snps[i].pos == pos[i] && r->snps[i].null_logl == 0.0);
  }
  snprintf(path, sizeof path, "%s/simulate_host_check.snp", dir);
  CHECK(fscl_amd_simulate_output(path, r) == 0);
  CHECK(fscl_amd_simulate_output("/nonexistent-directory/x.snp", r) == -1);
  back = load_snp_input(path, 0, 5);
  CHECK(back->n_snps == NS && back->n_chromosomes == 2 && back->n_depths == 2);
  for (i = 0; i < NS; i++) { /* (load_snp_input sorts by position within a chromosome) */
    int j;
    for (j = 0; j < NS; j++)
      if (back->snps[j].chr == r->snps[i].chr && back->snps[j].pos == r->snps[i].pos) break;
    CHECK(j < NS && back->snps[j].obs_freq == r->snps[i].obs_freq && back->snps[j].folded == r->snps[i].folded);
    CHECK(back->sample_depths[back->snps[j].depth_p] == depths[dp[i]]);
  }
  fscl_amd_scan_free(back);
  fscl_amd_scan_free(r);
  remove(path);

  /* the bootstrap file: 5 replicates of 2 sweeps, one sweep never found */
  memset(bt, 0, sizeof bt);
  for (i = 0; i < 10; i++) {
    bt[i].sweep = i / 5; bt[i].rep = i % 5; bt[i].chr = 0; bt[i].planted_pos = 40; bt[i].planted_alpha = 1e-3;
    bt[i].est_pos = i < 5 && i != 2 ? 30 + i : -1;
    bt[i].est_lalpha = i < 5 && i != 2 ? log(1e-3 * (5 - i)) : NAN;
    bt[i].clr = i < 5 && i != 2 ? 3.5 * i : NAN;
  }
  snprintf(path, sizeof path, "%s/simulate_host_check.boot", dir);
  fscl_amd_bootstrap_output(path, &s, sw, 2, 5, bt, "lab");
  {
    FILE *fp = fopen(path, "r");
    char line[512];
    int n = 0;
    CHECK(fp != NULL);
    while (fgets(line, sizeof line, fp)) {
      n++;
      if (n == 3) CHECK(!strcmp(line, "lab\tchrA\t40\t1.000e-03\t2\tNA\tNA\tNA\n"));
      if (n == 6) CHECK(!strcmp(line, "lab\tchrA\t40\tsummary\t5\t4\t30\t31\t33\t1.000e-03\t2.000e-03\t4.000e-03\t3.50\n"));
      if (n == 12) CHECK(!strcmp(line, "lab\tchrA\t20\tsummary\t5\t0\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"));
    }
    CHECK(n == 12);
    fclose(fp);
  }
  fscl_amd_bootstrap_output(path, &s, sw, 2, 0, NULL, NULL);  /* no replicate: two summaries of nothing */
  fscl_amd_bootstrap_output(path, &s, NULL, 0, 5, NULL, NULL);
  remove(path);
  for (d = 0; d < 2; d++) {
    for (f = 0; f <= depths[d]; f++) {
      free(sm[d].spline_func[f]->coef[0]); free(sm[d].spline_func[f]->coef); free(sm[d].spline_func[f]);
    }
    free(sm[d].spline_func);
  }
  printf("ok\n");
  return 0;
}
