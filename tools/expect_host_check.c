/* expect_host_check.c -- a stand-alone exercise of the host-only side of the expected terms under
 * the model (fscl_amd/csrc/host/expect.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/expect_host_check.c fscl_amd/csrc/host/expect.c fscl_amd/csrc/host/util.c -lm \
 *       -o /tmp/expect_host_check && /tmp/expect_host_check /tmp
 *
 * It needs no GPU and no device library: the folded-row and null-value tables with their index
 * arithmetic (an odd and an even depth, the smallest depth 2), the bins, every refusal with its
 * message, the size limit, and the writer read back line by line.  Exit status 0 and "ok" when
 * every check holds. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fscl_amd/csrc/host/fscl_host.h"

char *prepend_label, *output_fname;
int spline_pts, n_permute;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

enum { N_IV = 5, ND = 3 };

static spline_t *make_spline(int depth, int f, int folded) {
  spline_t *sp = malloc(sizeof *sp);
  double *flat = malloc(sizeof(double) * N_IV * 4);
  int iv, k;
  sp->n = N_IV;
  sp->knot_points = NULL;
  sp->coef = malloc(sizeof(double *) * N_IV);
  for (iv = 0; iv < N_IV; iv++) {
    sp->coef[iv] = flat + iv * 4;
    for (k = 0; k < 4; k++) sp->coef[iv][k] = (folded ? 0.5 : 0.) + 1000. * depth + 100. * f + 10. * iv + k;
  }
  return sp;
}
static void free_spline(spline_t *sp) { free(sp->coef[0]); free(sp->coef); free(sp); }

static int refused(const scan_t *s, const fsclg_site_req_t *req, int n, const double *la, int n_la, int n_bins, const char *msg) {
  return fscl_amd_expect_check(s, req, n, la, n_la, n_bins) == -1 && strstr(fscl_amd_expect_error(), msg) != NULL;
}

int main(int argc, char **argv) {
  static const int depths[ND] = {7, 6, 2};
  char name0[] = "chrA", name1[] = "x:1";
  chr_limits_t lim[2] = {{0, name0, 0, 6, 10, 60}, {1, name1, 6, 6, 5, 55}};
  scan_t s = {0, NULL, ND, (int *)depths, 0, NULL, lim, 2};
  sm_ptable_t sm[ND];
  double *bg[ND], *adj[ND];
  double *fc, *ne, *nu, *nf, la[70];
  int32_t dn[ND];
  fsclg_site_req_t req[3] = {{0, 35, -9.0}, {1, 20, -2.0}, {0, 10, 4.0}};
  char path[4096];
  const char *dir = argc > 1 ? argv[1] : ".";
  int d, f, iv, k, n_iv, i;
  size_t fo = 0, uo = 0, no = 0;

  configure_logmsg(1);

  /* the tables: folded rows [depth][interval][c][c0..c3], c = 1 .. n/2; the tables' fsp as the neutral spectrum; the
     null values from the background by compute_snp_null_model's two expressions */
  for (d = 0; d < ND; d++) {
    const int n = depths[d];
    bg[d] = malloc(sizeof(double) * (size_t)(n + 1));
    adj[d] = malloc(sizeof(double) * (size_t)(n + 1));
    for (f = 0; f <= n; f++) { bg[d][f] = (f + 1.) / 64. + d / 8.; adj[d][f] = (f + 2.) / 128.; }
    if (d == 1) bg[d][2] = 0.;   /* a class the background never saw: log 0 */
    sm[d].sample_size = n;
    sm[d].pbk = NULL;
    sm[d].fsp = adj[d];
    sm[d].spline_func = malloc(sizeof(spline_t *) * (size_t)(n + 1));
    sm[d].fspline_func = malloc(sizeof(spline_t *) * (size_t)(n / 2 + 1));
    for (f = 0; f <= n; f++) sm[d].spline_func[f] = make_spline(d, f, 0);
    for (f = 0; f <= n / 2; f++) sm[d].fspline_func[f] = make_spline(d, f, 1);
  }
  fscl_amd_expect_tables_build(sm, bg, ND, &fc, &ne, &nu, &nf, dn, &n_iv);
  CHECK(n_iv == N_IV);
  for (d = 0; d < ND; d++) {
    const int n = depths[d], nh = n / 2;
    CHECK(dn[d] == n);
    for (f = 1; f < n; f++) {
      CHECK(ne[uo + f - 1] == adj[d][f]);
      if (d == 1 && f == 2) CHECK(isinf(nu[uo + f - 1]) && nu[uo + f - 1] < 0);
      else CHECK(nu[uo + f - 1] == log(bg[d][f]));
    }
    for (f = 1; f <= nh; f++) {
      CHECK(nf[no + f - 1] == (f != n - f ? log(bg[d][f] + bg[d][n - f]) : log(bg[d][f])));
      for (iv = 0; iv < N_IV; iv++)
        for (k = 0; k < 4; k++) CHECK(fc[fo + ((size_t)iv * nh + (f - 1)) * 4 + k] == 0.5 + 1000. * d + 100. * f + 10. * iv + k);
    }
    fo += (size_t)N_IV * nh * 4; uo += (size_t)(n - 1); no += (size_t)nh;
  }
  CHECK(fo == (size_t)N_IV * 4 * (3 + 3 + 1) && uo == 6 + 5 + 1 && no == 3 + 3 + 1);
  free(fc); free(ne); free(nu); free(nf);

  /* the bins */
  CHECK(fscl_amd_expect_bin(-25., 24) == 0 && fscl_amd_expect_bin(-20., 24) == 0 && fscl_amd_expect_bin(-19., 24) == 1);
  CHECK(fscl_amd_expect_bin(4., 24) == 23 && fscl_amd_expect_bin(3.999, 24) == 23 && fscl_amd_expect_bin(2.999, 24) == 22);
  CHECK(fscl_amd_expect_bin(NAN, 24) == 0 && fscl_amd_expect_bin(1e300, 64) == 63 && fscl_amd_expect_bin(0., 1) == 0);

  /* the refusals, each naming its option */
  for (i = 0; i < 70; i++) la[i] = -20. + i * (24. / 69.);
  CHECK(fscl_amd_expect_check(&s, req, 3, la, 64, 24) == 0 && fscl_amd_expect_error()[0] == 0);
  CHECK(fscl_amd_expect_check(&s, NULL, 0, la, 1, 1) == 0);
  CHECK(refused(&s, req, 3, la, 64, 0, "--expect-bins") && refused(&s, req, 3, la, 64, 65, "--expect-bins"));
  CHECK(refused(&s, req, 3, la, 0, 24, "--expect-alphas") && refused(&s, req, 3, la, 65, 24, "--expect-alphas"));
  CHECK(refused(&s, req, 3, NULL, 3, 24, "--expect-alphas"));
  { double bad[3] = {-3., -3., 0.}; CHECK(refused(&s, req, 3, bad, 3, 24, "--expect-alphas")); }
  { double bad[2] = {-20.5, 0.}; CHECK(refused(&s, req, 3, bad, 2, 24, "--expect-alphas")); }
  { double bad[2] = {0., NAN}; CHECK(refused(&s, req, 3, bad, 2, 24, "--expect-alphas")); }
  { fsclg_site_req_t q = {2, 35, -9.}; CHECK(refused(&s, &q, 1, la, 3, 24, "unknown chromosome")); }
  { fsclg_site_req_t q = {-1, 35, -9.}; CHECK(refused(&s, &q, 1, la, 3, 24, "unknown chromosome")); }
  { fsclg_site_req_t q = {0, 35, 4.5}; CHECK(refused(&s, &q, 1, la, 3, 24, "--expect-sweep: alpha")); }
  { fsclg_site_req_t q = {0, 35, NAN}; CHECK(refused(&s, &q, 1, la, 3, 24, "--expect-sweep: alpha")); }
  { fsclg_site_req_t q = {0, 2147483647, -9.}; CHECK(refused(&s, &q, 1, la, 3, 24, "past the int range")); }
  CHECK(refused(NULL, req, 3, la, 3, 24, "NULL") && refused(&s, NULL, 3, la, 3, 24, "NULL"));
  CHECK(fscl_amd_expect_cap() == (size_t)1 << 30);
  setenv("FSCL_AMD_EXPECT_CAP", "5000", 1);
  CHECK(fscl_amd_expect_cap() == 5000 && refused(&s, req, 3, la, 3, 24, "FSCL_AMD_EXPECT_CAP"));
  CHECK(fscl_amd_expect_check(&s, req, 1, la, 1, 1) == 0);
  setenv("FSCL_AMD_EXPECT_CAP", "junk", 1);
  CHECK(fscl_amd_expect_cap() == (size_t)1 << 30);
  unsetenv("FSCL_AMD_EXPECT_CAP");

  /* the writer: two requests and 3 bins; request 0's list is (own, other), its bin 1 empty and bin 2 with SD 0;
     request 1's walk is empty */
  {
    fscl_amd_expect_t r, z;
    int first[3] = {0, 2, 3}, own[2] = {0, 0};
    double rl[3] = {log(1e-4), log(1e-2), log(2e-3)};
    fsclg_site_req_t rq[2] = {{0, 1234, 0.}, {1, 777, 0.}};
    fsclg_site_hdr_t hdr[3];
    fsclg_expect_tot_t tot[3 * 4];
    FILE *fp;
    char line[512];
    int n = 0;
    memset(&r, 0, sizeof r); memset(hdr, 0, sizeof hdr); memset(tot, 0, sizeof tot);
    rq[0].lalpha = rl[0]; rq[1].lalpha = rl[2];
    hdr[0].pt.chr = hdr[1].pt.chr = 0; hdr[2].pt.chr = 1;
    hdr[0].pt.sweep_pos = hdr[1].pt.sweep_pos = 1234; hdr[2].pt.sweep_pos = 777;
    tot[0] = (fsclg_expect_tot_t){2, 0, 1.5, 1.0, 0.25, -0.5, 1.0, 0., 0.};
    tot[2] = (fsclg_expect_tot_t){1, 1, 0.25, 0., 0., 0., 0., 0., 0.};
    tot[3] = (fsclg_expect_tot_t){3, 1, 1.75, 1.0, 0.25, -0.5, 1.0, 1e-3, 0.};
    tot[4 + 3] = (fsclg_expect_tot_t){5, 0, 0., 2.0, 1.0, 0., 1.0, 0., 0.};
    r.n = 2; r.n_tasks = 3; r.n_bins = 3; r.req = rq; r.first = first; r.own = own; r.la = rl; r.hdr = hdr; r.tot = tot;
    snprintf(path, sizeof path, "%s/expect_host_check.txt", dir);
    CHECK(fscl_amd_expect_output(path, &s, &r, "lab") == 0);
    CHECK(fscl_amd_expect_output("/nonexistent-directory/x.txt", &s, &r, NULL) == -1);
    CHECK(fscl_amd_expect_output(path, NULL, &r, NULL) == -1 && fscl_amd_expect_output(path, &s, NULL, NULL) == -1);
    fp = fopen(path, "r");
    CHECK(fp != NULL);
    while (fgets(line, sizeof line, fp)) {
      n++;
      if (n == 1) CHECK(!strcmp(line, "lab\tchrA\t1234\t1.000e-04\tbin\t-20.0000\t-12.0000\t2\t3.0000\t2.0000\t1.0000\t1.0000\t-1.0000\t2.0000\t2.0000\n"));
      if (n == 2) CHECK(!strcmp(line, "lab\tchrA\t1234\t1.000e-04\tbin\t-4.0000\t4.0000\t1\t0.5000\t0.0000\t0.0000\tNA\t0.0000\t0.0000\tNA\n"));
      if (n == 3) CHECK(!strcmp(line, "lab\tchrA\t1234\t1.000e-04\tcurve\t1.000e-04\t3\t2.0000\t1.0000\t-1.0000\t2.0000\t1.8974\n"));
      if (n == 5) CHECK(!strcmp(line, "lab\tchrA\t1234\t1.000e-04\tsummary\t3\t1\t3.5000\t2.0000\t1.0000\t1.5000\t-1.0000\t2.0000\t2.2500\t1.000e-03\t0.000e+00\n"));
      if (n == 6) CHECK(!strcmp(line, "lab\tx:1\t777\t2.000e-03\tcurve\t2.000e-03\t0\t0.0000\t0.0000\t0.0000\t0.0000\tNA\n"));
      if (n == 7) CHECK(!strcmp(line, "lab\tx:1\t777\t2.000e-03\tsummary\t0\t0\t0.0000\t0.0000\t0.0000\tNA\t0.0000\t0.0000\tNA\t0.000e+00\t0.000e+00\n"));
    }
    CHECK(n == 7);
    fclose(fp);
    /* a rank that evaluated nothing writes nothing and reports success; a result of no requests is an empty file */
    memset(&z, 0, sizeof z);
    CHECK(fscl_amd_expect_output(path, &s, &z, NULL) == 0);
    r.n = 0; r.n_tasks = 0;
    CHECK(fscl_amd_expect_output(path, &s, &r, NULL) == 0);
    fp = fopen(path, "r");
    CHECK(fp != NULL && fgets(line, sizeof line, fp) == NULL);
    fclose(fp);
    remove(path);
    /* fscl_amd_expect_free on a malloc'd result, and on an empty one */
    memset(&r, 0, sizeof r);
    r.req = malloc(8); r.first = malloc(8); r.own = malloc(8); r.la = malloc(8); r.hdr = malloc(8); r.tot = malloc(8);
    r.point = malloc(8);
    fscl_amd_expect_free(&r);
    CHECK(r.req == NULL && r.n == 0);
    fscl_amd_expect_free(&r);
    fscl_amd_expect_free(NULL);
  }

  for (d = 0; d < ND; d++) {
    for (f = 0; f <= depths[d]; f++) free_spline(sm[d].spline_func[f]);
    for (f = 0; f <= depths[d] / 2; f++) free_spline(sm[d].fspline_func[f]);
    free(sm[d].spline_func); free(sm[d].fspline_func); free(bg[d]); free(adj[d]);
  }
  printf("ok\n");
  return 0;
}
