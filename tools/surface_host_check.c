/* surface_host_check.c -- a stand-alone exercise of the host-only side of the likelihood surfaces
 * (fscl_amd/csrc/host/surface.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/surface_host_check.c fscl_amd/csrc/host/surface.c fscl_amd/csrc/host/util.c -lm \
 *       -o /tmp/surface_host_check && /tmp/surface_host_check /tmp
 *
 * It needs no GPU and no device library: the alpha list with the fitted alpha inserted, a request's
 * clipped positions, the region summary on hand-made arrays and the --surface-file writer.  Exit
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
  char name0[] = "chrA";
  chr_limits_t lim[1];
  scan_t s;
  double la[FSCL_AMD_SURFACE_MAX_LA], *heap;
  fscl_amd_surface_req_t q;
  fscl_amd_surface_region_t g;
  fscl_amd_surfaces_t r;
  fsclg_run_t run;
  unsigned char mark[12];
  char path[4096], line[512];
  const char *dir = argc > 1 ? argv[1] : ".";
  int i, n;
  FILE *fp;

  configure_logmsg(1);
  memset(&s, 0, sizeof s);
  memset(lim, 0, sizeof lim);
  lim[0].name = name0; lim[0].start_pos = 1000; lim[0].bp_length = 9000;
  s.chr_limits = lim; s.n_chromosomes = 1;

  /* the alpha list: exactly FSCL_AMD_SURFACE_MAX_LA doubles are written at most */
  heap = malloc(sizeof(double) * FSCL_AMD_SURFACE_MAX_LA);
  CHECK(fscl_amd_surface_alphas(-20., 4., 63, 0.1, heap) == 64 && heap[0] == -20. && heap[63] == 4.);
  for (i = 1; i < 64; i++) CHECK(heap[i] > heap[i - 1]);
  free(heap);
  CHECK(fscl_amd_surface_alphas(-20., 4., 33, -20. + 0.75 * 7, la) == 33 && la[7] == -20. + 0.75 * 7);
  CHECK(fscl_amd_surface_alphas(-20., 4., 33, -14.8, la) == 34 && la[7] == -14.8 && la[6] == -15.5 && la[8] == -14.75);
  CHECK(fscl_amd_surface_alphas(-10., 0., 3, -12., la) == 4 && la[0] == -12. && la[1] == -10.);
  CHECK(fscl_amd_surface_alphas(-10., 0., 3, 2., la) == 4 && la[3] == 2. && la[2] == 0.);
  CHECK(fscl_amd_surface_alphas(-10., 0., 3, NAN, la) == 3 && fscl_amd_surface_alphas(-10., 0., 3, 5., la) == 3);
  CHECK(fscl_amd_surface_alphas(-3., -3., 1, NAN, la) == 1 && la[0] == -3.);
  CHECK(fscl_amd_surface_alphas(-20., 4., 64, NAN, la) == -1 && fscl_amd_surface_alphas(-20., 4., 0, NAN, la) == -1);
  CHECK(fscl_amd_surface_alphas(-21., 4., 5, NAN, la) == -1 && fscl_amd_surface_alphas(-20., 4.5, 5, NAN, la) == -1);
  CHECK(fscl_amd_surface_alphas(1., 0., 5, NAN, la) == -1 && fscl_amd_surface_alphas(1., 1., 2, NAN, la) == -1);
  CHECK(fscl_amd_surface_alphas(NAN, 1., 2, NAN, la) == -1 && fscl_amd_surface_alphas(0., 1., 2, NAN, NULL) == -1);

  /* a request's positions, clipped to [1000, 9000] */
  memset(&q, 0, sizeof q);
  q.chr = 0; q.centre_pos = 5000; q.halfwidth = 2500; q.step = 1000; q.n_la = 1; q.point = -1;
  CHECK(fscl_amd_surface_run(&s, &q, &run) == 0 && run.start_pos == 3000 && run.count == 5 && run.step == 1000);
  q.centre_pos = 1500;
  CHECK(fscl_amd_surface_run(&s, &q, &run) == 0 && run.start_pos == 1500 && run.count == 3);
  q.centre_pos = 8800;
  CHECK(fscl_amd_surface_run(&s, &q, &run) == 0 && run.start_pos == 6800 && run.count == 3);
  q.centre_pos = 500; q.halfwidth = 400;
  CHECK(fscl_amd_surface_run(&s, &q, &run) == 0 && run.count == 0);
  q.centre_pos = 20000; q.halfwidth = 100000; q.step = 3000;
  CHECK(fscl_amd_surface_run(&s, &q, &run) == 0 && run.start_pos == 2000 && run.count == 3);
  q.halfwidth = 0; q.centre_pos = 4000;
  CHECK(fscl_amd_surface_run(&s, &q, &run) == 0 && run.start_pos == 4000 && run.count == 1);
  q.step = 0; CHECK(fscl_amd_surface_run(&s, &q, &run) == -1);
  q.step = 1; q.chr = 1; CHECK(fscl_amd_surface_run(&s, &q, &run) == -1);
  q.chr = 0; q.halfwidth = -1; CHECK(fscl_amd_surface_run(&s, &q, &run) == -1);

  /* the region: 3 positions x 4 alphas, a ridge and a second maximum cut off by a low cell */
  {
    const double nul[3] = {-10., -10., -10.};
    double sm[12] = {-10., -9., -10., -9.5, /**/ -9., -5., -6., NAN, /**/ -10., -9., -10., -5.5};
    heap = malloc(sizeof sm); /* exact-size copies: a read past either end is caught */
    memcpy(heap, sm, sizeof sm);
    CHECK(fscl_amd_surface_region(heap, nul, 3, 4, 2.0, &g, mark) == 1);
    CHECK(g.max_ipos == 1 && g.max_ila == 1 && g.max_v == 5. && g.n_region == 2);
    CHECK(mark[5] == 2 && mark[6] == 1 && mark[11] == 0 && mark[7] == 0);
    CHECK(g.ipos_lo == 1 && g.ipos_hi == 2 && g.open_pos_lo == 0 && g.open_pos_hi == 1);
    CHECK(g.ila_lo == 1 && g.ila_hi == 3 && g.open_la_lo == 0 && g.open_la_hi == 1);
    CHECK(fscl_amd_surface_region(heap, nul, 3, 4, 2.0, &g, NULL) == 1 && g.n_region == 2);
    CHECK(fscl_amd_surface_region(heap, nul, 3, 4, -1.0, &g, NULL) == -1 && fscl_amd_surface_region(heap, nul, 3, 4, NAN, &g, NULL) == -1);
    CHECK(fscl_amd_surface_region(NULL, nul, 3, 4, 2.0, &g, NULL) == -1 && fscl_amd_surface_region(heap, nul, 0, 4, 2.0, &g, NULL) == -1);
    for (i = 0; i < 12; i++) heap[i] = NAN;
    CHECK(fscl_amd_surface_region(heap, nul, 3, 4, 2.0, &g, mark) == 0 && g.max_ipos == -1 && g.n_region == 0 && isnan(g.max_v));
    CHECK(g.open_pos_lo == 0 && g.open_la_hi == 0);
    heap[0] = -7.;
    CHECK(fscl_amd_surface_region(heap, nul, 1, 1, 2.0, &g, mark) == 1 && g.n_region == 1 && g.open_pos_lo && g.open_pos_hi &&
          g.open_la_lo && g.open_la_hi && mark[0] == 2);
    free(heap);

    /* the writer: two surfaces, the second all NaN */
    memset(&r, 0, sizeof r);
    r.n = 2; r.n_pos = 4; r.n_cells = 3 * 4 + 1 * 2;
    r.hdr = calloc(2, sizeof *r.hdr); r.pts = calloc(4, sizeof *r.pts); r.sm = malloc(sizeof(double) * 14);
    memcpy(r.sm, sm, sizeof sm);
    r.sm[12] = NAN; r.sm[13] = NAN;
    for (i = 0; i < 4; i++) { r.pts[i].null_logl = -10.; r.pts[i].sweep_pos = 2000 + 1000 * i; }
    r.hdr[0].centre_pos = 3000; r.hdr[0].n_pos = 3; r.hdr[0].n_la = 4; r.hdr[0].point = 0;
    for (i = 0; i < 4; i++) r.hdr[0].la[i] = log(1e-4) + i;
    r.hdr[1].centre_pos = 5000; r.hdr[1].n_pos = 1; r.hdr[1].n_la = 2; r.hdr[1].pos_off = 3; r.hdr[1].cell_off = 12;
    r.hdr[1].la[0] = 0.; r.hdr[1].la[1] = 1.;
  }
  snprintf(path, sizeof path, "%s/surface_host_check.txt", dir);
  CHECK(fscl_amd_surface_output(path, &s, &r, 2.0, "lab") == 0);
  CHECK(fscl_amd_surface_output("/nonexistent-directory/x.txt", &s, &r, 2.0, NULL) == -1);
  CHECK(fscl_amd_surface_output(path, &s, &r, -1.0, NULL) == -1);
  fp = fopen(path, "r");
  CHECK(fp != NULL);
  for (n = 0; fgets(line, sizeof line, fp);) {
    n++;
    if (n == 1) CHECK(!strcmp(line, "lab\tchrA\t3000\t2000\t1.000e-04\t0.00\t-\n"));
    if (n == 6) CHECK(!strcmp(line, "lab\tchrA\t3000\t3000\t2.718e-04\t10.00\t*\n"));
    if (n == 7) CHECK(!strcmp(line, "lab\tchrA\t3000\t3000\t7.389e-04\t8.00\t+\n"));
    if (n == 8) CHECK(!strcmp(line, "lab\tchrA\t3000\t3000\t2.009e-03\tnan\t-\n") || !strcmp(line, "lab\tchrA\t3000\t3000\t2.009e-03\t-nan\t-\n"));
    if (n == 13) CHECK(!strcmp(line, "lab\tchrA\t3000\tsummary\t3\t4\t3000\t2.718e-04\t10.00\t3000\t4000\t0\t1\t2.718e-04\t2.009e-03\t0\t1\t2\n"));
    if (n == 16) CHECK(!strcmp(line, "lab\tchrA\t5000\tsummary\t1\t2\tNA\tNA\tNA\tNA\tNA\t0\t0\tNA\tNA\t0\t0\t0\n"));
  }
  CHECK(n == 16);
  fclose(fp);
  remove(path);
  r.hdr[1].cell_off = 13; /* a header past the arrays */
  CHECK(fscl_amd_surface_output(path, &s, &r, 2.0, NULL) == -1);
  fscl_amd_surfaces_free(&r);
  CHECK(r.hdr == NULL && r.n == 0);
  fscl_amd_surfaces_free(&r);
  printf("ok\n");
  return 0;
}
