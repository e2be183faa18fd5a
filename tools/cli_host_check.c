/* cli_host_check.c -- a stand-alone exercise of the `fscl` command line's argument loop and its
 * check-and-resolve pass (fscl_amd/csrc/host/cli_options.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/cli_host_check.c fscl_amd/csrc/host/cli_options.c fscl_amd/csrc/host/surface.c \
 *       fscl_amd/csrc/host/util.c -lm -o /tmp/cli_host_check && /tmp/cli_host_check
 *
 * It needs no GPU, no device library and no input file: a table of argument vectors, and for each
 * the resolved option record field by field -- every default that follows another option, in its
 * given and its not-given state (g is -g, G is -G):
 *
 *   bootstrap_window     G                        jackknife_block      max(G / 2, 1)
 *   surface_halfwidth    G                        jackknife_halfwidth  the resolved surface half-width
 *   surface_step         g with --surface-file,   jackknife_step       the given --surface-step, else g
 *                        else 1                   cond_step            g
 *   the jackknife, conditional and expect alpha grids: the surface's
 *
 * and the strictly parsed options at the ends of their ranges.  The refusals print their messages
 * to stderr as the program does.  Exit status 0 and "ok" when every check holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fscl_amd/csrc/host/cli_options.h"

char *prepend_label, *output_fname;
int spline_pts, n_permute;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s (after \"%s\")\n", __FILE__, __LINE__, #c, g_args); exit(1); } } while (0)

static const char *g_args = "";
static cli_opts_t o;

/* "fscl -f in -o out" and the blank-separated `args` through cli_parse and cli_check: 0 accepted,
   1 refused, else cli_parse's exit code + 1000 */
static int run(const char *args) {
  char buf[1024], *argv[64] = {"fscl", "-f", "in", "-o", "out"}, *t;
  int argc = 5, r;
  cli_opts_free(&o);
  g_args = args;
  snprintf(buf, sizeof buf, "%s", args);
  for (t = strtok(buf, " "); t && argc < 63; t = strtok(NULL, " ")) argv[argc++] = t;
  r = cli_parse(argc, argv, &o);
  return r >= 0 ? 1000 + r : cli_check(&o);
}

static int grid_is(const alpha_grid_t *g, double lo, double hi, int n) { return g->lo == lo && g->hi == hi && g->n == n; }

int main(void) {
  char *none[] = {"fscl"};
  memset(&o, 0, sizeof o);

  /* the argument loop */
  CHECK(cli_parse(1, none, &o) == 255);
  CHECK(run("--help") == 1000);
  CHECK(run("--sites-top") == 1255 && run("-g") == 1255 && run("--snpfile in2") == 1255);
  CHECK(run("--no-such-option=1 -Z") == 0);
  CHECK(run("--no-scan") == 0 && o.dont_scan == 1);
  CHECK(run("--no-scan --no-scan") == 0 && o.dont_scan == 0);
  CHECK(run("-g 250 --coarse-grid-spacing=5000 -p 7 --prepend-label=L -w 0.5") == 0);
  CHECK(o.small_grid_sp == 250 && o.large_grid_sp == 5000 && o.n_permute == 7 && !strcmp(o.prepend_label, "L") && o.scan_width_mb == 0.5);
  CHECK(!strcmp(o.snp_fname, "in") && !strcmp(o.output_fname, "out") && !o.ms_fname);
  CHECK(run("--given-sweep=a:1:1e-3 --conditional-file=c --given-sweep=b:2:1e-2") == 0);
  CHECK(o.given_sweep.n == 2 && !strcmp(o.given_sweep.v[0], "a:1:1e-3") && !strcmp(o.given_sweep.v[1], "b:2:1e-2"));

  /* nothing given: every default of the table, from g = 1000 and G = 100000 */
  CHECK(run("") == 0);
  CHECK(o.bootstrap_window == 100000 && o.surface_halfwidth == 100000 && o.surface_step == 1);
  CHECK(o.jackknife_step == 1000 && o.jackknife_block == 50000 && o.jackknife_halfwidth == 100000 && o.cond_step == 1000);
  CHECK(grid_is(&o.surface_grid, -20.0, 4.0, 33) && grid_is(&o.jackknife_grid, -20.0, 4.0, 33));
  CHECK(grid_is(&o.cond_grid, -20.0, 4.0, 33) && grid_is(&o.expect_grid, -20.0, 4.0, 33));
  CHECK(o.tail_df == 2 && o.tail_min_n == 20 && o.fw_trials == 1000 && o.cond_halfwidth == 0 && o.cond_rounds == 1);
  CHECK(o.cond_min_clr == 0.0 && o.expect_top == 3 && o.expect_bins == 24 && o.sites_top == 10 && o.surface_top == 3);
  CHECK(!o.grid_mode && !o.throughput && o.minimum_obs_depth == 5 && o.spline_pts == N_SPLINE_KNOTS);

  /* not given, from other g and G; --surface-file turns the surface step to g */
  CHECK(run("-g 500 -G 20000") == 0);
  CHECK(o.bootstrap_window == 20000 && o.surface_halfwidth == 20000 && o.surface_step == 1 && o.jackknife_step == 500);
  CHECK(o.jackknife_block == 10000 && o.jackknife_halfwidth == 20000 && o.cond_step == 500);
  CHECK(run("-g 500 -G 20000 --surface-file=s") == 0);
  CHECK(o.surface_step == 500 && o.jackknife_step == 500 && o.surface_halfwidth == 20000);
  CHECK(run("-g 1 -G 3") == 0 && o.jackknife_block == 1);
  CHECK(run("-g 1 -G 1") == 0 && o.jackknife_block == 1);
  CHECK(run("-g 1 -G 4") == 0 && o.jackknife_block == 2);

  /* given: the surface's values reach the jackknife, with or without --surface-file */
  CHECK(run("--bootstrap-window=7") == 0 && o.bootstrap_window == 7);
  CHECK(run("--bootstrap-window=0") == 0 && o.bootstrap_window == 0);
  CHECK(run("--surface-halfwidth=300 --surface-step=25") == 0);
  CHECK(o.surface_halfwidth == 300 && o.jackknife_halfwidth == 300 && o.surface_step == 25 && o.jackknife_step == 25);
  CHECK(run("--surface-file=s --surface-halfwidth=0 --surface-step=25 -g 500") == 0);
  CHECK(o.surface_halfwidth == 0 && o.jackknife_halfwidth == 0 && o.surface_step == 25 && o.jackknife_step == 25 && o.cond_step == 500);
  CHECK(run("--surface-halfwidth=300 --surface-step=25 --jackknife-halfwidth=5 --jackknife-step=9 --jackknife-block=77") == 0);
  CHECK(o.surface_halfwidth == 300 && o.surface_step == 25 && o.jackknife_halfwidth == 5 && o.jackknife_step == 9 && o.jackknife_block == 77);
  CHECK(run("--conditional-file=c --conditional-step=40 -g 500") == 0 && o.cond_step == 40);
  /* the sentinels mean "not given"; another negative half-width is refused */
  CHECK(run("--surface-step=-1 --surface-halfwidth=-1 --jackknife-step=-1 --jackknife-halfwidth=-1 --jackknife-block=-1 "
            "--bootstrap-window=-1 -g 500 -G 20000") == 0);
  CHECK(o.surface_step == 1 && o.surface_halfwidth == 20000 && o.jackknife_step == 500 && o.jackknife_halfwidth == 20000);
  CHECK(o.jackknife_block == 10000 && o.bootstrap_window == 20000);
  CHECK(run("--surface-halfwidth=-5") == 1 && run("--surface-halfwidth=-5 --jackknife-halfwidth=10") == 1);
  CHECK(run("--surface-step=0") == 1 && run("--jackknife-step=0") == 1 && run("--jackknife-block=0") == 1);

  /* the alpha grids */
  CHECK(run("--surface-alphas=-10:2:5") == 0);
  CHECK(grid_is(&o.surface_grid, -10.0, 2.0, 5) && grid_is(&o.jackknife_grid, -10.0, 2.0, 5));
  CHECK(grid_is(&o.cond_grid, -10.0, 2.0, 5) && grid_is(&o.expect_grid, -10.0, 2.0, 5));
  CHECK(run("--surface-alphas=-10:2:5 --jackknife-alphas=-3:3:7") == 0);
  CHECK(grid_is(&o.jackknife_grid, -3.0, 3.0, 7) && grid_is(&o.cond_grid, -10.0, 2.0, 5) && grid_is(&o.expect_grid, -10.0, 2.0, 5));
  CHECK(run("--surface-alphas=-10:2:5 --conditional-file=c --conditional-alphas=-4:0:3") == 0);
  CHECK(grid_is(&o.cond_grid, -4.0, 0.0, 3) && grid_is(&o.jackknife_grid, -10.0, 2.0, 5) && grid_is(&o.expect_grid, -10.0, 2.0, 5));
  CHECK(run("--surface-alphas=-10:2:5 --expect-file=e --expect-alphas=1:1:1") == 0);
  CHECK(grid_is(&o.expect_grid, 1.0, 1.0, 1) && grid_is(&o.cond_grid, -10.0, 2.0, 5) && grid_is(&o.surface_grid, -10.0, 2.0, 5));
  CHECK(run("--jackknife-alphas=-20:4:63") == 0 && grid_is(&o.jackknife_grid, -20.0, 4.0, 63) && grid_is(&o.surface_grid, -20.0, 4.0, 33));
  CHECK(run("--surface-alphas=-20:4:64") == 1 && run("--jackknife-alphas=-21:4:9") == 1 && run("--surface-alphas=-20:4:9x") == 1);
  CHECK(run("--expect-file=e --expect-alphas=2:1:9") == 1 && run("--conditional-file=c --conditional-alphas=1:1:2") == 1);

  /* the strictly parsed options at the ends of their ranges */
  CHECK(run("--tail-df=2") == 0 && o.tail_df == 2);
  CHECK(run("--tail-df=1000000") == 0 && o.tail_df == 1000000);
  CHECK(run("--tail-df=3") == 1 && run("--tail-df=1000002") == 1 && run("--tail-df=0") == 1 && run("--tail-df=4x") == 1);
  CHECK(run("--familywise-file=w --familywise-trials=1") == 0 && o.fw_trials == 1);
  CHECK(run("--familywise-file=w --familywise-trials=100000000") == 0 && o.fw_trials == 100000000);
  CHECK(run("--familywise-file=w --familywise-trials=0") == 1 && run("--familywise-file=w --familywise-trials=100000001") == 1);
  CHECK(run("--familywise-trials=5") == 1);
  CHECK(run("--conditional-file=c --conditional-rounds=1") == 0 && o.cond_rounds == 1);
  CHECK(run("--conditional-file=c --conditional-rounds=8") == 0 && o.cond_rounds == 8);
  CHECK(run("--conditional-file=c --conditional-rounds=0") == 1 && run("--conditional-file=c --conditional-rounds=9") == 1);
  CHECK(run("--expect-file=e --expect-bins=1") == 0 && o.expect_bins == 1);
  CHECK(run("--expect-file=e --expect-bins=64") == 0 && o.expect_bins == 64);
  CHECK(run("--expect-file=e --expect-bins=0") == 1 && run("--expect-file=e --expect-bins=65") == 1);
  CHECK(run("--expect-file=e --expect-top=0") == 0 && o.expect_top == 0);
  CHECK(run("--expect-file=e --expect-top=-1") == 1 && run("--expect-file=e --expect-top=2.5") == 1);
  CHECK(run("--conditional-file=c --conditional-halfwidth=0 --conditional-step=1 --conditional-min-clr=-2.5e1") == 0);
  CHECK(o.cond_halfwidth == 0 && o.cond_step == 1 && o.cond_min_clr == -25.0);
  CHECK(run("--conditional-file=c --conditional-halfwidth=2147483647") == 0 && o.cond_halfwidth == 2147483647);
  CHECK(run("--conditional-file=c --conditional-halfwidth=2147483648") == 1 && run("--conditional-file=c --conditional-halfwidth=-1") == 1);
  CHECK(run("--conditional-file=c --conditional-step=0") == 1 && run("--conditional-file=c --conditional-step=7x") == 1);
  CHECK(run("--conditional-file=c --conditional-min-clr=nan") == 1 && run("--conditional-file=c --conditional-min-clr=1x") == 1);
  /* the lenient ones stay atoi / atof */
  CHECK(run("--sites-top=abc") == 0 && o.sites_top == 0);
  CHECK(run("--sites-top=7x --alpha-drop=1.5x --bootstrap-reps=") == 0 && o.sites_top == 7 && o.alpha_drop == 1.5 && o.bootstrap_reps == 0);
  CHECK(run("--sites-top=-1") == 1);

  cli_opts_free(&o);
  printf("ok\n");
  return 0;
}
