/* trial_rule_check.c -- a stand-alone exercise of the permutation test's trial rule
 * (fh_trial_apply, fscl_amd/csrc/host/perm.c), meant to be built with the sanitizers:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
 *       tools/trial_rule_check.c fscl_amd/csrc/host/perm.c fscl_amd/csrc/host/util.c -lm \
 *       -o /tmp/trial_rule_check && /tmp/trial_rule_check
 *
 * It needs no GPU and no device library.  The crafted sequences are those of
 * tests/test_trial_rule_host.py; each point's record is a heap block of exactly `save` floats, so a
 * write at or past the cap is an ASan error.  Exit status 0 and "ok" when every check holds. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fscl_amd/csrc/host/fscl_host.h"

char *prepend_label, *output_fname;
int spline_pts, n_permute;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

typedef struct { const int *v; int n, asked; } script_t;

static int draw(void *ctx) {
  script_t *s = ctx;
  CHECK(s->asked < s->n);
  return s->v[s->asked++];
}

static scan_pt_t point(double clr, int p, int n, int save) {
  scan_pt_t q;
  memset(&q, 0, sizeof q);
  q.chr = 3; q.clr = clr; q.permute_p = p; q.permute_n = n;
  q.permute_clr = malloc(sizeof(float) * (size_t)(save ? save : 1));
  return q;
}

/* one result applied; the counts and the flag afterwards, and the draws asked so far */
static void step(scan_pt_t *q, script_t *s, int save, double clr, int p, int n, int fin, int asked) {
  const int n0 = q->permute_n;
  fh_trial_apply(q, clr, -1.5, 12345, save, draw, s);
  CHECK(q->permute_p == p && q->permute_n == n && q->permute_finished == fin && s->asked == asked);
  if (n0 < save) CHECK(isnan(clr) ? isnan(q->permute_clr[n0]) : q->permute_clr[n0] == (float)clr);
}

int main(void) {
  static const int top[1] = {2147483647}, zero[1] = {0}, half[1] = {1 << 30}, over[1] = {(1 << 30) + 1};
  scan_pt_t q;
  script_t s;
  int i;

  /* 19 hits ask for nothing; the 20th asks for one draw */
  q = point(5.0, 0, 0, 100);
  s = (script_t){top, 1, 0};
  for (i = 1; i <= 19; i++) step(&q, &s, 100, 6.0, i, i, 0, 0);
  step(&q, &s, 100, 6.0, 20, 20, 1, 1);
  free(q.permute_clr);

  /* Q7: 19 -> 20 at n = 39 compares 20/39, not 20/40 */
  {
    static const double frac[3] = {0.49, 0.505, 0.52};
    static const int want[3] = {1, 1, 0};
    for (i = 0; i < 3; i++) {
      const int r[1] = {(int)(frac[i] * (2147483647 + 1.0))};
      q = point(5.0, 19, 39, 100);
      s = (script_t){r, 1, 0};
      step(&q, &s, 100, 5.5, 20, 40, want[i], 1);
      free(q.permute_clr);
    }
  }

  /* a ratio equal to the draw prunes; the extreme draws */
  q = point(5.0, 19, 40, 100); s = (script_t){half, 1, 0};
  step(&q, &s, 100, 5.0, 20, 41, 1, 1);
  free(q.permute_clr);
  q = point(5.0, 19, 40, 100); s = (script_t){over, 1, 0};
  step(&q, &s, 100, 5.0, 20, 41, 0, 1);
  free(q.permute_clr);
  q = point(1.0, 30, 1000000, 10); s = (script_t){zero, 1, 0};
  step(&q, &s, 10, 2.0, 31, 1000001, 1, 1);
  free(q.permute_clr);
  q = point(1.0, 19, 20, 100); s = (script_t){top, 1, 0};
  step(&q, &s, 100, 2.0, 20, 21, 1, 1);
  free(q.permute_clr);
  q = point(1.0, 19, 21, 100); s = (script_t){top, 1, 0};
  step(&q, &s, 100, 2.0, 20, 22, 0, 1);
  free(q.permute_clr);

  /* an equal clr is a hit; a miss asks for nothing even at permute_p >= 20; NaN is a miss, saved and counted */
  q = point(7.25, 3, 10, 100); s = (script_t){NULL, 0, 0};
  step(&q, &s, 100, 7.25, 4, 11, 0, 0);
  step(&q, &s, 100, nextafter(7.25, 0.0), 4, 12, 0, 0);
  free(q.permute_clr);
  q = point(7.25, 25, 100, 200); s = (script_t){NULL, 0, 0};
  step(&q, &s, 200, 7.0, 25, 101, 0, 0);
  step(&q, &s, 200, NAN, 25, 102, 0, 0);   /* also the out-of-range line on stderr */
  step(&q, &s, 200, -1.0, 25, 103, 0, 0);
  free(q.permute_clr);

  /* the save cap: the record holds exactly `save` floats */
  q = point(50.0, 0, 6, 8); s = (script_t){NULL, 0, 0};
  for (i = 0; i < 4; i++) step(&q, &s, 8, 1.0 + i, 0, 7 + i, 0, 0);
  step(&q, &s, 8, 60.0, 1, 11, 0, 0);
  CHECK(q.permute_clr[6] == 1.0f && q.permute_clr[7] == 2.0f);
  free(q.permute_clr);
  q = point(50.0, 0, 0, 0); s = (script_t){NULL, 0, 0};
  step(&q, &s, 0, 1.0, 0, 1, 0, 0);
  free(q.permute_clr);

  printf("ok\n");
  return 0;
}
