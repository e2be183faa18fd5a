"""The permutation test's trial rule (fh_trial_apply, perm.c), called through ctypes and compared
with a restatement of scan-chromosome.c:488-502 written here.  tools/trial_rule_check.c drives
the same crafted sequences under the sanitizers.  No GPU."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from util import run_host_check
import fscl_amd

RAND_MAX = 2147483647
DRAW_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
GUARD = np.float32(-12345.5)


class Ref:
    """scan-chromosome.c:488-502 for one point: the >= count, the permute_p >= 20 prune test with the
    pre-increment permute_n (Q7), the float save below the cap, permute_n++."""

    def __init__(self, clr, p, n, save):
        self.clr, self.p, self.n, self.finished, self.save = clr, p, n, 0, save
        self.saved = np.full(save + 1, GUARD, np.float32)
        self.draws = 0

    def apply(self, clr, script):
        if clr >= self.clr:  # False for NaN
            self.p += 1
            if self.p >= 20:
                r = script[self.draws]
                self.draws += 1
                if self.p / float(self.n) >= r / (RAND_MAX + 1.0):
                    self.finished = 1
        if self.n < self.save:
            self.saved[self.n] = np.float32(clr)
        self.n += 1


def run_case(L, clr0, p0, n0, save, results, script):
    """Apply `results` (clr values) one by one to the product's point and to Ref; compare after each."""
    buf = np.full(save + 1, GUARD, np.float32)  # one guard value after the record
    pt = fscl_amd.ScanPtT(chr=3, sweep_pos=777, clr=clr0, permute_n=n0, permute_p=p0)
    pt.permute_clr = buf.ctypes.data_as(C.POINTER(C.c_float))
    ref = Ref(clr0, p0, n0, save)
    asked = []

    @DRAW_FN
    def draw(ctx):
        asked.append(len(asked))
        return script[len(asked) - 1]

    for k, clr in enumerate(results):
        L.fh_trial_apply(C.byref(pt), float(clr), -1.5, 12345, save, draw, None)
        ref.apply(float(clr), script)
        got = (pt.permute_p, pt.permute_n, pt.permute_finished, len(asked))
        assert got == (ref.p, ref.n, ref.finished, ref.draws), (k, clr, got)
        assert buf.tobytes() == ref.saved.tobytes(), (k, clr)
    assert buf[save] == GUARD
    return pt, ref


@pytest.fixture(scope="module")
def L(built):
    lib = fscl_amd.get_lib()
    lib.fh_trial_apply.restype = None
    lib.fh_trial_apply.argtypes = [C.POINTER(fscl_amd.ScanPtT), C.c_double, C.c_double, C.c_int, C.c_int, DRAW_FN,
                                   C.c_void_p]
    return lib


def test_first_draw_at_the_twentieth_hit(L):
    # 19 hits from nothing ask for no draw; the 20th asks for exactly one (20/19 >= anything below 1: pruned)
    pt, ref = run_case(L, 5.0, 0, 0, 100, [6.0] * 19, [])
    assert (pt.permute_p, ref.draws) == (19, 0)
    pt, ref = run_case(L, 5.0, 0, 0, 100, [6.0] * 20, [RAND_MAX])
    assert (pt.permute_p, pt.permute_finished, ref.draws) == (20, 1, 1)


@pytest.mark.parametrize("frac, want", [(0.49, 1), (0.505, 1), (0.52, 0)])
def test_q7_ratio_uses_the_count_before_its_increment(L, frac, want):
    """p 19 -> 20 at n = 39: the rule compares 20/39 = 0.5128; the post-increment reading would compare
    20/40 = 0.5.  A draw between the two (0.505) prunes only under the pre-increment reading."""
    r = int(frac * (RAND_MAX + 1.0))
    pt, _ = run_case(L, 5.0, 19, 39, 100, [5.5], [r])
    assert pt.permute_finished == want
    post = 1 if 20 / 40.0 >= r / (RAND_MAX + 1.0) else 0
    assert (post != want) == (frac == 0.505)


def test_ratio_equal_to_the_draw_prunes(L):
    pt, _ = run_case(L, 5.0, 19, 40, 100, [5.0], [1 << 30])  # 20/40 >= 0.5
    assert pt.permute_finished == 1
    pt, _ = run_case(L, 5.0, 19, 40, 100, [5.0], [(1 << 30) + 1])
    assert pt.permute_finished == 0


def test_extreme_draws(L):
    pt, _ = run_case(L, 1.0, 30, 10 ** 6, 10, [2.0], [0])  # a draw of 0: any ratio >= 0
    assert pt.permute_finished == 1
    pt, _ = run_case(L, 1.0, 19, 20, 100, [2.0], [RAND_MAX])  # 20/20 >= (2^31 - 1) / 2^31
    assert pt.permute_finished == 1
    pt, _ = run_case(L, 1.0, 19, 21, 100, [2.0], [RAND_MAX])
    assert pt.permute_finished == 0


def test_equal_clr_is_a_hit_and_a_miss_draws_nothing(L):
    pt, _ = run_case(L, 7.25, 3, 10, 100, [7.25, np.nextafter(7.25, 0.0)], [])
    assert pt.permute_p == 4
    pt, ref = run_case(L, 7.25, 25, 100, 200, [7.0, 0.0, 7.24999], [])  # permute_p already >= 20: misses ask nothing
    assert (pt.permute_p, pt.permute_n, ref.draws) == (25, 103, 0)


def test_nan_is_no_hit_but_is_saved_and_counted(L, capfd):
    pt, ref = run_case(L, 0.0, 25, 40, 100, [float("nan")], [])
    assert (pt.permute_p, pt.permute_n, ref.draws) == (25, 41, 0) and math.isnan(pt.permute_clr[40])
    assert capfd.readouterr().err == "3\t12345\t%g\t%1.3e\n" % (float("nan"), math.exp(-1.5))
    run_case(L, 0.0, 0, 0, 100, [-1.0, 1000000.5, 1000000.0, 0.0], [])  # the out-of-range line: below 0, above 1e6
    assert capfd.readouterr().err == "".join("3\t12345\t%g\t%1.3e\n" % (v, math.exp(-1.5)) for v in (-1.0, 1000000.5))


def test_nothing_is_written_at_or_past_the_save_cap(L):
    pt, ref = run_case(L, 50.0, 0, 6, 8, [1.0, 2.0, 3.0, 4.0, 60.0], [])
    assert pt.permute_n == 11 and pt.permute_p == 1
    assert list(ref.saved[6:]) == [1.0, 2.0, GUARD]
    run_case(L, 50.0, 0, 8, 8, [1.0], [])  # already at the cap
    run_case(L, 50.0, 0, 0, 0, [1.0], [])  # a cap of 0


def test_a_mixed_sequence(L):
    rng = np.random.default_rng(7)
    res = rng.choice([0.5, 2.0, 3.0, 3.0000001, float("nan"), 9.0], size=400)
    script = [int(v) for v in rng.integers(0, RAND_MAX + 1, size=400)]
    script[:6] = [RAND_MAX] * 6  # the first draws do not prune: the rule keeps running past them
    run_case(L, 3.0, 0, 0, 64, res, script)


def test_host_check_under_sanitizers(built, tmp_path):
    """tools/trial_rule_check.c: the same crafted sequences under ASan and UBSan, as a stand-alone program
    built from perm.c and util.c alone (no device library, nothing loaded into Python)."""
    run_host_check("trial_rule_check", ["perm.c", "util.c"], tmp_path)
