"""The rows a slot holds, restated: what the four row entry points of include/fsclg.h must leave on the
device, and the crafted cases that pin their kernels (scatter_rows_kernel, plan_swap_kernel,
plan_rot_save_kernel / plan_rot_kernel).  NumPy only; tests/test_rows_ref.py checks, without a GPU, that
every case is in the regime it is named for, tests/test_slot_rows_gpu.py runs them on the device.

Read-back.  No call returns a slot's rows, so they are read through sites_kernel on tables in which a
site's term is exactly its row: coef[row][iv] = (0, 0, 0, 0) in every interval (the interval chosen
cannot matter) and nullrow[row] = -(row + 1), so a term is 0 - nullrow = row + 1, exact in a double, and a
window's null sum is a negative integer, exact in any order of addition.  One request per chromosome with
the sweep on the chromosome's first site and lalpha = -20: the de-collision moves the sweep 1 bp to the
right, the first site stays the nearest (the next one is SPACING - 1 bp away), nothing lies to its left
and log(alpha d) never passes LOG_AD_MAX, so the walk's terms are the chromosome's rows in site order.

Plans.  apply_plan is the statement of include/fsclg.h, independent of the kernels and of
fh_plan_apply_u32: the groups in order; kind 0 exchanges rows[i + t] and rows[j + t] for t < len;
kind 1 is the reference's loop of element swaps (scan-chromosome.c:365-384) run in order on the
overlapping ranges, not the closed-form rotation.  plan_ok restates fsclg_slot_set_rows_plan's refusals
and adds the caller's contract (the entries of one group touch disjoint sites).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import walk_ref as wr

POS0, SPACING = 5000, 4  # the de-collided sweep is 1 bp from the first site, 3 bp from the second
LALPHA = -20.0           # LOG_AD_MIN: log(alpha d) <= LOG_AD_MAX up to d = e^24
N_IV_WIDE = 8            # intervals of the tables with more than 256 rows (walk_terms clamps as the device does)
READ_ER = 1 << 20        # above every chromosome here: one whole-chromosome window each

SWAP_MAX = 4096          # sites of a kind-0 entry (one workgroup)
SWAP_ROUND, SWAP_PER = 256, 3   # plan_swap_kernel: threads, sites of each range per thread per round
ROT_GRID = 1024 * 256    # plan_rot_*_kernel: the grid covers this many sites before a thread strides

# table rows per staging width in bytes: the most the width holds, and for 4 bytes values past 0xFFFF
WIDTH_ROWS = {1: 256, 2: 65536, 4: 70000}
WIDTH_DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}
SCATTER_N = [1, 63, 64, 1024, 1025, 3589, 3597]  # (3597: a whole 16-byte read and a rest in the 2-byte width too)


# ------------------------------------------------------------------ read-back
def positions(n: int) -> np.ndarray:
    return (POS0 + SPACING * np.arange(n, dtype=np.int64)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _identity(n_rows: int):
    n_iv = wr.N_IV if n_rows <= 256 else N_IV_WIDE
    return np.zeros((n_rows, n_iv, 4)), -(np.arange(n_rows, dtype=np.float64) + 1.0), wr.log_table()


def tables(n_rows: int, rows) -> wr.Tables:
    """Tables in which the term of a site is exactly rows[site] + 1 (the big arrays are shared)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    assert len(rows) and int(rows.max()) < n_rows
    coef, nul, lt = _identity(n_rows)
    return wr.Tables(positions(len(rows)), rows, coef, nul, lt)


def requests(chr_start) -> list:
    """One request per chromosome: the sweep on its first site."""
    return [(c, POS0 + SPACING * int(a), LALPHA) for c, a in enumerate(chr_start)]


def even_chromosomes(n: int, per: int):
    """(chr_start, chr_n): chromosomes of `per` sites, the last one shorter."""
    start = list(range(0, n, per))
    return start, [min(per, n - a) for a in start]


def rows_of_terms(near, nl, nr, ws, we, terms) -> np.ndarray:
    """The rows of sites ws .. we from one whole-window walk's terms (walk order: the nearest SNP, then
    leftwards, then rightwards); raises if the walk is not the whole window or a term is no row + 1."""
    if not (ws <= near <= we and nl == near - ws and nr == we - near and len(terms) == we - ws + 1):
        raise ValueError(f"walk ({near}, -{nl}, +{nr}) of {len(terms)} terms is not the window [{ws}, {we}]")
    t = np.asarray(terms, dtype=np.float64)
    site = np.concatenate([[near], np.arange(near - 1, near - 1 - nl, -1), np.arange(near + 1, near + 1 + nr)]) - ws
    out = np.zeros(len(t), dtype=np.float64)
    out[site.astype(np.int64)] = t
    if not (np.isfinite(out).all() and (out == np.floor(out)).all() and (out >= 1).all() and (out <= 2.0 ** 32).all()):
        bad = int(np.flatnonzero(~(np.isfinite(out) & (out == np.floor(out)) & (out >= 1) & (out <= 2.0 ** 32)))[0])
        raise ValueError(f"site {ws + bad}: term {out[bad]!r} is no row + 1")
    return (out - 1.0).astype(np.uint32)


def window_null(rows, ws: int, we: int) -> float:
    """The null sum of the window [ws, we] on the identity tables: -(sum of row + 1), an exact integer."""
    return -float(int(np.asarray(rows[ws:we + 1], dtype=np.int64).sum()) + (we - ws + 1))


# ------------------------------------------------------------------ plans
def apply_plan(rows, ent, grp) -> np.ndarray:
    """The rows after the plan: ent [(i, j, len, kind)], grp the n_grp + 1 offsets into ent."""
    r = np.array(rows, dtype=np.uint32, copy=True)
    for q in range(len(grp) - 1):
        for i, j, ln, kind in ent[grp[q]:grp[q + 1]]:
            if kind == 0:  # disjoint ranges: the element swaps in any order
                a, b = r[i:i + ln].copy(), r[j:j + ln].copy()
                r[i:i + ln], r[j:j + ln] = b, a
            else:          # overlapping ranges: one element swap after another, in order
                lo, hi = min(i, j), max(i, j) + ln
                v = r[lo:hi].tolist()
                for t in range(ln):
                    v[i - lo + t], v[j - lo + t] = v[j - lo + t], v[i - lo + t]
                r[lo:hi] = v
    return r


def plan_refusal(ent, grp, n: int, n_grp=None):
    """None for a plan fsclg_slot_set_rows_plan takes and whose groups keep the caller's contract; else
    the rule it breaks.  ent / grp may be None (a NULL pointer); n_grp defaults to len(grp) - 1."""
    if n_grp is None:
        n_grp = len(grp) - 1 if grp is not None else 0
    if n_grp < 0:
        return "negative group count"
    if n_grp == 0:
        return None
    if ent is None or grp is None:
        return "NULL entries or groups"
    if grp[0] != 0:
        return "grp[0] != 0"
    for q in range(n_grp):
        if grp[q + 1] <= grp[q]:
            return f"group {q} is empty"
        seen = []
        for i, j, ln, kind in ent[grp[q]:grp[q + 1]]:
            d = abs(i - j)
            if i < 0 or j < 0 or ln < 0:
                return "negative i, j or len"
            if i + ln > n or j + ln > n:
                return "range past the sites"
            if kind == 0:
                if d < ln:
                    return "kind 0 with overlapping ranges"
                if ln > SWAP_MAX:
                    return "kind 0 above 4096 sites"
                mine = [(i, i + ln), (j, j + ln)]
            elif kind == 1:
                if d >= ln:
                    return "kind 1 with disjoint ranges"
                if grp[q + 1] - grp[q] != 1:
                    return "kind 1 sharing a group"
                mine = [(min(i, j), max(i, j) + ln)]
            else:
                return f"kind {kind}"
            for a, b in mine:
                if any(a < y and x < b for x, y in seen):
                    return f"group {q}: entries touch the same sites (the caller's contract)"
            seen += [(a, b) for a, b in mine if a < b]
    return None


def plan_ok(ent, grp, n: int, n_grp=None) -> bool:
    return plan_refusal(ent, grp, n, n_grp) is None


def one_group_each(ents) -> tuple:
    """Every entry a group of its own."""
    return list(ents), list(range(len(ents) + 1))


PLAN_N = 12000
SWAP_LEN = [1, 255, 256, 257, 767, 768, 769, 1536, 1537, 4095, 4096]
ROT_LEN = [2, 3, 300, 5000]
BIG_N, BIG_PER, BIG_LEN, BIG_D = 300_000, 100_000, 200_000, 70_000


def rot_ds(ln: int) -> list:
    return sorted({d for d in (1, 2, ln // 2, ln - 1) if 1 <= d < ln})


@functools.lru_cache(maxsize=None)
def swap_plans() -> dict:
    """name -> (ent, grp) on PLAN_N sites, kind 0 only."""
    out = {}
    for k, ln in enumerate(SWAP_LEN):  # odd starts, across the 128-site interleave blocks, either order of i and j
        i, j = 301, 301 + ln + 1001 + (k & 1)
        out[f"len-{ln}"] = one_group_each([(i, j, ln, 0) if k % 3 else (j, i, ln, 0)])
    out["adjacent"] = one_group_each([(1001, 1001 + 769, 769, 0)])
    out["adjacent-1"] = one_group_each([(127, 128, 1, 0)])
    # several entries per group (the second group's entries begin at ent + 3), and later groups that move sites
    # the earlier ones moved
    ent = [(1, 5001, 700, 0), (801, 6001, 257, 0), (9001, 1201, 1000, 0),
           (3, 2503, 900, 0), (5003, 7003, 1537, 0), (1001, 9301, 300, 0), (11000, 10000, 999, 0),
           (0, 6000, 4096, 0), (4097, 10193, 1807, 0)]
    out["groups"] = (ent, [0, 3, 7, 9])
    out["order"] = ([(100, 2100, 1000, 0), (600, 5600, 1000, 0), (2000, 5000, 1500, 0)], [0, 1, 2, 3])
    return out


def random_plan(rng, n: int, rotations: bool = True) -> tuple:
    """A random plan plan_ok accepts: 1 .. 6 groups, each one rotation or up to 6 disjoint swaps."""
    ent, grp = [], [0]
    for _ in range(int(rng.integers(1, 7))):
        if rotations and rng.random() < 0.3:
            ln = int(rng.choice([2, 3, 17, 300, 1000, 3000]))
            d = int(rng.integers(0, ln))
            lo = int(rng.integers(0, n - ln - d + 1))
            ent.append((lo, lo + d, ln, 1) if rng.random() < 0.5 else (lo + d, lo, ln, 1))
        else:
            used = []
            for _ in range(int(rng.integers(1, 7))):
                for _try in range(50):
                    ln = int(rng.choice([1, 2, 63, 255, 256, 257, 768, 769, 1000, 2048, 4096])) if rng.random() < 0.5 \
                        else int(rng.integers(0, SWAP_MAX + 1))
                    i, j = int(rng.integers(0, n - ln + 1)), int(rng.integers(0, n - ln + 1))
                    mine = [(i, i + ln), (j, j + ln)]
                    if abs(i - j) >= ln and not any(a < y and x < b for a, b in mine for x, y in used):
                        used += mine
                        ent.append((i, j, ln, 0))
                        break
            if len(ent) == grp[-1]:  # (no room found: never in practice)
                ent.append((0, n - 1, 1, 0))
        grp.append(len(ent))
    return ent, grp


@functools.lru_cache(maxsize=None)
def random_plans() -> list:
    return [random_plan(np.random.default_rng(4100 + s), PLAN_N) for s in range(20)]


@functools.lru_cache(maxsize=None)
def rot_plans() -> dict:
    """name -> (ent, grp) on PLAN_N sites with kind-1 entries."""
    out = {}
    for ln in ROT_LEN:
        for d in rot_ds(ln):
            lo = 1001 if ln > 3 else 127  # (the short ones across an interleave block's end)
            out[f"len-{ln}-d-{d}-up"] = one_group_each([(lo, lo + d, ln, 1)])
            out[f"len-{ln}-d-{d}-down"] = one_group_each([(lo + d, lo, ln, 1)])
    out["d-0"] = one_group_each([(777, 777, 300, 1)])
    out["between-swaps"] = one_group_each([(500, 3000, 1500, 0), (1200, 1900, 2500, 1), (900, 3500, 2000, 0)])
    return out


def big_plan() -> tuple:
    """The grid-stride loops of the rotation kernels: R = len + d above ROT_GRID."""
    return one_group_each([(1000, 1000 + BIG_D, BIG_LEN, 1)])


@dataclass
class Refusal:
    name: str
    ent: object
    grp: object
    n_grp: int


def plan_refusals(n: int = PLAN_N) -> list:
    """The plans fsclg_slot_set_rows_plan must refuse on n sites (FSCLG_E_ARG before any device work)."""
    ok = (10, 5000, 100, 0)
    R = Refusal
    return [
        R("grp[0] != 0", [ok, ok], [1, 2], 1),
        R("an empty group", [ok], [0, 0, 1], 2),
        R("negative i", [(-1, 5000, 100, 0)], [0, 1], 1),
        R("negative j", [(10, -5, 100, 0)], [0, 1], 1),
        R("negative len", [(10, 5000, -1, 0)], [0, 1], 1),
        R("i + len > n", [(n - 99, 10, 100, 0)], [0, 1], 1),
        R("j + len > n", [(10, n - 99, 100, 0)], [0, 1], 1),
        R("j + len > n, kind 1", [(n - 150, n - 99, 100, 1)], [0, 1], 1),
        R("kind 0 with d < len", [(10, 109, 100, 0)], [0, 1], 1),
        R("kind 0 with len 4097", [(0, 5000, SWAP_MAX + 1, 0)], [0, 1], 1),
        R("kind 2", [(10, 5000, 100, 2)], [0, 1], 1),
        R("kind -1", [(10, 5000, 100, -1)], [0, 1], 1),
        R("kind 1 with d = len", [(10, 110, 100, 1)], [0, 1], 1),
        R("kind 1 with d > len", [(10, 5000, 100, 1)], [0, 1], 1),
        R("kind 1 sharing a group", [(10, 60, 100, 1), (5000, 6000, 100, 0)], [0, 2], 1),
        R("kind 1 sharing a group, second", [(5000, 6000, 100, 0), (10, 60, 100, 1)], [0, 2], 1),
        R("NULL ent", None, [0, 1], 1),
        R("NULL grp", [ok], None, 1),
        R("negative n_grp", [ok], [0, 1], -1),
    ]


# ------------------------------------------------------------------ rows of the cases
def base_rows(n: int, n_rows: int, seed: int = 1) -> np.ndarray:
    """The uploaded rows: every site another row while the table has that many."""
    rng = np.random.default_rng(seed)
    if n <= n_rows:
        return rng.permutation(n_rows)[:n].astype(np.uint32)
    return rng.integers(0, n_rows, n).astype(np.uint32)


def scatter_rows(width: int, n: int, seed: int = 0) -> np.ndarray:
    """n random rows of a `width`-byte staging that reach the width's highest table row (and row 0)."""
    n_rows = WIDTH_ROWS[width]
    rng = np.random.default_rng(1000 * width + n + seed)
    lo = 0x10000 if width == 4 else 0  # every 4-byte value above 0xFFFF but the planted 0
    r = rng.integers(lo, n_rows, n).astype(np.uint32)
    r[int(rng.integers(0, n))] = 0
    r[-1] = n_rows - 1  # the last site: the scalar tail's last element
    if n > 1:
        r[0] = n_rows - 1 - (1 if width == 4 else 0)
    return r
