"""A NumPy float64 restatement of the projected-tail fit (include/fsclg.h, fsclg_tail_submit), for
tests/test_tail_host.py and tests/test_tail_gpu.py: the density series, the score, 60-step score
bisection in a bracket doubled until the score is not positive, the log-domain tail and the flags.

Model: the positive samples of a point are noncentral chi-square with k = 2 h degrees of freedom and
noncentrality lam; with a = lam / 2, b = x / 2 the density is the Poisson mixture
    f(x) = sum_j e^-a a^j / j! * b^(h+j-1) e^-b / (2 (h+j-1)!)
whose terms t_j = a^j b^(h+j-1) / (j! (h+j-1)!) have the ratio a b / ((j+1) (j+h)); they are summed
outward from the largest one, scaled by it.  The upper tail at x0 (b0 = x0 / 2) is
    Q = e^(-a - b0) sum_j a^j / j! sum_{i < h + j} b0^i / i!
summed in the log domain.

E_L and E_Q are this restatement's own greatest errors against mpmath at 50 digits on the small
fixtures (tests/test_tail_host.py measures them again and holds them to these constants); the GPU
tests allow 64 times as much, and never less than m * 2^-52.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

FIT, CENTRAL, NOFIT = 0, 1, 2
FLAG_NAMES = ("fit", "central", "nofit")
BISECT, DOUBLINGS = 60, 64
LOG2 = 0.6931471805599453
LOG10E = 0.4342944819032518

# Measured by tests/test_tail_host.py::test_reference_against_mpmath (mpmath 1.3.0, mp.dps = 50) over
# every small fixture below, at the fixture's own lambda-hat and at its true lambda:
# E_L: the greatest |l_ref - l_mp| / sum_i |log f_i|            (measured 2.463e-14, at l400_k2)
# E_Q: the greatest |log10 Q_ref - log10 Q_mp| / max(1, |log10 Q_mp|)   (measured 3.703e-14, at l400_k2)
E_L = 2.5e-14
E_Q = 3.8e-14

_lg = np.frompyfunc(math.lgamma, 1, 1)


def lgam(x) -> np.ndarray:
    return _lg(np.asarray(x, dtype=np.float64)).astype(np.float64)


def positive(x) -> np.ndarray:
    """The samples that enter the fit: x > 0 and finite (zero, negative, NaN, inf count in m alone)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (x > 0) & np.isfinite(x)


def jstar(a, b, h):
    return np.maximum(np.floor(0.5 * (np.sqrt((h - 1.0) ** 2 + 4.0 * a * b) - (h - 1.0))), 0.0)


def series(a: float, b: np.ndarray, h: int):
    """(j*, S0, S1) per sample: S0 = sum_j t_j / t_j*, S1 = sum_j t_j b / (h + j) / t_j* (the series of k + 2
    degrees of freedom on the same scale)."""
    b = np.asarray(b, dtype=np.float64)
    P = a * b
    js = jstar(a, b, h)
    W = int(8.0 * math.sqrt(float(js.max(initial=0.0)) + 1.0) + 48)
    i = np.arange(W, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        ju = js[:, None] + i                                   # the term before each upward step
        up = np.cumprod(P[:, None] / ((ju + 1.0) * (ju + h)), axis=1)
        jd = js[:, None] - i                                   # the term before each downward step
        dn = np.cumprod(np.where(jd > 0.0, jd * (jd + h - 1.0) / np.where(P > 0.0, P, 1.0)[:, None], 0.0), axis=1)
    assert (up[:, -1] <= 2.0 ** -64).all() and (dn[:, -1] <= 2.0 ** -64).all(), "series window too short"
    S0 = 1.0 + up.sum(axis=1) + dn.sum(axis=1)
    S1 = b * (1.0 / (h + js) + (up / (h + ju + 1.0)).sum(axis=1) + np.where(dn > 0.0, dn / np.where(dn > 0.0, h + jd - 1.0, 1.0), 0.0).sum(axis=1))
    return js, S0, S1


def logpdf(x, k: int, lam: float) -> np.ndarray:
    """log f(x; k, lam) of positive x."""
    h = k // 2
    a = 0.5 * float(lam)
    b = 0.5 * np.asarray(x, dtype=np.float64)
    js, S0, _ = series(a, b, h)
    la = math.log(a) if a > 0.0 else 0.0
    lt = np.where(js > 0.0, js * la, 0.0) + (h - 1.0 + js) * np.log(b) - lgam(js + 1.0) - lgam(h + js)
    return lt + np.log(S0) - a - b - LOG2


def score(x, k: int, lam: float) -> float:
    """d l / d lam = 1/2 sum (f_{k+2} / f_k - 1) over positive x."""
    h = k // 2
    b = 0.5 * np.asarray(x, dtype=np.float64)
    _, S0, S1 = series(0.5 * float(lam), b, h)
    return 0.5 * float(np.sum(S1 / S0 - 1.0))


def logl(x, k: int, lam: float) -> float:
    return float(np.sum(logpdf(x, k, lam)))


def abs_logl(x, k: int, lam: float) -> float:
    return float(np.sum(np.abs(logpdf(x, k, lam))))


def log10_q(x0: float, k: int, lam: float) -> float:
    """log10 of the upper tail at x0; 0 for x0 <= 0 or NaN."""
    if not x0 > 0.0:
        return 0.0
    h = k // 2
    a, b0 = 0.5 * float(lam), 0.5 * float(x0)
    la, lb = (math.log(a) if a > 0.0 else -math.inf), math.log(b0)
    N = h + int(2.0 * max(a, float(jstar(a, b0, h))) + 2.0) + 64
    while True:
        i = np.arange(N, dtype=np.float64)
        ld = np.where(i > 0.0, i * lb, 0.0) - lgam(i + 1.0)
        logC = np.logaddexp.accumulate(ld)                     # logC[i] = log sum_{i' <= i} d_i'
        j = np.arange(N - (h - 1), dtype=np.float64)
        with np.errstate(invalid="ignore"):
            lw = np.where(j > 0.0, j * la, 0.0) - lgam(j + 1.0) if a > 0.0 else np.where(j > 0.0, -np.inf, 0.0)
        lT = lw + logC[h - 1:]
        M = float(lT.max())
        if lT[-1] < M - 50.0:
            break
        N *= 2
    lq = M + math.log(float(np.sum(np.exp(lT - M)))) - a - b0
    return min(lq, 0.0) * LOG10E


@dataclass
class Fit:
    m: int
    m_pos: int
    mean: float
    variance: float
    lam: float
    logl: float
    log10_q: float
    flag: int
    lo: float = math.nan       # the final bracket of a FIT point: score(lo) >= 0 >= score(hi)
    hi: float = math.nan
    abs_logl: float = math.nan  # sum |log f_i| at lam


def fit(samples, x0: float, k: int = 2, min_n: int = 20) -> Fit:
    x32 = np.asarray(samples, dtype=np.float32)
    m = len(x32)
    x = x32[positive(x32)].astype(np.float64)
    m_pos = len(x)
    mean = float(x.sum() / m_pos) if m_pos else math.nan
    var = float(((x - mean) ** 2).sum() / (m_pos - 1)) if m_pos > 1 else math.nan
    if m_pos < max(min_n, 1):
        return Fit(m, m_pos, mean, var, math.nan, math.nan, math.nan, NOFIT)
    lam, flag, lo, hi = 0.0, CENTRAL, math.nan, math.nan
    if mean > k:
        flag, lo, hi = FIT, 0.0, max(1.0, 2.0 * (mean - k))
        for _ in range(DOUBLINGS):
            if not score(x, k, hi) > 0.0:
                break
            lo, hi = hi, 2.0 * hi
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            if not lo < mid < hi:
                break
            if score(x, k, mid) > 0.0:
                lo = mid
            else:
                hi = mid
        lam = 0.5 * (lo + hi)
    return Fit(m, m_pos, mean, var, lam, logl(x, k, lam), log10_q(x0, k, lam), flag, lo, hi, abs_logl(x, k, lam))


def log10_p_tail(f: Fit) -> float:
    return math.nan if f.flag == NOFIT or f.m <= 0 else math.log10(f.m_pos / f.m) + f.log10_q


def log10_p_empirical(permute_p: int, permute_n: int) -> float:
    """The -o column's p-value (scan_output)."""
    return math.log10(1.0 / permute_n if permute_p < 2 else (permute_p - 1.0) / (permute_n - 1.0))


def output_row(name: str, pos: int, clr: float, permute_p: int, permute_n: int, f: Fit, k: int, label=None) -> list:
    """The fields of one --tail-file row (include/fscl_amd.h)."""
    row = ([label] if label else []) + [name, str(pos), "%1.2f" % clr, str(permute_p), str(permute_n), str(f.m_pos)]
    if f.flag == NOFIT:
        row += ["NA", "NA"]
    else:
        vr = f.variance / (2.0 * (k + 2.0 * f.lam))
        row += ["%1.4f" % f.lam, "%1.3f" % vr if math.isfinite(vr) else "NA"]
    row.append("%1.3f" % -log10_p_empirical(permute_p, permute_n) if permute_n > 0 else "NA")
    row.append("NA" if f.flag == NOFIT else "%1.3f" % (0.0 - log10_p_tail(f)))
    row.append(FLAG_NAMES[f.flag])
    return row


# ------------------------------------------------------------------ the tolerances of the GPU tests
def tol_l(f: Fit) -> float:
    return max(64.0 * E_L, f.m * 2.0 ** -52) * f.abs_logl


def tol_q(f: Fit, lq: float) -> float:
    return max(64.0 * E_Q, f.m * 2.0 ** -52) * max(1.0, abs(lq))


# ------------------------------------------------------------------ the fixtures
@dataclass
class Case:
    name: str
    k: int
    min_n: int
    lam: float              # the lambda the samples were drawn with
    samples: np.ndarray     # float32
    x0: float
    regime: int             # the flag the fixture is named for
    small: bool = True      # part of the mpmath measurement
    ref: Fit = field(default=None, repr=False)


def draw(seed: int, m: int, k: int, lam: float, zeros: int = 0) -> np.ndarray:
    g = np.random.default_rng(seed)
    x = (g.noncentral_chisquare(k, lam, m) if lam > 0.0 else g.chisquare(k, m)).astype(np.float32)
    if zeros:
        x[g.choice(m, zeros, replace=False)] = 0.0
    return x


def central_draw(seed: int, m: int, k: int, zeros: int = 0) -> np.ndarray:
    """Central chi-square samples whose positive mean lies clearly below k: the first of seed, seed + 100, ..."""
    while True:
        x = draw(seed, m, k, 0.0, zeros)
        if float(x[x > 0].mean()) <= k - 0.05:
            return x
        seed += 100


def _specs():
    out = []
    for k in (2, 4):
        s = 1000 * k
        out += [
            (f"single_k{k}", k, 1, 30.0, draw(s + 1, 1, k, 30.0), 40.0, FIT),
            (f"single_nofit_k{k}", k, 20, 30.0, draw(s + 1, 1, k, 30.0), 40.0, NOFIT),
            (f"pruned_k{k}", k, 20, 0.5, draw(s + 2, 20, k, 0.5), 9.0, None),
            (f"pruned_short_k{k}", k, 20, 0.5, draw(s + 3, 20, k, 0.5, zeros=5), 9.0, NOFIT),
            (f"w63_k{k}", k, 20, 30.0, draw(s + 4, 63, k, 30.0, zeros=7), 90.0, FIT),
            (f"w64_k{k}", k, 20, 30.0, draw(s + 5, 64, k, 30.0), 0.0, FIT),
            (f"w65_k{k}", k, 20, 0.5, draw(s + 6, 65, k, 0.5, zeros=9), 25.0, None),
            (f"l400_k{k}", k, 20, 400.0, draw(s + 7, 129, k, 400.0, zeros=3), 520.0, FIT),
            (f"far_k{k}", k, 20, 400.0, draw(s + 8, 129, k, 400.0), 1500.0, FIT),
            (f"central_k{k}", k, 20, 0.0, central_draw(s + 9, 129, k, zeros=20), 18.0, CENTRAL),
            (f"zeros_k{k}", k, 20, 0.0, np.zeros(64, dtype=np.float32), 5.0, NOFIT),
            (f"nans_k{k}", k, 20, 0.0, np.full(65, np.nan, dtype=np.float32), 5.0, NOFIT),
            (f"mixed_k{k}", k, 20, 30.0, np.concatenate([draw(s + 10, 60, k, 30.0), np.array(
                [np.nan, -1.0, 0.0, np.inf, -np.inf], dtype=np.float32)]), 70.0, FIT),
        ]
        below = draw(s + 11, 129, k, 30.0)
        out.append((f"below_k{k}", k, 20, 30.0, below, 0.5 * float(below.min()), FIT))
    out.append(("full_k2", 2, 20, 30.0, draw(77, 10000, 2, 30.0, zeros=1500), 120.0, FIT))
    return out


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    """Every single-point fixture with its reference fit, computed once per process."""
    res = []
    for name, k, min_n, lam, x, x0, regime in _specs():
        f = fit(x, x0, k, min_n)
        res.append(Case(name, k, min_n, lam, x, x0, f.flag if regime is None else regime, name != "full_k2", f))
    return tuple(res)


BATCH_N, BATCH_SEED = 300, 4242


@functools.lru_cache(maxsize=None)
def batch():
    """300 points of 0 .. 200 samples in one launch (k = 2, min_n = 20): (samples, offsets[301], x0, [Fit])."""
    g = np.random.default_rng(BATCH_SEED)
    ms = g.integers(0, 201, BATCH_N)
    ms[:4] = (0, 200, 19, 20)
    lams = g.choice([0.0, 0.5, 30.0, 400.0], BATCH_N)
    xs, x0 = [], np.empty(BATCH_N)
    for p in range(BATCH_N):
        x = draw(BATCH_SEED + 1 + p, int(ms[p]), 2, float(lams[p]), zeros=int(ms[p]) // 5)
        xs.append(x)
        x0[p] = float(g.choice([0.0, 3.0, 60.0, 1500.0]))
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.uint64)
    fits = [fit(xs[p], float(x0[p]), 2, 20) for p in range(BATCH_N)]
    return np.concatenate(xs).astype(np.float32), off, x0, fits
