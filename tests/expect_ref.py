"""A NumPy restatement of the expected terms under the model (include/fsclg.h, fsclg_expect_submit),
for tests/test_expect_host.py and tests/test_expect_gpu.py.

Per site of a walk, at x = logt(|d|) + log alpha: p_f = exp(spline_f(x)) and q_f = fsp[f] over the
derived counts f = 1 .. n-1 (a value that is not finite or not positive counts as 0), the observed
class c = f, or min(f, n - f) on a folded site, its term t_f = spline_c(x) - null_logl(depth, c) (the
folded row and the folded null value on a folded site), the usable classes (p_f > 0, q_f > 0, t_f
finite), and over them the renormalised first two moments of t under p and under q, and the lost mass.
NumPy sums the classes pairwise; the device sums them lane by lane and through a butterfly, and its exp
differs from NumPy's by a few ulp.

E_M1 and E_M2 are this restatement's own greatest errors against mpmath at 50 digits, per site,
relative to sum pi |t| (first moments) and to sum pi t^2 (second moments), measured by
tests/test_expect_host.py::test_reference_against_mpmath over every 25th site of the inputs below at
the sweeps' own alphas.  The GPU tests allow 64 times as much, the margin tail_kernel got: the device's
exp and its fixed class order are a few ulp each from NumPy's.

Totals.  A total of first moments is allowed 64 E_M1 times the sum of its sites' scales sum pi |t|.  A total of
variances sums var = m2 - m1^2 per site: an error d2 in m2 and d1 in m1 moves it by d2 + 2 |m1| d1 to first order, so
its scale per site is sum pi t^2 + 2 |m1| sum pi |t|, and the bound is 64 max(E_M1, E_M2) times the sum of those (the
larger constant, since both errors enter).  Either total also gets n eps times its scale for the sequential fold of n
sites, whose rounding neither constant covers.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

import sample_ref as sr
import walk_ref as wr
from sample_ref import case, model_of, site_log_ad  # noqa: F401  (the inputs of the tests)

LOG_AD_MIN, LOG_AD_MAX = sr.LOG_AD_MIN, sr.LOG_AD_MAX
# measured (mpmath 1.3.0, mp.dps = 50, every 25th site): the greatest values were 5.93e-10 and 3.19e-10, both
# on `mixed`, at sites far from the sweep where every t_f = y_f - null_f is a difference of two values near -3
# that nearly cancel (|t| about 1e-5): the double rounding of y_f is then 1e-11 of |t|, whatever sums them
E_M1 = 6.0e-10
E_M2 = 3.2e-10
GPU_FACTOR = 64.0
EXP_LO, EXP_HI = -708.3964185322641, 709.782712893384   # exp's underflow (to 0) and overflow thresholds


@dataclass
class ExpectModel:
    M: sr.Model
    fcoef: list       # per depth float64 [n/2][n_iv][4]: the folded rows c = 1 .. n/2
    null_u: list      # per depth float64 [n-1]: log(fsp[f])
    null_f: list      # per depth float64 [n/2]: log(fsp[c] + fsp[n-c]), or log(fsp[c]) at c = n - c
    q: list           # per depth float64 [n-1]: the tables' fsp[1 .. n-1] (the neutral spectrum)


@functools.lru_cache(maxsize=None)
def expect_model(name: str) -> ExpectModel:
    c = case(name)
    M = c.model
    s = c.scan.contents
    fcoef, null_u, null_f = [], [], []
    with np.errstate(divide="ignore"):
        for d, n in enumerate(M.depth_n):
            t = c.tables[d]
            n_iv = M.coef[d].shape[1]
            rows = []
            for cc in range(1, n // 2 + 1):
                sp = t.fspline_func[cc].contents
                assert sp.n == n_iv
                rows.append(np.ctypeslib.as_array(sp.coef[0], shape=(sp.n * 4,)).reshape(sp.n, 4).copy())
            fcoef.append(np.array(rows, dtype=np.float64).reshape(n // 2, n_iv, 4))
            bg = np.array([c.fsp[d][f] for f in range(n + 1)], dtype=np.float64)   # the spectrum of the null model
            null_u.append(np.log(bg[1:n]))
            null_f.append(np.array([np.log(bg[k] + bg[n - k]) if k != n - k else np.log(bg[k])
                                    for k in range(1, n // 2 + 1)], dtype=np.float64))
    assert s.n_depths == len(M.depth_n)
    return ExpectModel(M, fcoef, null_u, null_f, M.fsp)


def _clean(v):
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(v) & (v > 0.0), v, 0.0)


SITE_FIELDS = ("x", "m1_s", "m2_s", "m1_0", "m2_0", "lost_s", "lost_0", "scale1_s", "scale2_s", "scale1_0", "scale2_0",
               "logSQ", "y_margin")


def site_moments(E: ExpectModel, sites: np.ndarray, x: np.ndarray) -> dict:
    """The per-site quantities of the definitions for the sites ``sites`` (global indices) at log_ad ``x``.
    degenerate: bool; scale*: sum pi |t| and sum pi t^2 under either spectrum (the tolerances' scales);
    logSQ: log(S / Q) over all classes; y_margin: the least distance of a class's spline value (the
    unfolded p's and, on folded sites, nothing else takes an exp) from exp's underflow or overflow threshold."""
    M = E.M
    sites = np.asarray(sites, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    k = len(sites)
    out = {f: np.zeros(k) for f in SITE_FIELDS}
    out["x"] = x.copy()
    out["degenerate"] = np.ones(k, dtype=bool)
    out["y_margin"] = np.full(k, np.inf)
    for d, n in enumerate(M.depth_n):
        m = n - 1
        sel = np.flatnonzero(M.depth_p[sites] == d)
        if not len(sel) or m < 1:
            continue
        xs = x[sel]
        n_iv = M.coef[d].shape[1]
        fold = M.folded[sites[sel]] != 0
        with np.errstate(all="ignore"):
            iv = np.clip(np.trunc((xs - LOG_AD_MIN) / M.step), 0, n_iv - 1).astype(np.int64)
            c = M.coef[d][:, iv, :]
            y = xs * (c[..., 0] * xs * xs + c[..., 1] * xs + c[..., 2]) + c[..., 3]          # [m][sites]
            p = _clean(np.exp(y))
            q = np.repeat(_clean(E.q[d])[:, None], len(sel), axis=1)
            t = y - E.null_u[d][:, None]
            f = np.arange(1, n)
            cc = np.minimum(f, n - f)
            cf = E.fcoef[d][cc - 1][:, iv, :]
            tf = xs * (cf[..., 0] * xs * xs + cf[..., 1] * xs + cf[..., 2]) + cf[..., 3] - E.null_f[d][cc - 1][:, None]
            t = np.where(fold[None, :], tf, t)
            use = (p > 0.0) & (q > 0.0) & np.isfinite(t)
            S, Q = p.sum(axis=0), q.sum(axis=0)
            pu, qu, tu = np.where(use, p, 0.0), np.where(use, q, 0.0), np.where(use, t, 0.0)
            Su, Qu = pu.sum(axis=0), qu.sum(axis=0)
            good = np.isfinite(S) & (S > 0) & np.isfinite(Q) & (Q > 0) & (Su > 0) & (Qu > 0)
            vals = {
                "m1_s": (pu * tu).sum(axis=0) / Su, "m2_s": (pu * tu * tu).sum(axis=0) / Su,
                "m1_0": (qu * tu).sum(axis=0) / Qu, "m2_0": (qu * tu * tu).sum(axis=0) / Qu,
                "lost_s": 1.0 - Su / S, "lost_0": 1.0 - Qu / Q,
                "scale1_s": (pu * np.abs(tu)).sum(axis=0) / Su, "scale2_s": (pu * tu * tu).sum(axis=0) / Su,
                "scale1_0": (qu * np.abs(tu)).sum(axis=0) / Qu, "scale2_0": (qu * tu * tu).sum(axis=0) / Qu,
                "logSQ": np.log(S / Q),
            }
            marg = np.where(np.isfinite(y), np.minimum(np.abs(y - EXP_LO), np.abs(y - EXP_HI)), np.inf).min(axis=0)
        for key, v in vals.items():
            out[key][sel] = np.where(good, v, 0.0)
        out["degenerate"][sel] = ~good
        out["y_margin"][sel] = marg
    return out


def site_moments_mp(E: ExpectModel, site: int, x: float, dps: int = 50) -> dict:
    """One site in mpmath: the same definitions with the double inputs (coefficients, null values, fsp,
    x) taken as exact; the usable set is NumPy's (the inputs keep every class clear of a flip)."""
    import mpmath as mp
    mp.mp.dps = dps
    M = E.M
    d = int(M.depth_p[site])
    n = M.depth_n[d]
    n_iv = M.coef[d].shape[1]
    iv = int(np.clip(np.trunc((x - LOG_AD_MIN) / M.step), 0, n_iv - 1))
    fold = bool(M.folded[site])
    X = mp.mpf(float(x))
    Su = Qu = a1 = a2 = b1 = b2 = s1 = s2 = z1 = z2 = mp.mpf(0)
    for f in range(1, n):
        c = [mp.mpf(float(v)) for v in M.coef[d][f - 1, iv]]
        y = X * (c[0] * X * X + c[1] * X + c[2]) + c[3]
        yd = float(y)
        p = mp.exp(y) if EXP_LO < yd < EXP_HI else mp.mpf(0)
        qd = float(E.q[d][f - 1])
        q = mp.mpf(qd) if np.isfinite(qd) and qd > 0 else mp.mpf(0)
        if fold:
            k = min(f, n - f)
            g = [mp.mpf(float(v)) for v in E.fcoef[d][k - 1, iv]]
            nul = float(E.null_f[d][k - 1])
            t = X * (g[0] * X * X + g[1] * X + g[2]) + g[3]
        else:
            nul = float(E.null_u[d][f - 1])
            t = y
        if not (p > 0 and q > 0 and np.isfinite(nul)):
            continue
        t = t - mp.mpf(nul)
        Su += p; Qu += q
        a1 += p * t; a2 += p * t * t; b1 += q * t; b2 += q * t * t
        s1 += p * abs(t); z1 += q * abs(t)
    return {"m1_s": a1 / Su, "m2_s": a2 / Su, "m1_0": b1 / Qu, "m2_0": b2 / Qu,
            "scale1_s": s1 / Su, "scale2_s": a2 / Su, "scale1_0": z1 / Qu, "scale2_0": b2 / Qu}


def bin_of(x: np.ndarray, n_bins: int) -> np.ndarray:
    with np.errstate(all="ignore"):
        b = np.trunc(((x - LOG_AD_MIN) * float(n_bins)) / (LOG_AD_MAX - LOG_AD_MIN)).astype(np.int64)
    return np.where(x >= LOG_AD_MIN, np.minimum(b, n_bins - 1), 0)


def walk_x(E: ExpectModel, sites: np.ndarray, sweep_pos: int, lalpha: float) -> np.ndarray:
    return wr.logt(np.abs(E.M.pos[np.asarray(sites, dtype=np.int64)] - int(sweep_pos)), E.M.log_table) + float(lalpha)


def totals(mom: dict, n_bins: int) -> dict:
    """Per bin b < n_bins and for all sites (entry n_bins): site count, degenerate count, the sums of m1, var
    under either spectrum (folded sequentially in site order), and the tolerances' scales: the sums of
    the sites' scale1 (for the E columns) and of scale2 + 2 |m1| scale1 (for the variance columns)."""
    b = bin_of(mom["x"], n_bins)
    ok = ~mom["degenerate"]
    res = {k: np.zeros(n_bins + 1) for k in ("e_s", "v_s", "e_0", "v_0", "se_s", "sv_s", "se_0", "sv_0")}
    res["n_sites"] = np.zeros(n_bins + 1, dtype=np.int64)
    res["n_degenerate"] = np.zeros(n_bins + 1, dtype=np.int64)
    for j in range(n_bins + 1):
        sel = np.ones(len(b), dtype=bool) if j == n_bins else b == j
        res["n_sites"][j] = int(sel.sum())
        res["n_degenerate"][j] = int((sel & ~ok).sum())
        u = sel & ok
        for tag in ("s", "0"):
            m1, m2 = mom[f"m1_{tag}"][u], mom[f"m2_{tag}"][u]
            e = v = 0.0
            for a, c in zip(m1, m2):
                e += a
                v += max(c - a * a, 0.0)
            res[f"e_{tag}"][j], res[f"v_{tag}"][j] = e, v
            res[f"se_{tag}"][j] = float(mom[f"scale1_{tag}"][u].sum())
            res[f"sv_{tag}"][j] = float((mom[f"scale2_{tag}"][u] + 2.0 * np.abs(m1) * mom[f"scale1_{tag}"][u]).sum())
    return res


def tol_m1() -> float:
    return GPU_FACTOR * E_M1


def tol_m2() -> float:
    return GPU_FACTOR * E_M2
