"""A NumPy restatement of maxt_kernel's definitions (include/fsclg.h, fsclg_maxt_submit) and of the host combine
(include/fscl_amd.h, fscl_amd_familywise_combine / _threshold), for tests/test_familywise_gpu.py and
tests/test_familywise_host.py.  Everything is comparisons and integer counts, so the device must match bit for bit.

A value enters a maximum as v + 0.0 (a maximum of zeros is +0.0), a NaN never does, and a maximum over nothing or
over NaN alone is -inf with argmax -1; the argmax is the least index whose value equals the maximum."""
from __future__ import annotations

import math

import numpy as np

WG = 256      # FSCLG_MAXT_WG
TILE = 1024   # FSCLG_MAXT_TILE


def order_of(obs) -> np.ndarray:
    """Observed value descending, ties by index ascending, a NaN after every number."""
    x = np.asarray(obs, dtype=np.float64)
    return np.array(sorted(range(len(x)), key=lambda i: (math.isnan(x[i]), -x[i] if not math.isnan(x[i]) else 0.0, i)),
                    dtype=np.int32)


def _max_arg(v: np.ndarray, idx: np.ndarray):
    """Maximum and first argmax of the values v (canonical zeros) at point indices idx (ascending)."""
    ok = ~np.isnan(v)
    if not ok.any():
        return -np.inf, -1
    mx = v[ok].max()
    return float(mx), int(idx[ok][np.flatnonzero(v[ok] == mx)[0]])


def kernel(clr, obs, order, group, n_groups: int) -> dict:
    T = np.asarray(clr, dtype=np.float64) + 0.0
    x = np.asarray(obs, dtype=np.float64)
    o = np.asarray(order, dtype=np.int64)
    g = np.asarray(group, dtype=np.int64)
    nt, m = T.shape
    all_idx = np.arange(m)
    res = {"gmax": np.full(nt, -np.inf), "garg": np.full(nt, -1, np.int32), "chr_max": np.full((nt, n_groups), -np.inf),
           "chr_arg": np.full((nt, n_groups), -1, np.int32), "c_single": np.zeros(m, np.int32),
           "c_chr": np.zeros(m, np.int32), "c_step": np.zeros(m, np.int32)}
    members = [all_idx[g == c] for c in range(n_groups)]
    rank = np.empty(m, np.int64)
    rank[o] = np.arange(m)
    for t in range(nt):
        row = T[t]
        res["gmax"][t], res["garg"][t] = _max_arg(row, all_idx)
        for c in range(n_groups):
            res["chr_max"][t, c], res["chr_arg"][t, c] = _max_arg(row[members[c]], members[c])
        clean = np.where(np.isnan(row), -np.inf, row)
        u = np.maximum.accumulate(clean[o][::-1])[::-1] if m else clean   # u[j] = max over ranks k >= j
        with np.errstate(invalid="ignore"):
            res["c_single"] += (res["gmax"][t] >= x).astype(np.int32)
            if m:
                res["c_chr"] += (res["chr_max"][t][g] >= x).astype(np.int32)
                res["c_step"] += (u[rank] >= x).astype(np.int32)
    return res


def combine(c_single, c_chr, c_step, order, trials: int) -> dict:
    n, d = len(order), trials + 1.0
    rank, mono = np.zeros(n, np.int32), np.zeros(n, np.int64)
    run = 0
    for j, i in enumerate(order):
        run = int(c_step[i]) if j == 0 else max(run, int(c_step[i]))
        rank[i], mono[i] = j + 1, run
    return {"rank": rank, "p_single": (1.0 + np.asarray(c_single, np.float64)) / d,
            "p_chr": (1.0 + np.asarray(c_chr, np.float64)) / d, "p_step": (1.0 + mono) / d, "mono": mono}


def k_of(trials: int, level: float) -> int:
    return min(trials, int(math.floor(level * (trials + 1.0) + 1e-9)))


def threshold(maxima, level: float):
    M = len(maxima)
    k = k_of(M, level) if M else 0
    return k, (float(np.sort(np.asarray(maxima, np.float64))[::-1][k - 1]) if k > 0 else None)


def num(v, fmt: str) -> str:
    return "NA" if v is None or v != v or abs(v) == math.inf else fmt % v


def output_rows(names, chrs, pos, clr, lalpha, res: dict, trials: int, label=None) -> list:
    """The --familywise-file rows (split into columns): one per point, one per chromosome, one for the genome."""
    cb = combine(res["c_single"], res["c_chr"], res["c_step"], res["order"], trials)
    pre = [label] if label else []
    rows = []
    for i in range(len(pos)):
        ps = cb["p_step"][i]
        rows.append(pre + [names[chrs[i]], str(pos[i]), "%1.2f" % clr[i], "%1.3e" % math.exp(lalpha[i]), str(cb["rank"][i]),
                           "%1.3e" % cb["p_chr"][i], "%1.3e" % cb["p_single"][i], "%1.3e" % ps, "%1.3f" % (0.0 - math.log10(ps))])
    k05, k01 = k_of(trials, 0.05), k_of(trials, 0.01)

    def summary(name, maxima, pts, cnt):
        d = np.sort(np.asarray(maxima, np.float64))[::-1]
        q50 = d[trials // 2] if trials & 1 else 0.5 * (d[trials // 2 - 1] + d[trials // 2])
        thr = [threshold(maxima, a)[1] for a in (0.10, 0.05, 0.01)]
        return pre + [name, "summary", str(trials), str(len(pts)), num(float(q50), "%1.2f")] + [num(v, "%1.2f") for v in thr] + \
            [str(sum(1 + int(cnt[i]) <= k05 for i in pts)), str(sum(1 + int(cnt[i]) <= k01 for i in pts))]
    for c, name in enumerate(names):
        rows.append(summary(name, np.asarray(res["chr_max"]).reshape(trials, -1)[:, c], [i for i in range(len(pos)) if chrs[i] == c],
                            res["c_chr"]))
    rows.append(summary("genome", res["gmax"], list(range(len(pos))), cb["mono"]))
    return rows


def cases() -> list:
    """Crafted inputs at the smallest shapes where the kernel can go wrong: (name, clr, obs, group, n_groups)."""
    g = np.random.default_rng(20261021)
    out = []

    def groups(m, G, empty=None):
        """m points in G groups, sorted by group as chromosomes are; ``empty`` gets no point."""
        use = [c for c in range(G) if c != empty]
        return np.sort(np.array([use[k % len(use)] for k in range(m)], np.int32)) if m else np.zeros(0, np.int32)

    def values(nt, m):
        """Null-like CLRs: most exactly zero, the rest from a short list, so that ties abound."""
        v = g.choice(np.array([0.0, 0.0, 0.0, 0.5, 1.25, 2.0, 3.75, 7.5]), size=(nt, m))
        return v.astype(np.float64)

    for m in (1, 63, 64, 65, WG - 1, WG, WG + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        for nt in (1, 5):
            for G, empty in ((1, None), (22, 7)):
                T = values(nt, m)
                obs = g.choice(np.array([0.0, 0.0, 0.5, 1.25, 2.0, 7.5, 9.0]), size=m)   # ties within obs and with T
                out.append((f"m{m}_t{nt}_g{G}", T, obs, groups(m, G, empty), G))
    # an all-zero trial with points whose observed CLR is 0; a NaN entry, an all-NaN trial, a +inf; the maximum in
    # the first and in the last position; a -0.0; an obs above everything and a NaN obs; groups not sorted
    m = TILE + 37
    T = values(7, m)
    T[0, :] = 0.0
    T[1, 5] = np.nan
    T[2, :] = np.nan
    T[3, m // 2] = np.inf
    T[4, 0] = 50.0
    T[5, m - 1] = 50.0
    T[6, :] = -0.0
    obs = g.choice(np.array([0.0, 0.0, 0.5, 2.0, 7.5]), size=m)
    obs[3], obs[m - 2], obs[11] = 100.0, np.nan, np.inf
    out.append(("special", T, obs, groups(m, 22, 7), 22))
    out.append(("special_unsorted_groups", T, obs, g.permutation(groups(m, 22, 7)).astype(np.int32), 22))
    out.append(("all_nan_one_group", np.full((1, 65), np.nan), np.zeros(65), groups(65, 1), 1))
    return out
