"""NumPy reference of the block sums (fsclg_blocks_submit) and of fscl_amd_jackknife_combine.

block_sums starts from walk_ref.walk_terms: the walk's terms and their site indices are reordered to
ascending site index, grouped by clamp(pos // block_bp - b0, 0, nb - 1) and summed per group with
np.add.accumulate from +0.0.  jackknife_combine restates the host combination operation by operation.
"""
from __future__ import annotations

import math

import numpy as np

import walk_ref as wr


def walk_sites(T: wr.Tables, pt: wr.Point, la: float):
    """(terms, site indices) of one walk in ascending site index; its length is 1 + nl + nr."""
    t, (nl, nr) = wr.walk_terms(T, pt, la)
    if nl < 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    near = pt.nearest_snp
    idx = np.concatenate([[near], np.arange(near - 1, near - 1 - nl, -1), np.arange(near + 1, near + 1 + nr)]).astype(np.int64)
    o = np.argsort(idx, kind="stable")
    return t[o], idx[o]


def fold_groups(t, j, nb: int):
    """(sums [nb], counts [nb]) of the terms t grouped by the nondecreasing block ids j: every group summed with
    np.add.accumulate from +0.0 in the given order."""
    bs, cnt = np.zeros(nb), np.zeros(nb, dtype=np.uint32)
    if len(t) == 0:
        return bs, cnt
    assert (np.diff(j) >= 0).all()
    # positions ascend with the site index, so a group is a run of consecutive terms
    st = np.concatenate([[0], np.flatnonzero(np.diff(j)) + 1, [len(t)]])
    ln = np.diff(st)
    cnt[j[st[:-1]]] = ln
    with np.errstate(all="ignore"):
        small = np.flatnonzero(ln <= 80)
        if len(small):
            # one accumulate for the short groups, each padded behind with +0.0: a running sum started from
            # +0.0 is never -0.0, so adding +0.0 to it changes nothing (NaN stays NaN)
            pad = np.zeros((len(small), 1 + int(ln[small].max())))
            col = np.arange(pad.shape[1] - 1)
            take = col[None, :] < ln[small][:, None]
            pad[:, 1:][take] = t[(st[small][:, None] + col[None, :])[take]]
            bs[j[st[small]]] = np.add.accumulate(pad, axis=1)[:, -1]
        for g in np.flatnonzero(ln > 80):
            bs[j[st[g]]] = np.add.accumulate(np.concatenate([[0.0], t[st[g]:st[g + 1]]]))[-1]
    return bs, cnt


def block_sums(T: wr.Tables, pt: wr.Point, las, block_bp: int, b0: int, nb: int):
    """(bs [nb][n_la] float64, cnt [nb][n_la] uint32) of one position."""
    bs = np.zeros((nb, len(las)))
    cnt = np.zeros((nb, len(las)), dtype=np.uint32)
    for k, la in enumerate(las):
        t, idx = walk_sites(T, pt, float(la))
        j = np.clip(T.pos[idx].astype(np.int64) // int(block_bp) - int(b0), 0, nb - 1)
        bs[:, k], cnt[:, k] = fold_groups(t, j, nb)
    return bs, cnt


def fold(bs, skip=None):
    """V[p][k]: the sum of bs[p][j][k] over ascending j (j != skip) from +0.0."""
    v = np.zeros((bs.shape[0], bs.shape[2]))
    with np.errstate(all="ignore"):
        for j in range(bs.shape[1]):
            if j != skip:
                v = v + bs[:, j, :]
    return v


def first_max(v):
    """(ipos, ila, value) of the first strict maximum in position order, then alpha order; a NaN never
    wins; (-1, -1, nan) when every cell is NaN."""
    ip, ik, m = -1, -1, math.nan
    for p in range(v.shape[0]):
        for k in range(v.shape[1]):
            x = float(v[p][k])
            if x == x and (ip < 0 or x > m):
                ip, ik, m = p, k, x
    return ip, ik, m


def jackknife_combine(bs, cnt, pos, la):
    """The dict of fscl_amd_jackknife_combine's outputs: per block (has_terms, ipos, ila, v, n_terms) and the
    summary fields."""
    n_pos, nb, n_la = bs.shape
    blocks = []
    for b in range(nb):
        has = bool(cnt[:, b, :].any())
        ip, ik, m = first_max(fold(bs, b)) if has else (-1, -1, math.nan)
        blocks.append(dict(has_terms=int(has), ipos=ip, ila=ik, v=m, n_terms=0))
    ip, ik, m = first_max(fold(bs))
    g = sum(b["has_terms"] for b in blocks)
    out = dict(n_pos=n_pos, n_la=n_la, nb=nb, g=g, ipos=ip, ila=ik, v=m, top_shift=-1, top_loss=-1, n_edge_pos=0,
               n_edge_la=0, se_pos=math.nan, se_la=math.nan, se_clr=math.nan, bias_pos=math.nan, bias_la=math.nan,
               bias_clr=math.nan, blocks=blocks)
    if ip < 0:
        return out
    full = [float(pos[ip]), float(la[ik]), 2.0 * m]
    th, na, dmax, lmax, have_loss = [], 0, -1.0, 0.0, False
    for b, o in enumerate(blocks):
        o["n_terms"] = int(cnt[ip][b][ik])
        if not o["has_terms"]:
            continue
        if o["ipos"] < 0:
            na += 1
            continue
        t = [float(pos[o["ipos"]]), float(la[o["ila"]]), 2.0 * o["v"]]
        th.append(t)
        d, loss = abs(t[0] - full[0]), full[2] - t[2]
        if d > dmax:
            dmax, out["top_shift"] = d, b
        if not have_loss or loss > lmax:
            lmax, out["top_loss"], have_loss = loss, b, True
        out["n_edge_pos"] += o["ipos"] in (0, n_pos - 1)
        out["n_edge_la"] += o["ila"] in (0, n_la - 1)
    if g >= 2 and na == 0:
        for i, key in enumerate(("pos", "la", "clr")):
            s = 0.0
            for t in th:
                s += t[i]
            mean, ss = s / float(g), 0.0
            for t in th:
                ss += (t[i] - mean) * (t[i] - mean)
            out["se_" + key] = math.sqrt((float(g - 1) / float(g)) * ss)
            out["bias_" + key] = float(g - 1) * (mean - full[i])
    return out


def same_combine(blocks, summ, ref) -> list:
    """The differences between fscl_amd.jackknife_combine's records and jackknife_combine's dict."""
    bad = []
    for k in ("n_pos", "n_la", "nb", "g", "ipos", "ila", "top_shift", "top_loss", "n_edge_pos", "n_edge_la"):
        if int(summ[k]) != int(ref[k]):
            bad.append(f"summary {k}: {int(summ[k])} != {ref[k]}")
    for k in ("v", "se_pos", "se_la", "se_clr", "bias_pos", "bias_la", "bias_clr"):
        if not wr.same(float(summ[k]), float(ref[k])):
            bad.append(f"summary {k}: {float(summ[k])!r} != {ref[k]!r}")
    for b, (o, r) in enumerate(zip(blocks, ref["blocks"])):
        if (int(o["has_terms"]), int(o["ipos"]), int(o["ila"]), int(o["n_terms"])) != (r["has_terms"], r["ipos"], r["ila"], r["n_terms"]) \
                or not wr.same(float(o["v"]), float(r["v"])):
            bad.append(f"block {b}: {o} != {r}")
    return bad
