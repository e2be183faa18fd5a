"""The window null sums restated, with the crafted null values that pin the kernels.

The reference of a window start a is acc = 0.0; acc += v[i] for i = a .. a + W - 1, strictly in order
(seq_windows).  chunk_params and lmax_of restate the host's choice of binades and block levels;
WaveModel restates chunk_table_kernel / chunk_tree_kernel (the tables, in the kernels' own float64
arithmetic) and window_chunk_kernel one wave at a time -- the same chunks, blocks and descents in the
same order, all 64 lanes at once -- and counts the events that say which regime a vector is in.
tests/test_window_ref.py checks, without a GPU, that the model equals the sequential sums and that
every case shows the events it is named for; tests/test_window_sums_gpu.py runs the cases on the device.
"""
from __future__ import annotations

import functools
import math
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

import walk_ref as wr

WC, WCG, CT_LMAX, TASK = 64, 16, 12, 256
MAX_WINDOW = 189 * 1024 - 1  # profile runs refuse longer windows (the walks' segment table, MAXSEG_W)
TWO53 = 9007199254740992.0
CHR_NULL = -123.25           # the sentinel whole-chromosome null sum of the chromosomes no longer than W


# ------------------------------------------------------------------ the two per-window restatements
def chunked_window_sum(v, W, a, emin, ne, C=64):
    """Python restatement of window_chunk_kernel / chunk_table_kernel (fsclg.hip): the exact
    chunked form of acc = 0.0; acc += v[i] for i = a .. a + W - 1."""

    def table(c, e):
        vals = v[c * C:(c + 1) * C]
        if len(vals) < C or any(not (x <= 0.0) or x == -math.inf for x in vals):
            return None
        u = math.ldexp(1.0, e - 52)
        out = []
        for p in (0, 1):
            d, par = 0, p
            for x in vals:
                q = x / u
                F = math.floor(q)
                if q - F == 0.5:
                    d += F + ((par + F) & 1)
                    par = 0
                else:
                    R = round(q)
                    d += R
                    par = (par + R) & 1
            out.append(d)
        return out

    s, i, end = 0.0, a, a + W
    while i < end:  # head
        if i % C == 0 and s <= -math.ldexp(1.0, emin):
            break
        s = s + v[i]
        i += 1
    while i + C <= end:  # chunks
        e = math.frexp(-s)[1] - 1 if s < 0.0 else None
        t = table(i // C, e) if e is not None and emin <= e < emin + ne else None
        if t is not None:
            u = math.ldexp(1.0, e - 52)
            m = int(s / u)
            mn = m + t[m & 1]
            if mn > -(1 << 53):
                s, i = mn * u, i + C
                continue
        for j in range(C):
            s = s + v[i + j]
        i += C
    while i < end:
        s = s + v[i]
        i += 1
    return s


def tree_window_sum(v, W, a, emin, ne, C=64, lmax=11):
    """Python restatement of the block steps of window_chunk_kernel (fsclg.hip):
    the chunk maps m -> m + D[m & 1] of chunk_table_kernel composed over aligned blocks of 2^L
    chunks (chunk_tree_kernel), and the running sum advanced by the largest aligned block that
    keeps it in its binade, halving the block on a crossing; the rest as the chunked form."""

    def table(c, e):
        vals = v[c * C:(c + 1) * C]
        if len(vals) < C or any(not (x <= 0.0) or x == -math.inf for x in vals):
            return None
        u = math.ldexp(1.0, e - 52)
        out = []
        for p in (0, 1):
            d, par = 0, p
            for x in vals:
                q = x / u
                F = math.floor(q)
                if q - F == 0.5:
                    d += F + ((par + F) & 1)
                    par = 0
                else:
                    R = round(q)
                    d += R
                    par = (par + R) & 1
            out.append(d)
        return out

    def compose(f1, f2):  # f2 after f1: the block map for either entry parity
        if f1 is None or f2 is None:
            return None
        return [f1[p] + f2[(p + f1[p]) & 1] for p in (0, 1)]

    memo = {}

    def block(L, b, e):  # the map of chunks [b 2^L, (b + 1) 2^L) in binade e
        key = (L, b, e)
        if key not in memo:
            memo[key] = table(b, e) if L == 0 else compose(block(L - 1, 2 * b, e), block(L - 1, 2 * b + 1, e))
        return memo[key]

    s, i, end = 0.0, a, a + W
    while i < end:  # head
        if i % C == 0 and s <= -math.ldexp(1.0, emin):
            break
        s = s + v[i]
        i += 1
    L = lmax
    while i + C <= end:  # whole chunks: aligned blocks
        e = math.frexp(-s)[1] - 1 if s < 0.0 else None
        c = i // C
        if e is not None and emin <= e < emin + ne:
            Lc = min(L, lmax, ((c & -c).bit_length() - 1) if c else lmax, ((end - i) // C).bit_length() - 1)
            t = block(Lc, c >> Lc, e)
            u = math.ldexp(1.0, e - 52)
            m = int(s / u)
            if t is not None and m + t[m & 1] > -(1 << 53):
                s, i, L = (m + t[m & 1]) * u, i + (C << Lc), lmax
                continue
            if Lc > 0:
                L = Lc - 1
                continue
        for j in range(C):  # the general step: chunk c site by site
            s = s + v[i + j]
        i += C
        L = lmax
    while i < end:
        s = s + v[i]
        i += 1
    return s


# ------------------------------------------------------------------ the reference and the host's rules
def seq_windows(v: np.ndarray, W: int, starts) -> np.ndarray:
    """acc = 0.0; acc += v[i], i = a .. a + W - 1 in order, for every a of starts."""
    return np.array([wr.seq_sum(0.0, v[a:a + W])[0] for a in starts])


def chunk_params(nullrow, W: int):
    """(emin, ne, accepted) of the host's chunk_params: 64 max|null| < 2^emin, W max|null| < 2^(emin+ne-1)
    (the device's null table has an all-zero row in front, which changes nothing)."""
    a = np.asarray(nullrow, dtype=np.float64)
    fin = np.abs(a[np.isfinite(a)])
    mx = float(fin.max()) if len(fin) else 0.0
    if not mx > 0.0:
        return 0, 0, False
    e1, e2 = math.frexp(64.0 * mx)[1], math.frexp(float(W) * mx)[1]
    ne = max(1, e2 - e1 + 1)
    return e1, ne, e1 + ne - 1 <= 52


def lmax_of(W: int, tree: bool = True) -> int:
    L = 0
    if tree:
        while L < CT_LMAX and (2 << L) * WC <= W:
            L += 1
    return L


def _low_bit(x: np.ndarray) -> np.ndarray:
    """(long long)x & 1 of an integer-valued double (0 where it is NaN or too large to matter)."""
    with np.errstate(all="ignore"):
        ok = np.abs(x) < 2.0 ** 62
        return np.where(ok, np.where(ok, x, 0.0).astype(np.int64) & 1, 0)


def compose_maps(x1, y1, x2, y2):
    """compose_maps of fsclg.hip on arrays of (d0, d1 - d0): the second map after the first."""
    with np.errstate(all="ignore"):
        a0, a1, b0, b1 = x1, x1 + y1, x2, x2 + y2
        D0 = a0 + np.where(_low_bit(a0) == 1, b1, b0)
        D1 = a1 + np.where(_low_bit(a1) == 0, b1, b0)  # entry parity 1: odd after an even increment
        return D0, D1 - D0


class WaveModel:
    """The chunk table, the block maps and window_chunk_kernel's stepping for null values v (one per
    site, all chromosomes in a row) and windows of W sites."""

    def __init__(self, v, W, emin, ne, lmax, wdesc=True):
        self.v = np.asarray(v, dtype=np.float64)
        self.n, self.W, self.emin, self.ne, self.lmax, self.wdesc = len(self.v), W, emin, ne, lmax, wdesc
        self.ev = Counter()
        self.nch = nch = (self.n + WC - 1) // WC
        whole = self.n // WC
        vals = self.v[:whole * WC].reshape(whole, WC)
        with np.errstate(all="ignore"):
            ok = np.all((vals <= 0.0) & (vals != -np.inf), axis=1)
        safe = np.where(ok[:, None], vals, 0.0)
        X = np.full((ne, nch), np.nan)
        Y = np.full((ne, nch), np.nan)
        ties = np.zeros((ne, nch), dtype=np.int64)
        for k in range(ne):
            e = emin + k
            q = safe * math.ldexp(1.0, 52 - min(e, 52))
            d0 = np.zeros(whole); d1 = np.zeros(whole)
            p0 = np.zeros(whole, dtype=np.int64); p1 = np.ones(whole, dtype=np.int64)
            for j in range(WC):
                qj = q[:, j]
                F = np.floor(qj)
                tie = qj - F == 0.5
                Fi = F.astype(np.int64)
                R = np.rint(qj)
                Rp = R.astype(np.int64) & 1
                d0 = d0 + np.where(tie, (Fi + ((p0 + Fi) & 1)).astype(np.float64), R)
                d1 = d1 + np.where(tie, (Fi + ((p1 + Fi) & 1)).astype(np.float64), R)
                p0 = np.where(tie, 0, (p0 + Rp) & 1)
                p1 = np.where(tie, 0, (p1 + Rp) & 1)
                ties[k, :whole] += tie & ok
            X[k, :whole] = np.where(ok, d0, np.nan)
            Y[k, :whole] = np.where(ok, d1 - d0, np.nan)
        self.tab = [(X, Y)]
        self.tiecum = np.concatenate([np.zeros((ne, 1), dtype=np.int64), np.cumsum(ties, axis=1)], axis=1)
        self.ties = ties
        for L in range(1, lmax + 1):
            px, py = self.tab[L - 1]
            nb = nch >> L
            self.tab.append(compose_maps(px[:, 0:2 * nb:2], py[:, 0:2 * nb:2], px[:, 1:2 * nb:2], py[:, 1:2 * nb:2]))

    # -- one wave: the windows of starts ws0 .. ws0 + nv - 1
    def wave(self, ws0: int, nv: int) -> np.ndarray:
        W, emin, ne, ev, v = self.W, self.emin, self.ne, self.ev, self.v
        lane = np.arange(64)
        ws = ws0 + np.minimum(lane, nv - 1)
        end = ws + W
        s = np.zeros(64)
        wsL = ws0 + nv - 1
        cend = ((wsL + W - 1) >> 6) + 1
        fast_lo, fast_hi = (wsL + WC - 1) >> 6, (ws0 + W) >> 6
        c = ws0 >> 6

        def expo(x):
            return ((x.view(np.int64) >> 52) & 0x7FF) - 1023

        def stepped(m, d0, dd):
            with np.errstate(all="ignore"):
                return m + (d0 + (m.view(np.int64) & 1).astype(np.float64) * dd)

        def fits(mn):
            with np.errstate(all="ignore"):
                return bool(np.all(mn > -TWO53))

        def took(k, cc, l, m, dd):  # a table entry of level l applied at chunk cc, binade index k
            ev[f"level{l}"] += 1
            if self.tiecum[k, cc + (1 << l)] - self.tiecum[k, cc] > 0:
                ev["fast_tie"] += 1
            if l == 0 and self.ties[k, cc] == WC:
                ev["all_tie_chunk"] += 1
            if dd != 0.0:
                odd = int(np.count_nonzero(m.view(np.int64) & 1))
                ev["dd_odd" if l == 0 else "blk_dd_odd"] += odd
                ev["dd_even" if l == 0 else "blk_dd_even"] += 64 - odd
            if k >= 12:
                ev["k_ge_12"] += 1

        while c < cend:
            if fast_lo <= c < fast_hi:
                e = expo(s)
                eu = int(e[0])
                uniform = bool(np.all((s < 0.0) & (e == eu)))
                inr = emin <= eu < emin + ne
                if not uniform and bool(np.all(s < 0.0)) and np.all((e >= emin) & (e < emin + ne)):
                    ev["mixed_binade"] += 1
                if inr and uniform:
                    k = eu - emin
                    sc, isc = math.ldexp(1.0, 52 - eu), math.ldexp(1.0, eu - 52)
                    m = s * sc
                    if self.lmax > 0:
                        L = self.lmax

                        def entry(cc, l):
                            x, y = self.tab[l]
                            return float(x[k, cc >> l]), float(y[k, cc >> l])

                        while c < fast_hi:
                            Lc = min(L, (fast_hi - c).bit_length() - 1)
                            if c:
                                Lc = min(Lc, (c & -c).bit_length() - 1)
                            d0, dd = entry(c, Lc)
                            mn = stepped(m, d0, dd)
                            if fits(mn):
                                took(k, c, Lc, m, dd)
                                m = mn; c += 1 << Lc; L = self.lmax
                                continue
                            if d0 != d0 and Lc >= 1:
                                ev["nan_block"] += 1
                            if Lc == 0:
                                ev["break_chunk"] += 1
                                break
                            if not self.wdesc or Lc < 2:
                                L = Lc - 1
                                continue
                            ev["fail_ge2"] += 1
                            l1, l2 = Lc - 1, Lc - 2
                            a0, ad = entry(c, l1)
                            b0, bd = entry(c + (1 << l1), l2)
                            f0, fd = entry(c, l2)
                            ma = stepped(m, a0, ad)
                            if fits(ma):
                                took(k, c, l1, m, ad)
                                m = ma; c += 1 << l1
                                mb = stepped(m, b0, bd)
                                if fits(mb):
                                    took(k, c, l2, m, bd)
                                    m = mb; c += 1 << l2; L = self.lmax
                                    ev["desc_fit_fit"] += 1
                                    continue
                                ev["desc_fit_fail"] += 1
                            else:
                                mf = stepped(m, f0, fd)
                                if fits(mf):
                                    took(k, c, l2, m, fd)
                                    m = mf; c += 1 << l2; L = self.lmax
                                    ev["desc_fail_fit"] += 1
                                    continue
                                ev["desc_fail_fail"] += 1
                            if l2 == 0:
                                ev["break_descent"] += 1
                                break
                            L = l2 - 1
                        s = m * isc
                        if c >= fast_hi:
                            continue
                    else:
                        gn = min(WCG, fast_hi - c)
                        x, y = self.tab[0]
                        j = gn
                        for g in range(gn):
                            d0, dd = float(x[k, c + g]), float(y[k, c + g])
                            mn = stepped(m, d0, dd)
                            if not fits(mn):
                                j = g
                                ev["break_chunk"] += 1
                                break
                            took(k, c + g, 0, m, dd)
                            m = mn
                        s = m * isc
                        c += j
                        if j == gn:
                            continue
            # the general step for chunk c
            cb = c * WC
            lo, hi = np.maximum(ws - cb, 0), np.minimum(end - cb, WC)
            need = lo < hi
            full = need & (lo == 0) & (hi == WC)
            e = expo(s)
            can = full & (s < 0.0) & (e >= emin) & (e < emin + ne)
            if can.any():
                kk = np.where(can, e - emin, 0)
                x, y = self.tab[0]
                d0, dd = x[kk, c], y[kk, c]
                with np.errstate(all="ignore"):
                    m = s * np.ldexp(1.0, np.where(can, 52 - e, 0))
                    mn = stepped(m, d0, dd)
                    good = can & (mn > -TWO53)
                    s = np.where(good, mn * np.ldexp(1.0, np.where(can, e - 52, 0)), s)
                if good.any():
                    ev["own_entry"] += int(np.count_nonzero(good))
                    if len(set(kk[good].tolist())) > 1:
                        ev["own_entry_binades"] += 1
                    odd = (m.view(np.int64) & 1) == 1
                    ev["dd_odd"] += int(np.count_nonzero(good & (dd != 0.0) & odd))
                    ev["dd_even"] += int(np.count_nonzero(good & (dd != 0.0) & ~odd))
                    if np.any(self.ties[kk[good], c] > 0):
                        ev["fast_tie"] += 1
                    if np.any(kk[good] >= 12):
                        ev["k_ge_12"] += 1
                need = need & ~good
            head = full & need & ~(s != s) & ((s >= 0.0) | (e < emin))
            if head.any():
                ev["head"] += 1
            if need.any():
                if (full & need & ~head).any():
                    ev["chunk_by_sites"] += 1
                with np.errstate(all="ignore"):
                    for q in range(WC):
                        xq = v[cb + q] if cb + q < self.n else 0.0
                        mask = need & (q >= lo) & (q < hi)
                        sn = np.where(mask, s + xq, s)
                        if xq > 0.0 and np.any(mask & (s < 0.0) & (expo(s) >= emin) & (expo(sn) < expo(s))):
                            ev["binade_back"] += 1
                        s = sn
                    if np.any(need & (s > 0.0)):
                        ev["positive_sum"] += 1
            c += 1
        if np.any(np.abs(s[:nv]) < math.ldexp(1.0, emin)):
            ev["never_emin"] += 1
        return s[:nv]

    def windows(self, a: int, count: int, task: int = TASK) -> np.ndarray:
        """The sums of window starts a .. a + count - 1, in tasks of 256 starts from a."""
        out = []
        for t0 in range(a, a + count, task):
            tn = min(task, a + count - t0)
            for w0 in range(0, tn, 64):
                out.append(self.wave(t0 + w0, min(64, tn - w0)))
        return np.concatenate(out) if out else np.zeros(0)


# ------------------------------------------------------------------ the geometry of a profile run
@dataclass
class Run:
    chr: int
    site0: int   # the chromosome's site the first position stands on
    count: int


def point_geometry(chr_start, chr_n, er, run: Run):
    """(nearest_snp, window_start, window_end) of a run's positions -- one per site from site0, each
    on its SNP -- by init_scan_result's rule; global site indices."""
    cs, n = chr_start[run.chr], chr_n[run.chr]
    ce = cs + n - 1
    near = cs + run.site0 + np.arange(run.count)
    assert run.site0 >= 0 and run.site0 + run.count <= n
    ws = np.where(near - er < cs, cs, np.where(near + er > ce, max(cs, ce - 2 * er), near - er))
    we = np.where(near - er < cs, min(cs + 2 * er, ce), np.where(near + er > ce, ce, near + er))
    return near, ws, we


def window_ranges(chr_start, chr_n, er, runs):
    """The host's window_ranges: one range of window starts per run (from the site before the run's
    first), merged; and whether fsclg_slot_windows then sums only those (launch_partial_windows)."""
    W = 2 * er + 1
    need = []
    for r in runs:
        cs, n = chr_start[r.chr], chr_n[r.chr]
        if n <= W:
            continue
        ce = cs + n - 1

        def wsof(nl):
            near = cs + nl
            return cs if near - er < cs else (max(cs, ce - 2 * er) if near + er > ce else near - er)
        # search_snppos's j of a position on site i is max(i, 1): the least index in [1, n) at or past it
        nlo = max(max(r.site0, 1) - 1, 0)
        nhi = min(max(r.site0 + r.count - 1, 1), n - 1)
        need.append((wsof(nlo), wsof(nhi) + 1))
    need.sort()
    out = []
    for x in need:
        if out and x[0] <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], x[1]))
        else:
            out.append(x)
    all_ = sum((n - W + 1 + 255) // 256 for n in chr_n if n > W)
    waves = sum((b - a + 255) // 256 for a, b in out)
    return out, bool(all_) and 2 * waves < all_


# ------------------------------------------------------------------ the cases
@dataclass
class Geometry:
    name: str
    er: int
    chr_n: tuple

    @property
    def W(self):
        return 2 * self.er + 1

    @property
    def chr_start(self):
        return tuple(int(x) for x in np.concatenate([[0], np.cumsum(self.chr_n)[:-1]]))

    @property
    def n(self):
        return int(sum(self.chr_n))


GEOMS = {g.name: g for g in (
    Geometry("small", 300, (1500, 400, 1111, 700)),
    Geometry("mid", 4096, (8193 + 700,)),
    Geometry("mid-odd", 4095, (8191 + 700,)),       # lmax 5: 2^7 chunks do not fit 8191 sites
    Geometry("long", 300, (601 + 2499,)),            # 2500 windows: few runs are a partial set for the host
    Geometry("prod", 81920, (163841 + 321,)),
    Geometry("cap", 262144, (524289 + 64,)),
)}


@dataclass
class WCase:
    name: str
    geom: Geometry
    nullrow: np.ndarray
    row: np.ndarray                 # per site
    events: tuple                   # each must be counted at least once (test_window_ref.py)
    expect: dict = field(default_factory=dict)  # "accepted", "ne", "ne_min", "lmax"
    on_device: bool = True

    @property
    def values(self) -> np.ndarray:
        return self.nullrow[self.row]

    def dense_runs(self):
        """small: every site of every chromosome (windows at both ends, and the whole-chromosome
        window of the short one); the others: every window start of the long chromosome."""
        g = self.geom
        if g.name == "small":
            return [Run(c, 0, n) for c, n in enumerate(g.chr_n)]
        return [Run(0, g.er, g.chr_n[0] - g.W + 1)]

    def partial_runs(self):
        """Three disjoint runs of 1, 70 and 300 starts in one call, or none where they would not fit
        in half the windows."""
        g = self.geom
        nwin = g.chr_n[0] - g.W + 1
        if sum(n - g.W + 1 for n in g.chr_n if n > g.W) <= 2 * (371 + 3) or nwin < 700:
            return []
        return [Run(0, g.er + 5, 1), Run(0, g.er + 93, 70), Run(0, g.er + nwin - 340, 300)]

    def tables(self) -> wr.Tables:
        g = self.geom
        pos = np.concatenate([wr.POS0 + wr.SPACING * np.arange(n) for n in g.chr_n]).astype(np.int32)
        coef = np.zeros((len(self.nullrow), wr.N_IV, 4))
        return wr.Tables(pos, self.row.astype(np.uint32), coef, self.nullrow, wr.log_table())

    def model(self, tree=True, wdesc=True) -> WaveModel:
        emin, ne, ok = chunk_params(self.nullrow, self.geom.W)
        assert ok
        return WaveModel(self.values, self.geom.W, emin, ne, lmax_of(self.geom.W, tree), wdesc)

    def expected(self, runs):
        """[(nearest_snp, window_start, window_end, null_logl)] of the runs' points, from the
        sequential sums."""
        g, v, out = self.geom, self.values, []
        for r in runs:
            near, ws, we = point_geometry(g.chr_start, g.chr_n, g.er, r)
            if g.chr_n[r.chr] <= g.W:
                nl = np.full(r.count, CHR_NULL)
            else:
                u, inv = np.unique(ws, return_inverse=True)
                nl = seq_windows(v, g.W, u)[inv]
            out += list(zip(near.tolist(), ws.tolist(), we.tolist(), nl.tolist()))
        return out


BINADES = range(3, 24)  # every binade the windows of any geometry pass through with |null| of a few units


def _tie_rows():
    """Per binade e: -(k + 2^(e-53)) and -(k + 3 2^(e-53)) (lowest set bit u/2 at e: a tie there, and an
    exact multiple of u below e), -(k + 2^(e-52)) and -(k + 2^(e-51)) (an odd and an even multiple of u)."""
    rows = []
    for e in BINADES:
        h = math.ldexp(1.0, e - 53)
        k = [0.125 * (1 + (7 * e + j) % 30) for j in range(4)]  # 0.125 .. 3.75
        rows += [-(k[0] + h), -(k[1] + 3 * h), -(k[2] + 2 * h), -(k[3] + 4 * h)]
    return np.array(rows)


def _real_rows():
    from util import GOLD
    nul = wr.OracleTables(GOLD / "g2.snp").tables.nullrow
    nul = nul[np.isfinite(nul) & (nul < 0.0)]
    return np.unique(nul)[:400]


def _case(name, geom, nullrow, row, events, **kw):
    nullrow = np.asarray(nullrow, dtype=np.float64)
    assert len(nullrow) <= 400 and len(row) == GEOMS[geom].n and row.max() < len(nullrow)
    on_device = GEOMS[geom].W <= MAX_WINDOW
    return WCase(f"{geom}/{name}", GEOMS[geom], nullrow, np.asarray(row, dtype=np.int64), tuple(events), kw, on_device)


def _real(geom, seed=1):
    rng = np.random.default_rng(seed)
    nul = _real_rows()
    ev = ["level1", "own_entry", "head", "break_chunk"]
    if geom == "prod":
        ev += [f"level{L}" for L in range(1, 10)]
    return _case("real", geom, nul, rng.integers(0, len(nul), GEOMS[geom].n), ev)


def _ties(geom, seed=2):
    """Ties at every binade, entered with either parity; sites 64 j .. of one stretch all tie at the
    binade the windows that start ~600 sites before pass it in."""
    g = GEOMS[geom]
    rng = np.random.default_rng(seed)
    rows = _tie_rows()
    nul = np.concatenate([rows, [-1.0, -0.5, -2.25, -3.0]])
    row = rng.integers(0, len(nul), g.n)
    emin, ne, _ = chunk_params(nul, g.W)
    if g.n > 8000:  # a stretch of four chunks whose every site ties at binade e: |S| ~ 1.9 per site
        at = 640 if geom != "prod" else 1280
        e = 10 if geom != "prod" else 11
        i = 4 * (e - BINADES[0])
        row[at:at + 256] = rng.choice([i, i + 1], 256)
    ev = ["fast_tie", "dd_even", "dd_odd", "blk_dd_even", "blk_dd_odd", "own_entry", "head"]
    if g.n > 8000:
        ev.append("all_tie_chunk")
    if geom == "long":
        ev.append("mixed_binade")
    return _case("ties", geom, nul, row, ev)


def top_level(g) -> int:
    """The largest level with an aligned block past the first in the data: a window's first block is never
    stepped over whole (the sum starts at 0.0, below 2^emin), so level lmax itself is out of reach where
    only the block at chunk 0 fits (mid, prod)."""
    L = lmax_of(g.W)
    while L > 0 and (2 << L) * WC > g.n:
        L -= 1
    return L


def _crossings(geom, seed=3, share=0.125):
    """Mostly -1.0: the sum passes -2^e exactly 2^e sites after the window start, give or take the tie
    rows mixed in, which make a skipped, repeated or mis-composed block show in the low bits.  From the
    second block of the top level on the rows are mostly -0.25, so that this block keeps the sum in one
    binade and is taken whole."""
    g = GEOMS[geom]
    rng = np.random.default_rng(seed)
    nul = np.concatenate([[-1.0, -0.25], _tie_rows()])
    row = np.where(rng.random(g.n) < share, rng.integers(2, len(nul), g.n), 0)
    lt = top_level(g)
    ev = ["fast_tie", "break_chunk", "own_entry", "head", "level1", "mixed_binade"]
    if lt >= 5:
        z = (WC << lt) + WC
        row[z:] = np.where(row[z:] == 0, 1, row[z:])
        ev += ["fail_ge2", "desc_fit_fit", "desc_fit_fail", "desc_fail_fit", "desc_fail_fail", "break_descent"]
        ev += [f"level{L}" for L in range(1, lt + 1) if (geom, L) != ("cap", 11)]  # (cap's sums stop short of 2^19)
    return _case("crossings", geom, nul, row, ev, lmax=lmax_of(g.W))


def _irregular():
    """small: positive, NaN, -inf, signed zeros and subnormal null values inside chunks, each in some
    windows and not in others."""
    g = GEOMS["small"]
    rng = np.random.default_rng(4)
    tie = _tie_rows()
    special = [3.5, 6.0, 50.0 / 8, math.nan, -math.inf, -0.0, 0.0, -5e-324, -2.0 ** -1000, -2.0 ** -12]
    nul = np.concatenate([special, [-1.0, -2.0, -1.75, -3.0, -2.5], tie])
    S0 = len(special)
    row = S0 + rng.integers(0, len(nul) - S0, g.n)
    c0, c1, c2, c3 = g.chr_start
    row[c0 + 100] = 3            # NaN: the windows from 0 .. 100 of the first chromosome
    row[c0 + 3] = 2              # an early positive value: the sums of windows 0 .. 3 start positive
    row[c0 + 800] = 0            # +3.5 in a middle chunk: that chunk site by site for every window over it
    for j in range(620, 660, 9):  # +6.0 where windows starting ~260 sites before have just passed -512
        row[c0 + j] = 1
    for j, r in ((40, 5), (41, 6), (42, 7), (43, 8), (200, 5), (333, 7), (334, 8), (640, 6), (700, 5)):
        row[c2 + j] = r          # -0.0, 0.0, -5e-324, -2^-1000: at window starts and inside whole chunks
    row[c2:c2 + 3] = [5, 7, 6]   # a window that starts with -0.0
    row[c2 + 440:c3] = rng.choice([5, 6, 7, 8, 9, 9], c3 - c2 - 440)  # windows that never reach 2^emin
    row[c3 + 650] = 4            # -inf: the windows from 50 on of the last chromosome
    return _case("irregular", "small", nul, row,
                 ["nan_block", "chunk_by_sites", "positive_sum", "binade_back", "own_entry", "head", "fast_tie",
                  "never_emin"])


def _scaled(geom, lo, hi, seed=5, scale=1.0):
    """real-like values mapped onto [-hi, -lo] (times scale): their own low bits, the range chosen."""
    g = GEOMS[geom]
    rng = np.random.default_rng(seed)
    r = _real_rows()
    f = (r - r.min()) / (r.max() - r.min())
    nul = -(lo + (hi - lo) * f) * scale
    return nul, rng.integers(0, len(nul), g.n)


def _ne13(geom):
    """max|null| = 3.5: W max|null| passes 2^19 at prod (ne 13), 2^20 at cap (ne 14), and with every
    value above 3.25 the sums reach the binade of table index 12."""
    nul, row = _scaled(geom, 3.25, 3.5)
    ev = ["own_entry", "head", "level9"] + (["k_ge_12"] if geom == "cap" else [])
    return _case("ne13", geom, nul, row, ev, **({"ne": 13} if geom == "prod" else {"ne_min": 14}))


def _top_binade():
    """mid-odd, |null| just above 2^39: emin + ne - 1 == 52, where u = 1.  W max|null| < 2^52, so the sums
    end in binade 51 (u = 1/2): rows of -(2^39 - j + 1/4) tie there, -(2^39 + 1/2) would tie at 52."""
    g = GEOMS["mid-odd"]
    rng = np.random.default_rng(6)
    b = 2.0 ** 39
    nul = np.array([-(b + 0.5), -(b - 3.0 + 0.25), -(b - 17.0 + 0.75), -(b - 64.0 + 0.125), -(b - 5.0), -(b - 1.5),
                    -(b - 1000.0 + 0.375), -(0.75 * b + 0.25)])
    return _case("top_binade", "mid-odd", nul, rng.integers(0, len(nul), g.n),
                 ["fast_tie", "dd_even", "dd_odd", "level5", "own_entry", "head"], top=52)


def _sequential(kind):
    g = GEOMS["mid"] if kind == "big" else GEOMS["small"]
    rng = np.random.default_rng(7)
    if kind == "big":   # |null| near 2^45: W max|null| is past 2^52
        nul = -(2.0 ** 45) * np.array([1.0, 1.0 + 2.0 ** -40, 1.25, 1.5 + 2.0 ** -33, 1.999])
    elif kind == "zero":
        nul = np.array([0.0, -0.0, 0.0])
    else:
        nul = np.array([math.nan, math.nan])
    return _case(f"sequential-{kind}", g.name, nul, rng.integers(0, len(nul), g.n), [], accepted=False)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = [_real("small"), _ties("small"), _crossings("small"), _irregular(),
           _real("mid"), _ties("mid"), _crossings("mid"), _ties("mid-odd"), _crossings("mid-odd"),
           _top_binade(), _sequential("big"), _sequential("zero"), _sequential("nan"),
           _ties("long"), _crossings("long"),
           _real("prod"), _crossings("prod"), _ties("prod"), _ne13("prod"),
           _crossings("cap"), _ne13("cap")]
    return {c.name: c for c in out}


WORKER_CASES = ("small/irregular", "mid/crossings", "mid/ties", "prod/ne13")  # the child-process variants


# ------------------------------------------------------------------ a case on the device shim
def device_mismatches(shim, c: WCase, runs, label: str) -> list:
    """fsclg_profile over the runs in one call (the case uploaded before): every point's geometry and
    null_logl against the sequential reference, the mismatches as text with hex floats."""
    g = c.geom
    call = [(r.chr, wr.POS0 + wr.SPACING * r.site0, wr.SPACING, r.count) for r in runs]
    got = shim.profile(call, eval_range=g.er)
    want = c.expected(runs)
    assert len(got) == len(want)
    bad = []
    for i, ((p, _), (near, ws, we, nl)) in enumerate(zip(got, want)):
        if (p.nearest_snp, p.window_start, p.window_end) != (near, ws, we):
            bad.append(f"{c.name} {label} point {i}: geometry ({p.nearest_snp}, {p.window_start}, {p.window_end}) "
                       f"!= ({near}, {ws}, {we})")
        elif not wr.same(p.null_logl, nl):
            bad.append(f"{c.name} {label} point {i} window {ws}: null_logl {p.null_logl!r} "
                       f"({float(p.null_logl).hex()}) != {nl!r} ({float(nl).hex()})")
    return bad


def upload_case(shim, c: WCase):
    g = c.geom
    shim.upload(c.tables(), list(g.chr_start), list(g.chr_n))
    shim.set_chr_null(CHR_NULL, len(g.chr_n))
