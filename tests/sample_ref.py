"""A NumPy restatement of the sweep-model sampler's site semantics (include/fsclg.h,
fsclg_sample_submit), for tests/test_simulate_host.py and tests/test_simulate_gpu.py.

Per site: the nearest sweep of its chromosome (a tie goes to the lower position), log_ad =
logt(|d|) + log(alpha) with the three-branch logt of the scan, the model spectrum p_f =
exp(spline_f(log_ad)) over f = 1 .. n-1 (the neutral spectrum without a sweep or past LOG_AD_MAX),
one counter-based uniform u(seed, rep, site), and the least f whose cumulative sum exceeds u * S.

The cumulative sums are NumPy's sequential ones; the device forms them in another (fixed) order,
and its exp differs from NumPy's by a few ulp.  A sum of at most 400 such terms is then off by
about 1e-13 relative, so a site whose threshold t = u * S lies within MARGIN = 1e-9 (relative to S)
of some cumulative sum is *undecided*: the tests use only inputs without such a site (checked on
the CPU) and then demand equality at every site.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

import fscl_amd
import walk_ref as wr

LOG_AD_MIN, LOG_AD_MAX = -20.0, 4.0
MARGIN = 1e-9
MASK = (1 << 64) - 1
SAMPLE_KEY = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------ the uniform draw
def mix64_py(z: int) -> int:
    """splitmix64's output function in Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def uniform_py(seed: int, rep: int, i: int) -> float:
    h = mix64_py(mix64_py((seed & MASK) ^ SAMPLE_KEY) ^ (((rep & 0xFFFFFFFF) << 32) | (i & 0xFFFFFFFF)))
    return (h >> 11) * 2.0 ** -53


def _mix64(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniforms(seed: int, rep: int, n: int) -> np.ndarray:
    key = np.uint64(mix64_py((seed & MASK) ^ SAMPLE_KEY))
    ctr = (np.uint64((rep & 0xFFFFFFFF) << 32)) | np.arange(n, dtype=np.uint64)
    h = _mix64(np.full(n, key, dtype=np.uint64) ^ ctr)
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# ------------------------------------------------------------------ the host tables
@dataclass
class Model:
    pos: np.ndarray        # int64 [n_snps]
    chrom: np.ndarray      # int32 [n_snps] chromosome index of each site
    depth_p: np.ndarray    # int32 [n_snps]
    obs: np.ndarray        # int32 [n_snps] observed count (kept by a degenerate site)
    folded: np.ndarray     # int32 [n_snps]
    depth_n: list          # sample size of each depth index
    coef: list             # per depth float64 [n-1][n_iv][4]: the unfolded rows f = 1 .. n-1
    fsp: list              # per depth float64 [n-1]: sm_p[depth].fsp[1 .. n-1]
    log_table: np.ndarray
    step: float


def model_of(scan, tables) -> Model:
    """The sites of a scan_t and the coefficients of its sm_ptable_t array, through ctypes."""
    s = scan.contents
    n = s.n_snps
    raw = np.frombuffer((fscl_amd.SnpT * n).from_address(C.addressof(s.snps.contents)),
                        dtype=np.dtype([("chr", "i4"), ("pos", "i4"), ("null_logl", "f8"), ("obs_freq", "i4"),
                                        ("depth_p", "i4"), ("folded", "i4"), ("pad", "i4")]))
    assert raw.dtype.itemsize == C.sizeof(fscl_amd.SnpT)
    chrom = np.full(n, -1, dtype=np.int32)
    for c in range(s.n_chromosomes):
        lim = s.chr_limits[c]
        chrom[lim.start_index:lim.start_index + lim.n_snps] = c
    depth_n, coef, fsp = [], [], []
    n_iv = None
    for d in range(s.n_depths):
        t = tables[d]
        nn = int(t.sample_size)
        assert nn == s.sample_depths[d]
        rows = []
        for f in range(1, nn):
            sp = t.spline_func[f].contents
            n_iv = sp.n if n_iv is None else n_iv
            assert sp.n == n_iv
            rows.append(np.ctypeslib.as_array(sp.coef[0], shape=(sp.n * 4,)).reshape(sp.n, 4).copy())
        depth_n.append(nn)
        coef.append(np.array(rows, dtype=np.float64).reshape(nn - 1, n_iv, 4))
        fsp.append(np.array([t.fsp[f] for f in range(1, nn)], dtype=np.float64))
    return Model(raw["pos"].astype(np.int64), chrom, raw["depth_p"].astype(np.int32), raw["obs_freq"].astype(np.int32),
                 raw["folded"].astype(np.int32), depth_n, coef, fsp, wr.log_table(),
                 (LOG_AD_MAX - LOG_AD_MIN) / (n_iv + 1.0))


# ------------------------------------------------------------------ the site semantics
def nearest_sweep(sweeps, chrom: int, pos: int) -> int:
    """Index in ``sweeps`` ((chr index, pos, alpha) each) of the sweep that governs a site, -1 if
    its chromosome has none: least |d|, a tie to the lower sweep position, then to the first given."""
    best, key = -1, None
    for k, (c, p, _a) in enumerate(sweeps):
        if int(c) != int(chrom):
            continue
        q = (abs(int(pos) - int(p)), int(p))
        if key is None or q < key:
            best, key = k, q
    return best


def site_log_ad(M: Model, sweeps):
    """(log_ad, governing sweep index) of every site: NaN and -1 on a chromosome without a sweep."""
    n = len(M.pos)
    which = np.full(n, -1, dtype=np.int64)
    dist = np.zeros(n, dtype=np.int64)
    spos = np.zeros(n, dtype=np.int64)
    for k, (c, p, _a) in enumerate(sweeps):
        on = M.chrom == int(c)
        d = np.abs(M.pos - int(p))
        take = on & ((which < 0) | (d < dist) | ((d == dist) & (int(p) < spos)))
        which[take], dist[take], spos[take] = k, d[take], int(p)
    la = np.array([np.log(np.float64(a)) for _c, _p, a in sweeps] + [np.nan])
    x = np.where(which >= 0, wr.logt(dist, M.log_table) + la[which], np.nan)
    return x, which


@dataclass
class Draw:
    f: np.ndarray          # int32 [n_snps] the drawn derived count (the observed one at a degenerate site)
    margin: np.ndarray     # float64: min_f |t - C_f| / S (inf at a degenerate site)
    log_ad: np.ndarray     # float64, NaN without a sweep
    swept: np.ndarray      # bool: the site took the sweep branch
    p_drawn: np.ndarray    # float64: p_f of the drawn f (NaN at a degenerate site)
    n_degenerate: int

    @property
    def undecided(self) -> int:
        return int((self.margin <= MARGIN).sum())


def _clean(p):
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(p) & (p >= 0.0), p, 0.0)


def sample(M: Model, sweeps, seed: int, rep: int) -> Draw:
    n = len(M.pos)
    u = uniforms(seed, rep, n)
    x, which = site_log_ad(M, sweeps)
    with np.errstate(invalid="ignore"):
        swept = (which >= 0) & ~(x > LOG_AD_MAX)
    f_out = M.obs.copy()
    margin = np.full(n, np.inf)
    p_drawn = np.full(n, np.nan)
    n_deg = 0
    for d, nn in enumerate(M.depth_n):
        m = nn - 1
        idx = np.flatnonzero(M.depth_p == d)
        if not len(idx) or m < 1:
            n_deg += len(idx)
            continue
        P = np.empty((len(idx), m))
        sw = swept[idx]
        P[~sw] = _clean(M.fsp[d])[None, :]
        if sw.any():
            xs = x[idx][sw]
            n_iv = M.coef[d].shape[1]
            with np.errstate(all="ignore"):
                iv = np.clip(np.trunc((xs - LOG_AD_MIN) / M.step), 0, n_iv - 1).astype(np.int64)
                c = M.coef[d][:, iv, :]                      # [m][sites][4]
                y = xs * (c[..., 0] * xs * xs + c[..., 1] * xs + c[..., 2]) + c[..., 3]
                P[sw] = _clean(np.exp(y)).T
        with np.errstate(all="ignore"):
            Cs = np.cumsum(P, axis=1)
            S = Cs[:, -1]
            ok = np.isfinite(S) & (S > 0.0)
            t = u[idx] * S
            over = Cs > t[:, None]
            first = np.argmax(over, axis=1)
            none = ~over.any(axis=1)
            last_pos = m - 1 - np.argmax(P[:, ::-1] > 0.0, axis=1)
            k = np.where(none, last_pos, first)
            mg = np.min(np.abs(Cs - t[:, None]), axis=1) / S
        f_out[idx[ok]] = (k[ok] + 1).astype(np.int32)
        margin[idx[ok]] = mg[ok]
        p_drawn[idx[ok]] = P[np.flatnonzero(ok), k[ok]]
        n_deg += int((~ok).sum())
    return Draw(f_out.astype(np.int32), margin, x, swept, p_drawn, n_deg)


# ------------------------------------------------------------------ the inputs of the tests
# Every input of tests/test_simulate_gpu.py, built once per process on the host (no GPU): the SNP
# file from synth.generate, the scan_t, the background spectra, the tables, the null model, and
# the sweeps, seed and replicate of its draw.  tests/test_simulate_host.py checks that the
# reference alone leaves no site of any of them undecided.
import functools  # noqa: E402
import tempfile  # noqa: E402
from pathlib import Path  # noqa: E402

from fscl_amd import synth  # noqa: E402

CHR_LEN = 60_000        # every site within 30 kb of the sweep: alpha d <= 3, the spectrum is far from neutral
BOOT_LEN = 3_000_000    # the bootstrap's chromosome: 30 coarse grid cells
ALPHA = 1e-4
WAVE_DEPTHS = (64, 65, 66, 129, 130)   # n - 1 = 63, 64, 65, 128, 129: around one and two waves
CASE_NAMES = ("d2_3",) + tuple(f"d{n}" for n in WAVE_DEPTHS) + ("mixed", "asc")
SEED, REP = 0x5EED5, 3


@dataclass
class Case:
    name: str
    path: Path
    scan: object
    fsp: object
    tables: object
    model: Model
    sweeps: list           # (chromosome index, pos, alpha)
    sweep_names: list      # "name:pos:alpha" of each, as the CLI takes them
    asc: tuple = (0, 1)


@functools.lru_cache(maxsize=None)
def _dir() -> Path:
    return Path(tempfile.mkdtemp(prefix="fscl_simulate_"))


def _load(name, chroms, min_depth=5, asc=(0, 1)):
    path = _dir() / f"{name}.snp"
    synth.write_snp_file(str(path), chroms)
    L = fscl_amd.get_lib()
    L.configure_logmsg(0)
    fscl_amd.init_log_table()
    scan = L.load_snp_input(str(path).encode(), 0, min_depth)   # (the C entry: depths below 5 allowed)
    fsp = fscl_amd.background_fsp(scan)
    tab = fscl_amd.compute_sweep_model_tables(scan, fsp, asc[0], asc[1])
    fscl_amd.compute_snp_null_model(scan, fsp)
    return path, scan, fsp, tab


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    mid = CHR_LEN // 2
    asc = (0, 1)
    if name == "d2_3":       # the degenerate ends n - 1 = 1 and 2, as two depths of one input
        chroms = synth.generate(1, CHR_LEN // 3, 6000, 3, seed=21, missing=0.5, max_missing=1)
        sweeps, min_depth = [(0, CHR_LEN // 6, ALPHA)], 2
    elif name in {f"d{n}" for n in WAVE_DEPTHS}:
        chroms = synth.generate(1, CHR_LEN, 3000, int(name[1:]), seed=22)
        sweeps, min_depth = [(0, mid, ALPHA)], 5
    elif name == "mixed":    # three chromosomes, two depths, 30 % folded; 3 003 sites
        chroms = synth.generate(3, CHR_LEN, 1001, 30, folded=0.3, seed=23, missing=0.2, max_missing=1)
        assert int(chroms[1][1][400]) > 5_000
        on_site = int(chroms[0][1][500])                 # a sweep exactly on a site: d = 0
        tie = int(chroms[1][1][400])                     # a site equidistant between two sweeps
        sweeps, min_depth = [(0, on_site, ALPHA), (1, tie + 5_000, 3e-4), (1, tie - 5_000, ALPHA)], 5
    elif name == "asc":
        asc = (20, 2)
        chroms = synth.generate(1, CHR_LEN, 3000, 40, seed=24, asc_depth=20, asc_min_freq=2)
        sweeps, min_depth = [(0, mid, ALPHA)], 5
    elif name == "boot":     # the bootstrap's input (compared with its own pieces, not with this reference)
        chroms = synth.generate(1, BOOT_LEN, 3000, 30, seed=25)
        sweeps, min_depth = [(0, BOOT_LEN // 2, 2e-4)], 5
    else:
        raise KeyError(name)
    path, scan, fsp, tab = _load(name, chroms, min_depth, asc)
    names = [f"{chroms[c][0]}:{p}:{a!r}" for c, p, a in sweeps]
    return Case(name, path, scan, fsp, tab, model_of(scan, tab), sweeps, names, asc)


@functools.lru_cache(maxsize=None)
def reference(name: str, neutral: bool = False, rep: int = REP) -> Draw:
    c = case(name)
    return sample(c.model, [] if neutral else c.sweeps, SEED, rep)
