/* scan.c -- host driver of the CLR scan (scan-chromosome.c, sm-search.c entry points) over the
 * gfx950 kernels: the device state, the shares and exchanges, the scans, the output.  The
 * block-permutation tests are in trials.c, the analysis drivers in analyses.c; scan_internal.h
 * declares what they share with this file.
 *
 * The host keeps what is inherently serial in the reference: the cell
 * sequence, the block permutation drawn from the glibc rand() stream, the
 * sequential window null sums, and the pruning pass in ascending point order
 * (each may draw rand()).  Every search_maxpos -- the 99.6 % of the
 * reference's time -- runs on the GPU, one workgroup per cell, in lockstep
 * trials: host permutes -> H2D rows -> GPU evaluates all active cells ->
 * D2H CLRs -> host prunes.  With several ranks (one process per GPU) every
 * rank replays the same host logic and evaluates a cost-balanced contiguous
 * share of the cells; one int64 sum-allreduce per trial assembles the CLRs.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <omp.h>

#include "scan_internal.h"

#define PERM_SEED 0xFD821A6      /* fscl.c:135 */

/* fscl.c:33-34 define these; weak so the library links standalone */
__attribute__((weak)) int n_permute = 0;
__attribute__((weak)) char *output_fname = NULL;
__attribute__((weak)) char *prepend_label = NULL;

/* The permutation stream: glibc's rand() seeded once per process (srand(0xFD821A6) in
   init_options, fscl.c:135), so it continues across scan_permute calls as the reference's
   does (e.g. the per-block ms loop, fscl.c:296-305).  fscl_amd_srand() restarts it (what
   a fresh process would see). */
static fh_rand_t g_rng;
static int g_rng_seeded = 0;

void fscl_amd_srand(unsigned seed) {
  fh_srand(&g_rng, seed);
  g_rng_seeded = 1;
}

fh_rand_t *fh_perm_rng(void) {
  if (!g_rng_seeded) fscl_amd_srand(PERM_SEED);
  return &g_rng;
}

/* an integer environment switch clamped to [lo, hi]; dflt when unset (an empty or non-numeric
   value reads as 0, then clamped) */
int fh_env_int(const char *name, int dflt, int lo, int hi) {
  const char *e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  return !e ? dflt : v < lo ? lo : v > hi ? hi : v;
}

/* what the SIGINT dump writes (scan-chromosome.c:553-560 reads fscl.c's globals
   output_fname / prepend_label; a library caller without fscl.c sets them here) */
static const char *g_dump_fname = NULL, *g_dump_label = NULL;
static int g_dump_set = 0;

void fscl_amd_set_dump_output(const char *fname, const char *label) {
  g_dump_fname = fname; g_dump_label = label; g_dump_set = 1;
}

void fh_dump_target(const char **fname, const char **label) {
  *fname = g_dump_set ? g_dump_fname : output_fname;
  *label = g_dump_set ? g_dump_label : prepend_label;
}

/* ----------------------------------------------------------------- log table */
static double *g_log_table = NULL;

void init_log_table(void) { /* sm-search.c:14-26 */
  int i;
  if (g_log_table) return;
  g_log_table = fh_malloc(sizeof(double) * 0x10000, "log_table");
  for (i = 1; i <= 0xFFFF; i++) g_log_table[i] = log(i);
  g_log_table[0] = 0.; /* a sweep on top of a SNP counts as 1 bp away */
}
const double *fh_log_table(void) { init_log_table(); return g_log_table; }

/* scan-chromosome.c:23-37 */
void compute_snp_null_model(scan_t *s, double **fsp) {
  int i;
  for (i = 0; i < s->n_snps; i++) {
    snp_t *p = s->snps + i;
    const int depth = s->sample_depths[p->depth_p];
    if (p->folded && p->obs_freq != depth - p->obs_freq)
      p->null_logl = log(fsp[p->depth_p][p->obs_freq] + fsp[p->depth_p][depth - p->obs_freq]);
    else
      p->null_logl = log(fsp[p->depth_p][p->obs_freq]);
  }
}

/* sm-search.c:269-295: the coarse grid is an accumulated for-loop, the refine
   grid depends only on the coarse winner, so all of them are tabulated here
   with the reference's own floating-point loops */
int fh_alpha_grid(double *coarse, int max_coarse, double *refine, int32_t *n_refine) {
  const double step = (LOG_AD_MAX - LOG_AD_MIN) / 10.0;
  double la;
  int nc = 0, c;
  for (la = LOG_AD_MIN; la <= LOG_AD_MAX; la += step) {
    if (nc == max_coarse) return -1;
    coarse[nc++] = la;
  }
  for (c = 0; c <= nc; c++) { /* row nc: the initial state lalpha = LOG_AD_MAX (sm-search.c:272) */
    const double best = c < nc ? coarse[c] : LOG_AD_MAX;
    double le = best - step, re = best + step, s2;
    int k = 0;
    if (le < LOG_AD_MIN) le = LOG_AD_MIN;
    if (re > LOG_AD_MAX) re = LOG_AD_MAX;
    s2 = (re - le) / 15.;
    for (la = le + s2; la < re; la += s2) {
      if (k == 16) return -2;
      refine[c * 16 + k++] = la;
    }
    n_refine[c] = k;
  }
  return nc;
}

/* ---------------------------------------------------------- device state (scan_internal.h) */
dev_t_ D = {.rank = 0, .world = 1};


static void dev_close_all(void) {
  int l, k;
  for (l = 0; l < D.n_dev; l++) fsclg_close(D.ctx[l]);
  for (k = 0; k < FSCLG_N_SLOTS; k++) { fsclg_host_free(D.stage[k]); D.stage[k] = NULL; }
  D.stage_cap = 0;
  D.n_dev = 0;
  D.tab_key = NULL; D.snp_key = NULL;
  fh_sampler_forget();
}

int fscl_amd_set_devices(const int *devices, int n) {
  int l;
  if (n > FH_MAX_DEV || n < -1) return -1;
  dev_close_all();
  if (n == 0 || n == -1) { D.want_n = -1; return 0; }  /* every visible device */
  D.want_n = n;
  for (l = 0; l < n; l++) D.want_dev[l] = devices ? devices[l] : l;
  return 0;
}

int fscl_amd_set_device(int device) { return fscl_amd_set_devices(&device, 1); }

int fscl_amd_n_devices(void) { return D.n_dev; }

int fscl_amd_set_ranks(int rank, int world, fscl_amd_exchange_fn fn, void *ctx) {
  if (world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) return -1;
  fh_pool_drop();  /* the pool belongs to the old exchange */
  fh_shm_close(D.shm); D.shm = NULL;
  D.rank = rank; D.world = world; D.xfn = fn; D.xctx = ctx;
  return 0;
}

int fscl_amd_set_ranks_shm(int rank, int world, const char *name) {
  const char *e = getenv("FSCL_AMD_SHM_MB");
  const size_t cap = (size_t)(e && atoi(e) > 0 ? atoi(e) : 64) << 20;
  if (world < 1 || rank < 0 || rank >= world || !name) return -1;
  fh_pool_drop();  /* the pool belongs to the old exchange */
  fh_shm_close(D.shm); D.shm = NULL;
  D.rank = rank; D.world = world; D.xfn = NULL; D.xctx = NULL;
  if (world == 1) return 0;
  D.shm = fh_shm_open(rank, world, name, cap);
  return D.shm ? 0 : -1;
}

int fh_dbg(void) {
  static int v = -1;
  if (v < 0) v = getenv("FSCL_AMD_DEBUG") != NULL;
  return v;
}

void fh_dev_check(int r, const char *what) {
  if (r != FSCLG_OK) logmsg(MSG_FATAL, "fscl_amd: %s failed: %s (code %d)", what, fsclg_last_error(), r);
}

/* Scaling rehearsal (test build only: -DFSCL_AMD_REHEARSAL, fscl_amd/_build_rehearsal,
   tools/scale_sim.sh).  FSCL_AMD_SIM=record:<file> (one process, all shares) writes every
   batch's results; FSCL_AMD_SIM=replay:<file>:<world>[:<rank>] runs as one rank of a
   `world`-process job: it evaluates only its own share and takes the others from the recording
   (checking its own bit for bit) -- the time of a W-rank job's rank on one GPU.  The product
   library has no such hook: it refuses the variable. */
static void sim_init(void) {
  static int done = 0;
  const char *e = getenv("FSCL_AMD_SIM");
  if (done) return;
  done = 1;
  if (!e) return;
#ifdef FSCL_AMD_REHEARSAL
  {
    char path[1024];
    int w = 1, r = 0;
    if (sscanf(e, "record:%1023[^:]", path) == 1 && !strncmp(e, "record:", 7)) {
      D.sim = fopen(path, "wb");
      D.sim_replay = 0;
    } else if (!strncmp(e, "replay:", 7) && sscanf(e + 7, "%1023[^:]:%d:%d", path, &w, &r) >= 2) {
      D.sim = fopen(path, "rb");
      D.sim_replay = 1;
      D.world = w; D.rank = r; D.xfn = NULL; D.shm = NULL;
    }
    if (!D.sim) logmsg(MSG_FATAL, "fscl_amd: FSCL_AMD_SIM=%s: cannot open the file", e);
  }
#else
  logmsg(MSG_FATAL, "fscl_amd: FSCL_AMD_SIM is a scaling-rehearsal hook of the test build (fscl_amd/_build_rehearsal)");
#endif
}

#ifdef FSCL_AMD_REHEARSAL
/* the rehearsal's exchange: record the batch, or replay the other ranks' shares */
static void sim_exchange(fsclg_point_t *out, int n, int lo, int hi) {
  if (!D.sim_replay) {
    if (fwrite(&n, sizeof n, 1, D.sim) != 1 || fwrite(out, sizeof(fsclg_point_t), (size_t)n, D.sim) != (size_t)n)
      logmsg(MSG_FATAL, "fscl_amd: FSCL_AMD_SIM record write failed");
  } else {
    fsclg_point_t *rec = fh_malloc(sizeof(fsclg_point_t) * (n ? n : 1), "sim");
    int m = -1, i;
    if (fread(&m, sizeof m, 1, D.sim) != 1 || m != n || fread(rec, sizeof(fsclg_point_t), (size_t)n, D.sim) != (size_t)n)
      logmsg(MSG_FATAL, "fscl_amd: FSCL_AMD_SIM replay: batch of %d cells, recording has %d", n, m);
    for (i = lo; i < hi; i++)
      if (memcmp(&rec[i].lalpha, &out[i].lalpha, 4 * sizeof(double)) != 0)
        logmsg(MSG_FATAL, "fscl_amd: FSCL_AMD_SIM replay: cell %d of a batch differs from the recording", i);
    memcpy(out, rec, sizeof(fsclg_point_t) * (size_t)n);
    free(rec);
  }
}
#endif

void fh_dev_open(void) {
  int l, n;
  if (D.n_dev) return;
  sim_init();
  if (D.want_n == 0) {
    const char *e = getenv("FSCL_AMD_DEVICE");
    if (!e) e = getenv("LOCAL_RANK");
    D.want_dev[0] = e ? atoi(e) : 0;
    n = 1;
  } else if (D.want_n < 0) {
    n = fsclg_device_count();
    if (n > FH_MAX_DEV) n = FH_MAX_DEV;
    for (l = 0; l < n; l++) D.want_dev[l] = l;
  } else {
    n = D.want_n;
  }
  if (n < 1) logmsg(MSG_FATAL, "fscl_amd: no GPU visible (%s); the scan path runs only on the GPU", fsclg_last_error());
  for (l = 0; l < n; l++) {
    const int r = fsclg_open(D.want_dev[l], &D.ctx[l]);
    if (r != FSCLG_OK)
      logmsg(MSG_FATAL, "fscl_amd: cannot open GPU %d (%s); the scan path runs only on the GPU", D.want_dev[l],
             fsclg_last_error());
    D.dev[l] = D.want_dev[l];
    D.n_dev = l + 1;
    /* batch 0 -- the initial scan and the permutation pipeline's blocking batch: when it has
       few cells, each gets several workgroups (FSCL_AMD_SPLIT members, default 8; 1 = off) */
    {
      const char *e = getenv("FSCL_AMD_SPLIT");
      fh_dev_check(fsclg_set_batch_split(D.ctx[l], 0, e ? (atoi(e) < 1 ? 1 : atoi(e)) : 8), "batch split");
    }
  }
  if (n > 1) logmsg(MSG_STATUS, "fscl_amd: %d GPUs in this process", n);
}

static void free_rowmap(fh_rowmap_t *m) {
  free(m->depth_n); free(m->row_base); free(m->dev_row);
  memset(m, 0, sizeof *m);
}

/* flatten the sm_ptable_t spline trees into [row][interval][4] and upload them to the
   given contexts; device rows are those some site of snps (idx) uses, ranked by site count
   (the device caches a window of every row in LDS), or every row when all_rows is set */
static double *flatten_tables(fh_rowmap_t *m, const sm_ptable_t *sm, int n_depths, const int *depth_n,
                              const snp_t *snps, const int *idx, int n_idx, int all_rows, double **nullrow_out,
                              const double *null_known, int n_known) {
  int d, r, i;
  double *coef, *nullrow;
  unsigned char *seen;
  free_rowmap(m);
  m->n_depths = n_depths;
  m->depth_n = fh_malloc(sizeof(int) * n_depths, "rowmap");
  m->row_base = fh_malloc(sizeof(int) * n_depths, "rowmap");
  m->n_rows = 0;
  for (d = 0; d < n_depths; d++) {
    if (sm[d].sample_size != depth_n[d])
      logmsg(MSG_FATAL, "fscl_amd: sweep-model table %d is for depth %d, data has %d", d, sm[d].sample_size,
             depth_n[d]);
    m->depth_n[d] = depth_n[d];
    m->row_base[d] = m->n_rows;
    m->n_rows += depth_n[d] + 1 + depth_n[d] / 2 + 1;
  }
  m->n_iv = sm[0].spline_func[0]->n;
  /* null_logl is a function of the row (scan-chromosome.c:23-37): take it from the sites */
  seen = fh_calloc(m->n_rows, 1, "null rows");
  m->dev_row = fh_malloc(sizeof(int) * m->n_rows, "rowmap");
  {
    double *full_null = fh_calloc(m->n_rows, sizeof(double), "null rows");
    if (null_known) memcpy(full_null, null_known, sizeof(double) * (size_t)(n_known < m->n_rows ? n_known : m->n_rows));
    for (i = 0; i < n_idx; i++) {
      const snp_t *p = snps + (idx ? idx[i] : i);
      const uint32_t rr = fh_full_row(m, p);
      if (!seen[rr]) { full_null[rr] = p->null_logl; seen[rr] = 1; }
      else if (memcmp(&full_null[rr], &p->null_logl, sizeof(double)) != 0)
        logmsg(MSG_FATAL, "fscl_amd: null_logl differs between sites of the same class (call "
                          "compute_snp_null_model first)");
    }
    if (all_rows) {
      for (r = 0; r < m->n_rows; r++) m->dev_row[r] = r;
      m->n_dev_rows = m->n_rows;
    } else {
      /* device rows in descending order of site count (ties by row) */
      long long *cnt = fh_calloc(m->n_rows, sizeof(long long), "row counts");
      int *ord = fh_malloc(sizeof(int) * m->n_rows, "row order");
      int nu = 0, a, b;
      for (i = 0; i < n_idx; i++) cnt[fh_full_row(m, snps + (idx ? idx[i] : i))]++;
      for (r = 0; r < m->n_rows; r++) if (seen[r]) ord[nu++] = r;
      for (a = 1; a < nu; a++) {  /* insertion sort: a few hundred rows */
        const int v = ord[a];
        for (b = a; b > 0 && (cnt[ord[b - 1]] < cnt[v] || (cnt[ord[b - 1]] == cnt[v] && ord[b - 1] > v)); b--)
          ord[b] = ord[b - 1];
        ord[b] = v;
      }
      for (r = 0; r < m->n_rows; r++) m->dev_row[r] = -1;
      for (a = 0; a < nu; a++) m->dev_row[ord[a]] = a;
      m->n_dev_rows = nu;
      free(cnt);
      free(ord);
    }
    if (m->n_dev_rows == 0) m->n_dev_rows = 1;  /* no sites: one zero row keeps the tables well-formed */
    nullrow = fh_calloc(m->n_dev_rows, sizeof(double), "null rows");
    for (r = 0; r < m->n_rows; r++) if (m->dev_row[r] >= 0) nullrow[m->dev_row[r]] = full_null[r];
    free(full_null);
  }
  coef = fh_calloc((size_t)m->n_dev_rows * m->n_iv * 4, sizeof(double), "flat tables");
  for (d = 0; d < n_depths; d++) {
    const int n = depth_n[d];
    for (r = 0; r <= n + n / 2 + 1; r++) {
      const spline_t *sp = r <= n ? sm[d].spline_func[r] : sm[d].fspline_func[r - n - 1];
      const int dr = m->dev_row[m->row_base[d] + r];
      if (sp->n != m->n_iv) logmsg(MSG_FATAL, "fscl_amd: splines with different knot counts");
      if (dr < 0) continue;
      for (i = 0; i < sp->n; i++) memcpy(coef + ((size_t)dr * m->n_iv + i) * 4, sp->coef[i], sizeof(double) * 4);
    }
  }
  free(seen);
  *nullrow_out = nullrow;
  return coef;
}

static void upload_flat(fsclg_ctx *const *ctx, int n_ctx, const fh_rowmap_t *m, const double *coef,
                        const double *nullrow) {
  double coarse[16], refine[17 * 16];
  int32_t nref[17];
  const int nc = fh_alpha_grid(coarse, 16, refine, nref);
  int l;
  if (nc <= 0) logmsg(MSG_FATAL, "fscl_amd: alpha grid");
  for (l = 0; l < n_ctx; l++) {
    /* log_ad_step of the tables' knot grid (sm-spline.c:325) */
    fh_dev_check(fsclg_upload_tables(ctx[l], fh_log_table(), coef, m->n_dev_rows, m->n_iv, nullrow,
                                  (LOG_AD_MAX - LOG_AD_MIN) / (m->n_iv + 1.)),
              "upload tables");
    fh_dev_check(fsclg_set_alpha_grid(ctx[l], coarse, nc, refine, nref), "alpha grid");
  }
}

static void check_site(const scan_t *s, const snp_t *p) {
  const int n = s->sample_depths[p->depth_p];
  if (p->obs_freq < 0 || p->obs_freq > n || (p->folded && p->obs_freq > n / 2))
    logmsg(MSG_FATAL, "fscl_amd: site class %d out of range for depth %d (folded=%d)", p->obs_freq, n, p->folded);
}

/* content hash (64-bit words, multiply-xorshift), for the device caches' keys */
uint64_t fh_hash_words(const void *p, size_t n, uint64_t h) {
  const unsigned char *b = p;
  size_t i;
  for (i = 0; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, b + i, 8);
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
  }
  for (; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

/* make every local device hold this scan's sites and these tables; the cache key is a hash
   of the content (a freed and re-allocated scan may reuse addresses) */
void fh_prepare(scan_t *s, sm_ptable_t *sm) {
  int i, d, l;
  uint64_t key = 1469598103934665603ull;
  double *coef, *nullrow;
  init_log_table();
  fh_dev_open();
  key = fh_hash_words(&s->n_snps, sizeof s->n_snps, key);
  key = fh_hash_words(s->snps, sizeof(snp_t) * (size_t)s->n_snps, key);
  key = fh_hash_words(s->sample_depths, sizeof(int) * (size_t)s->n_depths, key);
  for (i = 0; i < s->n_chromosomes; i++) key = fh_hash_words(&s->chr_limits[i].start_index, 4 * sizeof(int), key);
  for (d = 0; d < s->n_depths; d++) {
    const int n = sm[d].sample_size;
    key = fh_hash_words(&n, sizeof n, key);
    for (i = 0; i <= n + n / 2 + 1; i++) {
      const spline_t *sp = i <= n ? sm[d].spline_func[i] : sm[d].fspline_func[i - n - 1];
      key = fh_hash_words(sp->coef[0], sizeof(double) * 4 * (size_t)sp->n, key);
    }
  }
  if (D.snp_key && key == D.key) return;
  DBG("prepare: uploading %d sites, %d depths to %d device(s)\n", s->n_snps, s->n_depths, D.n_dev);
  for (i = 0; i < s->n_snps; i++) check_site(s, s->snps + i);
  coef = flatten_tables(&D.rm, sm, s->n_depths, s->sample_depths, s->snps, NULL, s->n_snps, 0, &nullrow, NULL, 0);
  upload_flat(D.ctx, D.n_dev, &D.rm, coef, nullrow);
  free(coef);
  free(D.nullrow);
  D.nullrow = nullrow;
  free(D.row); free(D.pos); free(D.chr_start); free(D.chr_n);
  D.row = fh_malloc(sizeof(uint32_t) * s->n_snps, "rows");
  D.pos = fh_malloc(sizeof(int32_t) * s->n_snps, "positions");
  for (i = 0; i < s->n_snps; i++) {
    D.row[i] = fh_row_of(&D.rm, s->snps + i);
    D.pos[i] = s->snps[i].pos;
  }
  D.rb = D.rm.n_dev_rows <= 0x100 ? 1 : D.rm.n_dev_rows <= 0x10000 ? 2 : 4;
  free(D.rowp);
  D.rowp = fh_malloc((size_t)D.rb * (s->n_snps ? s->n_snps : 1), "rows");
  for (i = 0; i < s->n_snps; i++) {
    if (D.rb == 1) ((uint8_t *)D.rowp)[i] = (uint8_t)D.row[i];
    else if (D.rb == 2) ((uint16_t *)D.rowp)[i] = (uint16_t)D.row[i];
    else ((uint32_t *)D.rowp)[i] = D.row[i];
  }
  D.n_chr = s->n_chromosomes;
  D.chr_start = fh_malloc(sizeof(int32_t) * D.n_chr, "chr");
  D.chr_n = fh_malloc(sizeof(int32_t) * D.n_chr, "chr");
  for (i = 0; i < D.n_chr; i++) {
    D.chr_start[i] = s->chr_limits[i].start_index;
    D.chr_n[i] = s->chr_limits[i].n_snps;
  }
  for (l = 0; l < D.n_dev; l++)
    fh_dev_check(fsclg_upload_snps(D.ctx[l], D.pos, D.row, s->n_snps, D.chr_start, D.chr_n, D.n_chr), "upload snps");
  if (D.stage_cap < s->n_snps || D.stage_rb != D.rb) {
    int k;
    for (k = 0; k < FSCLG_N_SLOTS; k++) {
      fsclg_host_free(D.stage[k]);
      D.stage[k] = fsclg_host_alloc((size_t)D.rb * s->n_snps);
      if (!D.stage[k]) logmsg(MSG_FATAL, "fscl_amd: row staging: %s", fsclg_last_error());
    }
    D.stage_cap = s->n_snps;
    D.stage_rb = D.rb;
  }
  D.tab_key = sm; D.snp_key = s->snps; D.n_snps_key = s->n_snps; D.key = key;
}

/* the whole-chromosome null sums at each staging width (rows_impl.h), and their dispatch on D.rb */
#include "rows_impl.h"

void fh_chr_null_sums(const void *row, double *out) {
  if (D.rb == 1) chr_null_sums_8(row, out);
  else if (D.rb == 2) chr_null_sums_16(row, out);
  else chr_null_sums_32(row, out);
}

/* contiguous share [lo, hi) of n items for one share index: item i belongs to the
   share whose slice of the total cost holds the cost accumulated before i */
void fscl_amd_partition(const double *cost, int n, int rank, int world, int *lo, int *hi) {
  double tot = 0., acc = 0.;
  int i;
  *lo = *hi = n;
  if (world <= 1) { *lo = 0; return; }
  for (i = 0; i < n; i++) tot += cost[i];
  for (i = 0; i < n; i++) {
    int owner = tot > 0 ? (int)(acc / tot * world) : (int)((long long)i * world / n);
    if (owner >= world) owner = world - 1;
    if (owner >= rank && *lo == n) *lo = i;
    if (owner > rank) { *hi = i; break; }
    acc += cost[i];
  }
}

/* the local devices' shares of n items: lo[l], hi[l] (consecutive; this process's range is
   [lo[0], hi[n_dev - 1])) */
void fh_dev_shares(const double *cost, int n, int *lo, int *hi) {
  const int T = D.world * D.n_dev;
  int l;
  for (l = 0; l < D.n_dev; l++) {
    if (T <= 1) { lo[l] = 0; hi[l] = n; continue; }
    fscl_amd_partition(cost, n, D.rank * D.n_dev + l, T, &lo[l], &hi[l]);
  }
}

/* the same among the local devices alone: the analysis scans, which rank 0 evaluates by itself */
void fh_local_shares(const double *cost, int n, int *lo, int *hi) {
  int l;
  for (l = 0; l < D.n_dev; l++) fscl_amd_partition(cost, n, l, D.n_dev, &lo[l], &hi[l]);
}

static unsigned long long dev_terms(int l) {
  fsclg_stats_t st;
  return fsclg_get_stats(D.ctx[l], &st) == FSCLG_OK ? st.n_terms : 0ull;
}

/* One batch of an analysis scan (curves, surfaces, conditional scan, block sums) on the local
   devices' shares lo[], hi[] of its runs.  A scan fills a dev_job_t with its arrays and gives its
   submit (runs [lo, hi) to device l) and wait (device k's results to where run lo's belong); the
   protocol is here alone: every device is submitted to before the first is waited for; the first
   error ends the submits and is the one returned; every device submitted to is waited for, the one
   whose submit failed never.  dev_ms[k] gains device k's kernel time (a scan of several batches
   adds them up; the devices run side by side, so its time is dev_ms_max); *n_terms, if given,
   gains the terms the devices counted meanwhile. */
int fh_run_on_devices(const char *what, const int *lo, const int *hi, dev_submit_fn submit, dev_wait_fn wait,
                          double (*last_ms)(fsclg_ctx *, int), const dev_job_t *j, double *dev_ms,
                          unsigned long long *n_terms) {
  int l, k, n_sub, r = FSCLG_OK;
  for (l = 0; n_terms && l < D.n_dev; l++) *n_terms -= dev_terms(l);
  for (l = 0; l < D.n_dev && r == FSCLG_OK; l++) {
    DBG("%s: device %d, runs [%d, %d)\n", what, D.dev[l], lo[l], hi[l]);
    r = submit(l, lo[l], hi[l], j);
  }
  n_sub = r == FSCLG_OK ? l : l - 1; /* the submit that failed left nothing to wait for */
  for (k = 0; k < n_sub; k++) {
    const int rw = wait(k, lo[k], j);
    dev_ms[k] += last_ms(D.ctx[k], 0);
    if (r == FSCLG_OK) r = rw;
  }
  for (l = 0; n_terms && l < D.n_dev; l++) *n_terms += dev_terms(l);
  return r;
}

double fh_dev_ms_max(const double *dev_ms) {
  double ms = 0.;
  int l;
  for (l = 0; l < D.n_dev; l++)
    if (dev_ms[l] > ms) ms = dev_ms[l];
  return ms;
}

/* off[i]: the positions of the runs before run i, i <= n (malloc'd) */
size_t *fh_run_offsets(const fsclg_run_t *runs, int n) {
  size_t *off = fh_malloc(sizeof(size_t) * ((size_t)n + 1), "run offsets");
  int i;
  off[0] = 0;
  for (i = 0; i < n; i++) off[i + 1] = off[i] + (size_t)runs[i].count;
  return off;
}

/* complete a batch's results on every rank: this process holds [lo, hi) of out[n].  With
   `flags` (this rank's flag word on entry, the OR over the ranks on return) the exchange is
   made even for an empty batch, and out[] must have room for n + 1 items (the torch
   exchange carries the word in item n). */
void fh_exchange_points_flags(fsclg_point_t *out, int n, int lo, int hi, unsigned *flags) {
#ifdef FSCL_AMD_REHEARSAL
  if (D.sim) { sim_exchange(out, n, lo, hi); return; }
#endif
  if (D.world <= 1 || (n == 0 && !flags)) return;
  if (D.shm) {
    if (fh_shm_allgather_flags(D.shm, out, sizeof(fsclg_point_t), n, lo, hi, flags) != 0)
      logmsg(MSG_FATAL, "fscl_amd: rank exchange failed");
    return;
  }
  memset(out, 0, sizeof(fsclg_point_t) * (size_t)lo);
  memset(out + hi, 0, sizeof(fsclg_point_t) * (size_t)(n - hi));
  if (flags) {
    memset(out + n, 0, sizeof(fsclg_point_t));
    ((long long *)(out + n))[0] = *flags;
  }
  if (D.xfn((long long *)out, (int)((n + (flags ? 1 : 0)) * (sizeof(fsclg_point_t) / sizeof(long long))), D.xctx) != 0)
    logmsg(MSG_FATAL, "fscl_amd: rank exchange failed");
  if (flags) *flags = ((long long *)(out + n))[0] != 0;
}

void fh_exchange_points(fsclg_point_t *out, int n, int lo, int hi) { fh_exchange_points_flags(out, n, lo, hi, NULL); }

/* every rank's `word` must be the same (collective; not in a rehearsal replay, whose exchanges
   are the recorded batches) */
void fh_ranks_agree(const char *what, uint64_t word) {
  fsclg_point_t *a;
  int r;
  if (D.world <= 1 || D.sim) return;
  a = fh_calloc((size_t)D.world + 1, sizeof(fsclg_point_t), "agree");
  memcpy(&a[D.rank].lalpha, &word, sizeof word);
  a[D.rank].flags = 1;
  fh_exchange_points(a, D.world, D.rank, D.rank + 1);
  for (r = 0; r < D.world; r++)
    if (a[r].flags != 1 || memcmp(&a[r].lalpha, &word, sizeof word) != 0)
      logmsg(MSG_FATAL, "fscl_amd: ranks disagree on %s (rank %d vs rank %d)", what, D.rank, r);
  free(a);
}

/* evaluate cells, each local device its share, then complete the results on every rank */
void fh_eval_cells(const fsclg_cell_t *cells, int n, int eval_range, int bp_resl, fsclg_point_t *out) {
  double *cost = NULL;
  int lo[FH_MAX_DEV], hi[FH_MAX_DEV], l, i;
  if (D.world * D.n_dev > 1) {
    cost = fh_malloc(sizeof(double) * (n ? n : 1), "cost");
    for (i = 0; i < n; i++) cost[i] = fh_window_cost(cells[i].chr, eval_range);
  }
  fh_dev_shares(cost, n, lo, hi);
  free(cost);
  for (l = 0; l < D.n_dev; l++) {
    DBG("search_maxpos: device %d, cells [%d, %d)\n", D.dev[l], lo[l], hi[l]);
    fh_dev_check(fsclg_search_submit(D.ctx[l], 0, 0, cells + lo[l], hi[l] - lo[l], eval_range, bp_resl),
              "search submit");
    D.st.gp_evals += (unsigned long long)(hi[l] - lo[l]);
  }
  for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_search_wait(D.ctx[l], 0, out + lo[l]), "search wait");
  fh_exchange_points(out, n, lo[0], hi[D.n_dev - 1]);
}

void fh_to_scan_pt(scan_pt_t *p, const fsclg_point_t *o) {
  memset(p, 0, sizeof *p);
  p->chr = o->chr; p->nearest_snp = o->nearest_snp; p->sweep_pos = o->sweep_pos; p->n_snps = o->n_snps;
  p->window_start = o->window_start; p->window_end = o->window_end;
  p->lalpha = o->lalpha; p->null_logl = o->null_logl; p->sm_logl = o->sm_logl; p->clr = o->clr;
}

typedef struct { scan_pt_t p; int seq; } keyed_pt_t;
static int pt_cmp(const void *va, const void *vb) {
  const keyed_pt_t *a = va, *b = vb;
  if (a->p.chr != b->p.chr) return a->p.chr < b->p.chr ? -1 : 1;
  if (a->p.sweep_pos != b->p.sweep_pos) return a->p.sweep_pos < b->p.sweep_pos ? -1 : 1;
  return a->seq - b->seq; /* scan-chromosome.c:218-225 under glibc's stable merge sort */
}

/* the unpermuted rows and whole-chromosome null sums into slot 0 of every device */
void fh_set_original_rows(void) {
  double *nul = fh_malloc(sizeof(double) * (D.n_chr ? D.n_chr : 1), "null sums");
  int l;
  fh_chr_null_sums(D.rowp, nul);
  for (l = 0; l < D.n_dev; l++) {
    fh_dev_check(fsclg_set_rows(D.ctx[l], NULL), "set rows");
    fh_dev_check(fsclg_set_chr_null(D.ctx[l], nul), "set null sums");
  }
  free(nul);
}

/* what the fscl_amd_*_runs test handles begin with: the arguments, the scan on the devices, and the
   rows the runs are evaluated on -- the uploaded ones (rows NULL: *slot 0) or `rows` (n_snps device
   rows, set into slot 1 of the first device with their whole-chromosome null sums: *slot 1) */
int fh_runs_handle_begin(scan_t *s, sm_ptable_t *sm, const fsclg_run_t *runs, int n_runs, const uint32_t *rows,
                             int *slot) {
  double *nul;
  int i, r;
  if (!s || !sm || (!runs && n_runs) || n_runs < 0) return FSCLG_E_ARG;
  fh_prepare(s, sm);
  *slot = 0;
  if (!rows) { fh_set_original_rows(); return FSCLG_OK; }
  for (i = 0; i < s->n_snps; i++)
    if (rows[i] >= (uint32_t)D.rm.n_dev_rows) return FSCLG_E_ARG;
  nul = fh_malloc(sizeof(double) * (D.n_chr ? D.n_chr : 1), "null sums");
  chr_null_sums_32(rows, nul);
  *slot = 1;
  r = fsclg_slot_set_rows(D.ctx[0], *slot, rows, nul);
  free(nul);
  return r;
}

/* the cell sequence one scan_thread walks (scan-chromosome.c:176-212) */
fsclg_cell_t *fh_scan_cells(const scan_t *s, int large_grid_sp, int *n_out) {
  int n = 0, cap = 1024, chm = 0, pos;
  fsclg_cell_t *cells = fh_malloc(sizeof(fsclg_cell_t) * cap, "cells");
  if (s->n_chromosomes > 0) {
    pos = s->chr_limits[0].start_pos;
    for (;;) {
      if (pos >= s->chr_limits[chm].bp_length) {
        if (++chm == s->n_chromosomes) break;
        pos = s->chr_limits[chm].start_pos;
      }
      if (n == cap) cells = fh_realloc(cells, sizeof(fsclg_cell_t) * (cap *= 2), "cells");
      cells[n].chr = chm;
      cells[n].start_pos = pos;
      cells[n].end_pos = pos + large_grid_sp > s->chr_limits[chm].bp_length ? s->chr_limits[chm].bp_length
                                                                             : pos + large_grid_sp;
      cells[n].pad = 0;
      n++;
      pos += large_grid_sp;
    }
  }
  *n_out = n;
  return cells;
}

/* scan-chromosome.c:228-265 */
void scan_chromosome(scan_t *s, sm_ptable_t *sm, int eval_range, int bp_resl, int large_grid_sp, int n_threads) {
  fsclg_cell_t *cells;
  fsclg_point_t *out;
  keyed_pt_t *kp;
  int n = 0, i;
  double t0 = fh_now();
  (void)n_threads; /* the GPUs evaluate every cell concurrently */
  fh_prepare(s, sm);
  cells = fh_scan_cells(s, large_grid_sp, &n);
  fh_set_original_rows();
  out = fh_malloc(sizeof(fsclg_point_t) * (n ? n : 1), "points");
  fh_eval_cells(cells, n, eval_range, bp_resl, out);
  kp = fh_malloc(sizeof(keyed_pt_t) * (n ? n : 1), "points");
  for (i = 0; i < n; i++) { fh_to_scan_pt(&kp[i].p, out + i); kp[i].seq = i; }
  qsort(kp, n, sizeof(keyed_pt_t), pt_cmp);
  if (s->scan_pts)
    for (i = 0; i < s->n_scan_pts; i++) free(s->scan_pts[i].permute_clr);
  free(s->scan_pts);
  s->scan_pts = fh_malloc(sizeof(scan_pt_t) * (n ? n : 1), "scan points");
  for (i = 0; i < n; i++) { /* scan-chromosome.c:239-241: a null-distribution buffer per point */
    s->scan_pts[i] = kp[i].p;
    s->scan_pts[i].permute_clr = fh_malloc(sizeof(float) * CLR_NULL_DIST_SAVE, "permute_clr");
  }
  s->n_scan_pts = n;
  free(kp); free(out); free(cells);
  D.st.scan_s += fh_now() - t0;
  logmsg(MSG_STATUS, "\nInitial scan finished.\n");
}

/* --------------------------------------------------- search_maxalpha drop-in
   sm-search.c:269-300 for one caller-initialised point.  The reference calls it once per
   point from its own scan loop (scan-chromosome.c:126-135), so the drop-in keeps a context
   of its own on the first device, with state that survives between calls:
     * the tables, keyed by the sm_ptable_t pointer, the depths in use and a hash of the
       coefficients (every row of those depths on the device; a row's null_logl, known only
       from the sites, is added when a window first shows it);
     * the sites of the last window uploaded, as (position, row) pairs: the next call reuses
       them when its window lies inside and its sites compare equal (the caller's scan
       loop evaluates many points of one window; a permuted array differs and is uploaded).
   The scan path's own contexts are not touched. */
static struct {
  fsclg_ctx *ctx;
  const sm_ptable_t *sm;
  int n_depths;
  uint64_t tab_hash;
  fh_rowmap_t rm;
  double *null_full;       /* [rm.n_rows] null_logl of each row, as seen so far */
  unsigned char *null_seen;
  int32_t *pos;            /* uploaded window [lo, lo + n) */
  uint32_t *row;
  int lo, n, cap;
  int32_t *tpos;
  uint32_t *trow;
  int tcap;
} DI;

/* the first and last coefficient blocks of every row (tables are built once and never
   changed by the reference; this catches a caller that rebuilds them in place) */
uint64_t fh_tables_hash(const sm_ptable_t *sm, int n_depths) {
  uint64_t h = 88172645463325252ull;
  int d, i;
  for (d = 0; d < n_depths; d++) {
    const int n = sm[d].sample_size;
    h = fh_hash_words(&n, sizeof n, h);
    for (i = 0; i <= n + n / 2 + 1; i++) {
      const spline_t *sp = i <= n ? sm[d].spline_func[i] : sm[d].fspline_func[i - n - 1];
      h = fh_hash_words(sp->coef[0], sizeof(double) * 4, h);
      h = fh_hash_words(sp->coef[sp->n - 1], sizeof(double) * 4, h);
    }
  }
  return h;
}

/* every row of depths [0, n_depths) on the drop-in context; the null values known so far
   (rows of earlier depths keep their numbers when depths are added) plus this window's */
static void dropin_tables(const sm_ptable_t *sm, int n_depths, const snp_t *snps, int ws, int n, int keep) {
  int *dn = fh_malloc(sizeof(int) * n_depths, "depths"), *idx = fh_malloc(sizeof(int) * (n ? n : 1), "window");
  const int n_known = keep ? DI.rm.n_rows : 0;
  unsigned char *seen;
  double *coef, *nullrow;
  int d, i;
  for (d = 0; d < n_depths; d++) dn[d] = sm[d].sample_size;
  for (i = 0; i < n; i++) idx[i] = ws + i;
  coef = flatten_tables(&DI.rm, sm, n_depths, dn, snps, idx, n, 1, &nullrow, DI.null_full, n_known);
  seen = fh_calloc(DI.rm.n_rows, 1, "null rows");
  if (n_known) memcpy(seen, DI.null_seen, (size_t)(n_known < DI.rm.n_rows ? n_known : DI.rm.n_rows));
  for (i = 0; i < n; i++) seen[fh_full_row(&DI.rm, snps + ws + i)] = 1;
  free(DI.null_full); free(DI.null_seen);
  DI.null_full = nullrow;  /* every row: device row = row */
  DI.null_seen = seen;
  upload_flat(&DI.ctx, 1, &DI.rm, coef, nullrow);
  free(coef); free(dn); free(idx);
  DI.n = 0;  /* the tables were replaced: the sites go up again */
}

static void search_maxalpha_locked(scan_pt_t *pt, snp_t *snps, sm_ptable_t *sm) {
  const int ws = pt->window_start, we = pt->window_end, n = we - ws + 1;
  int i, maxd = 0, need_tables, reuse;
  fsclg_point_t p;
  init_log_table();
  fh_dev_open();
  if (!DI.ctx) fh_dev_check(fsclg_open(D.dev[0], &DI.ctx), "open the search_maxalpha context");
  if (n <= 0) logmsg(MSG_FATAL, "fscl_amd: search_maxalpha: empty window");
  for (i = ws; i <= we; i++) if (snps[i].depth_p > maxd) maxd = snps[i].depth_p;
  need_tables = DI.sm != sm || DI.n_depths < maxd + 1 || fh_tables_hash(sm, DI.n_depths) != DI.tab_hash;
  if (!need_tables) /* a row class this window shows for the first time: its null value */
    for (i = ws; i <= we && !need_tables; i++) {
      const uint32_t r = fh_full_row(&DI.rm, snps + i);
      if (!DI.null_seen[r]) need_tables = 1;
      else if (memcmp(&DI.null_full[r], &snps[i].null_logl, sizeof(double)) != 0)
        logmsg(MSG_FATAL, "fscl_amd: null_logl differs between sites of the same class (call "
                          "compute_snp_null_model first)");
    }
  if (need_tables) {
    const int same = DI.sm == sm && DI.null_full != NULL;
    const int nd = !same || maxd + 1 > DI.n_depths ? maxd + 1 : DI.n_depths;
    dropin_tables(sm, nd, snps, ws, n, same);
    DI.sm = sm; DI.n_depths = nd; DI.tab_hash = fh_tables_hash(sm, nd);
  }
  /* the window's sites as the device holds them */
  if (DI.tcap < n) {
    DI.tcap = n;
    DI.tpos = fh_realloc(DI.tpos, sizeof(int32_t) * n, "window");
    DI.trow = fh_realloc(DI.trow, sizeof(uint32_t) * n, "window");
  }
  for (i = 0; i < n; i++) { DI.tpos[i] = snps[ws + i].pos; DI.trow[i] = fh_row_of(&DI.rm, snps + ws + i); }
  reuse = DI.n > 0 && ws >= DI.lo && we < DI.lo + DI.n &&
          !memcmp(DI.pos + (ws - DI.lo), DI.tpos, sizeof(int32_t) * n) &&
          !memcmp(DI.row + (ws - DI.lo), DI.trow, sizeof(uint32_t) * n);
  if (!reuse) {
    int32_t cs = 0, cn = n;
    if (DI.cap < n) {
      DI.cap = n;
      DI.pos = fh_realloc(DI.pos, sizeof(int32_t) * n, "window");
      DI.row = fh_realloc(DI.row, sizeof(uint32_t) * n, "window");
    }
    memcpy(DI.pos, DI.tpos, sizeof(int32_t) * n);
    memcpy(DI.row, DI.trow, sizeof(uint32_t) * n);
    DI.lo = ws; DI.n = n;
    fh_dev_check(fsclg_upload_snps(DI.ctx, DI.pos, DI.row, n, &cs, &cn, 1), "upload window");
  }
  memset(&p, 0, sizeof p);
  p.chr = 0; p.nearest_snp = pt->nearest_snp - DI.lo; p.sweep_pos = pt->sweep_pos; p.n_snps = pt->n_snps;
  p.window_start = ws - DI.lo; p.window_end = we - DI.lo; p.null_logl = pt->null_logl;
  fh_dev_check(fsclg_search_points(DI.ctx, &p, 1), "search_maxalpha");
  pt->lalpha = p.lalpha; pt->sm_logl = p.sm_logl; pt->clr = p.clr;
}

/* the reference calls search_maxalpha from its --n-threads workers (scan-chromosome.c:258,
   514, 531): the drop-in's state (DI: context, tables, the resident window) is shared, so
   calls are serialised; each is one short device launch */
static pthread_mutex_t g_dropin_mu = PTHREAD_MUTEX_INITIALIZER;

void search_maxalpha(scan_pt_t *pt, snp_t *snps, sm_ptable_t *sm) {
  pthread_mutex_lock(&g_dropin_mu);
  search_maxalpha_locked(pt, snps, sm);
  pthread_mutex_unlock(&g_dropin_mu);
}

/* ------------------------------------------------------ grid-maximum scan and test
   The statistic of the reference's disabled fine-grid loops (scan-chromosome.c:269-296 the
   scan, :505-523 the trial): a cell's point is the first position of strictly greatest clr
   among its grid positions -- start + j * small_grid_sp with start <= pos <= end (the clipped
   end; the start shared with the lower cell included; the end appended when the step misses
   it), fscl_amd_profile_grid's positions of the cell.  One run per cell, or two for a
   chromosome's last cell, evaluated by fsclg_cellmax_submit on the rows a slot holds. */
static int cell_runs(const fsclg_cell_t *c, int g, fsclg_run_t *r) {
  const int span = c->end_pos - c->start_pos;
  r[0].chr = c->chr; r[0].start_pos = c->start_pos; r[0].step = g; r[0].count = span / g + 1;
  if (span % g == 0) return 1;
  r[1].chr = c->chr; r[1].start_pos = c->end_pos; r[1].step = g; r[1].count = 1;
  return 2;
}

static double g_cellmax_ms;
double fscl_amd_cellmax_last_ms(void) { return g_cellmax_ms; }

/* the grid maxima of n cells on the rows of `slot`: the local devices take contiguous shares
   of the cells balanced by window size x positions, every device is submitted to before the
   first is waited for; out[i] is cell i's maximum */
void fh_eval_cell_maxima(int slot, const fsclg_cell_t *cells, int n, int g, int eval_range, fsclg_point_t *out) {
  fsclg_run_t *runs = fh_malloc(sizeof(fsclg_run_t) * 2 * (size_t)(n ? n : 1), "grid runs");
  fsclg_point_t *ro = fh_malloc(sizeof(fsclg_point_t) * 2 * (size_t)(n ? n : 1), "grid points");
  int *first = fh_malloc(sizeof(int) * ((size_t)n + 1), "grid runs"); /* cell i's runs: [first[i], first[i + 1]) */
  double *cost = fh_malloc(sizeof(double) * (n ? n : 1), "cost");
  int lo[FH_MAX_DEV], hi[FH_MAX_DEV], l, i, nr = 0;
  for (i = 0; i < n; i++) {
    int k, np = 0;
    first[i] = nr;
    nr += cell_runs(cells + i, g, runs + nr);
    for (k = first[i]; k < nr; k++) np += runs[k].count;
    cost[i] = fh_window_cost(cells[i].chr, eval_range) * np;
    D.st.gp_evals += (unsigned long long)np;
  }
  first[n] = nr;
  fh_dev_shares(cost, n, lo, hi);
  g_cellmax_ms = 0.;
  for (l = 0; l < D.n_dev; l++) {
    DBG("cell maxima: device %d, cells [%d, %d)\n", D.dev[l], lo[l], hi[l]);
    fh_dev_check(fsclg_cellmax_submit(D.ctx[l], 0, slot, runs + first[lo[l]], first[hi[l]] - first[lo[l]], eval_range),
              "cell maxima submit");
  }
  for (l = 0; l < D.n_dev; l++) {
    double ms;
    fh_dev_check(fsclg_cellmax_wait(D.ctx[l], 0, ro + first[lo[l]]), "cell maxima wait");
    ms = fsclg_cellmax_last_ms(D.ctx[l], 0);
    if (ms > g_cellmax_ms) g_cellmax_ms = ms; /* the devices run side by side */
  }
  for (i = 0; i < n; i++) { /* a last cell's appended end: after its run, the same strict > */
    out[i] = ro[first[i]];
    if (first[i + 1] - first[i] == 2 && ro[first[i] + 1].clr > out[i].clr) out[i] = ro[first[i] + 1];
  }
  free(runs); free(ro); free(first); free(cost);
}

/* the test handle of fsclg_cellmax_submit / fsclg_cellmax_wait on the first device: the runs'
   maxima on the uploaded rows (rows NULL: slot 0, batch 0) or on `rows` (n_snps device rows, set
   into slot 1 with their whole-chromosome null sums; batch 1) */
int fscl_amd_cellmax_runs(scan_t *s, sm_ptable_t *sm, const fsclg_run_t *runs, int n_runs, int eval_range,
                          const uint32_t *rows, fsclg_point_t *out) {
  int slot, r = fh_runs_handle_begin(s, sm, runs, n_runs, rows, &slot);
  if (r != FSCLG_OK) return r;
  g_cellmax_ms = 0.;
  r = fsclg_cellmax_submit(D.ctx[0], slot, slot, runs, n_runs, eval_range);
  if (r != FSCLG_OK) return r;
  r = fsclg_cellmax_wait(D.ctx[0], slot, out);
  g_cellmax_ms = fsclg_cellmax_last_ms(D.ctx[0], slot);
  return r;
}

/* the device row of every site, as uploaded (n_snps values): what a permutation of the sites
   rearranges (fscl_amd_cellmax_runs' rows) */
int fscl_amd_site_rows(scan_t *s, sm_ptable_t *sm, uint32_t *out) {
  if (!s || !sm || !out) return -1;
  fh_prepare(s, sm);
  memcpy(out, D.row, sizeof(uint32_t) * (size_t)s->n_snps);
  return s->n_snps;
}

/* the points fscl_amd_scan_chromosome_grid made last: fscl_amd_scan_permute_grid tests only
   those, with the same spacings, on the same data (D.key) */
static struct {
  const scan_pt_t *pts;
  int n, g, G;
  uint64_t key, pkey;
} GS;

/* the points' content, chr .. clr (a freed and re-allocated point array may reuse its address) */
static uint64_t points_hash(const scan_t *s) {
  uint64_t h = 1469598103934665603ull;
  int i;
  for (i = 0; i < s->n_scan_pts; i++)
    h = fh_hash_words(s->scan_pts + i, offsetof(scan_pt_t, clr) + sizeof(double), h);
  return h;
}

int fh_grid_points_are(const scan_t *s, int small_grid_sp, int large_grid_sp) {
  return s->scan_pts && s->scan_pts == GS.pts && s->n_scan_pts == GS.n && small_grid_sp == GS.g &&
         large_grid_sp == GS.G && D.key == GS.key && points_hash(s) == GS.pkey;
}

void fscl_amd_scan_chromosome_grid(scan_t *s, sm_ptable_t *sm, int eval_range, int small_grid_sp, int large_grid_sp) {
  fsclg_cell_t *cells;
  fsclg_point_t *out;
  int n = 0, i;
  double t0 = fh_now();
  if (small_grid_sp < 1 || large_grid_sp < 1 || large_grid_sp % small_grid_sp != 0)
    logmsg(MSG_FATAL, "fscl_amd: grid scan: fine grid spacing %d must be positive and divide the coarse grid spacing %d",
           small_grid_sp, large_grid_sp);
  if (D.world > 1) logmsg(MSG_FATAL, "fscl_amd: the grid scan mode runs in one process (not with %d ranks)", D.world);
  fh_prepare(s, sm);
  cells = fh_scan_cells(s, large_grid_sp, &n);
  fh_set_original_rows();
  out = fh_malloc(sizeof(fsclg_point_t) * (n ? n : 1), "points");
  fh_eval_cell_maxima(0, cells, n, small_grid_sp, eval_range, out);
  if (s->scan_pts)
    for (i = 0; i < s->n_scan_pts; i++) free(s->scan_pts[i].permute_clr);
  free(s->scan_pts);
  s->scan_pts = fh_malloc(sizeof(scan_pt_t) * (n ? n : 1), "scan points");
  for (i = 0; i < n; i++) { /* cell order is (chromosome, position) order: no sort */
    fh_to_scan_pt(s->scan_pts + i, out + i);
    s->scan_pts[i].permute_clr = fh_malloc(sizeof(float) * CLR_NULL_DIST_SAVE, "permute_clr");
  }
  s->n_scan_pts = n;
  GS.pts = s->scan_pts; GS.n = n; GS.g = small_grid_sp; GS.G = large_grid_sp; GS.key = D.key;
  GS.pkey = points_hash(s);
  free(out); free(cells);
  D.st.scan_s += fh_now() - t0;
  logmsg(MSG_STATUS, "\nInitial scan finished (grid maxima at %d bp).\n", small_grid_sp);
}

/* ---------------------------------------------------------------- output */
void scan_output(char *fname, scan_t *s, int maximum_only, int n_perm, char *label) {
  FILE *f = stdout;
  const scan_pt_t *best;
  double max_clr;
  char pos_str[64];
  int i;
  if (D.world > 1 && D.rank != 0) return; /* one writer */
  if (fname) {
    f = fopen(fname, "w");
    if (!f) { fprintf(stderr, "Can't open output file \"%s\" (%s)", fname, strerror(errno)); return; }
  }
  if (s->n_scan_pts == 0) { if (fname) fclose(f); return; }
  best = s->scan_pts;
  max_clr = s->scan_pts[0].clr;
  for (i = 1; i < s->n_scan_pts; i++)
    if (s->scan_pts[i].clr > max_clr) { max_clr = s->scan_pts[i].clr; best = s->scan_pts + i; }
  if (best->sweep_pos > 1000000)
    snprintf(pos_str, sizeof pos_str, "chromosome %s %1.2f Mb", s->chr_limits[best->chr].name, best->sweep_pos / 1e6);
  else if (best->sweep_pos > 2000)
    snprintf(pos_str, sizeof pos_str, "chromosome %s %1.2f Kb", s->chr_limits[best->chr].name, best->sweep_pos / 1e3);
  else
    snprintf(pos_str, sizeof pos_str, "chromosome %s %d bp", s->chr_limits[best->chr].name, best->sweep_pos);
  logmsg(MSG_STATUS, "\rOutput complete -- maximum CLR of %g at %s (alpha = %g)\n", max_clr, pos_str,
         exp(best->lalpha));
  if (maximum_only) {
    if (label) fprintf(f, "%s\t", label);
    fprintf(f, "%s\t%d\t%1.2f\t%1.3e\t%d\t%d\t%d\n", s->chr_limits[best->chr].name, best->sweep_pos, max_clr,
            exp(best->lalpha), best->n_snps, s->snps[best->window_start].pos, s->snps[best->window_end].pos);
    if (fname) fclose(f); /* the reference leaks the handle here (scan-chromosome.c:715) */
    return;
  }
  for (i = 0; i < s->n_scan_pts; i++) {
    const scan_pt_t *q = s->scan_pts + i;
    if (label) fprintf(f, "%s\t", label);
    if (n_perm > 0) {
      /* Q8: an empirical ratio, no chi-square projection */
      const double pv = q->permute_p < 2 ? 1.0 / q->permute_n : (q->permute_p - 1.0) / (double)(q->permute_n - 1.0);
      fprintf(f, "%s\t%d\t%1.2f\t%1.3e\t%d\t%d\t%1.3f\n", s->chr_limits[q->chr].name, q->sweep_pos, q->clr,
              exp(q->lalpha), q->permute_p, q->permute_n, -log10(pv));
    } else {
      fprintf(f, "%s\t%d\t%1.2f\t%1.3e\t%d\t%d\t%d\n", s->chr_limits[q->chr].name, q->sweep_pos, q->clr,
              exp(q->lalpha), q->n_snps, s->snps[q->window_start].pos, s->snps[q->window_end].pos);
    }
  }
  if (fname) fclose(f);
}

static int float_cmp(const void *a, const void *b) {
  const float x = *(const float *)a, y = *(const float *)b;
  return (x > y) - (x < y);
}

/* scan-chromosome.c:753-796 */
void fh_output_clr_null_distribution(const char *fname, scan_t *s) {
  char *fn = fh_malloc(strlen(fname) + 20, "fname");
  FILE *f;
  int i, j;
  sprintf(fn, "%s-nulldist", fname);
  f = fopen(fn, "w");
  free(fn);
  if (!f) { fprintf(stderr, "Can't open output file for CLR null distribution (%s)\n", strerror(errno)); return; }
  fprintf(f, "chr\tpos\tCLR\talpha\tp\tn");
  for (j = 0; j < CLR_NULL_DIST_SAVE; j++) fprintf(f, "\t%1.4f", j / (double)CLR_NULL_DIST_SAVE);
  fprintf(f, "\n");
  for (i = 0; i < s->n_scan_pts; i++) {
    scan_pt_t *q = s->scan_pts + i;
    const int np = q->permute_n < CLR_NULL_DIST_SAVE ? q->permute_n : CLR_NULL_DIST_SAVE;
    if (q->permute_clr) qsort(q->permute_clr, np, sizeof(float), float_cmp);
    fprintf(f, "%s\t%d\t%1.3f\t%1.3e\t%d\t%d", s->chr_limits[q->chr].name, q->sweep_pos, q->clr, exp(q->lalpha),
            q->permute_p, q->permute_n);
    for (j = 0; j < np && q->permute_clr; j++) fprintf(f, "\t%1.2f", (double)q->permute_clr[j]);
    fprintf(f, "\n");
  }
  fclose(f);
}

/* ----------------------------------------------------------------- stats */
/* this process's counters; device counters summed over its devices (busy_ms: the sum of
   each device's busy time, i.e. device-seconds) */
void fscl_amd_get_stats(fscl_amd_stats_t *st) {
  int l;
  *st = D.st;
  st->kernel_ms = 0; st->n_terms = st->n_null = st->n_walks = st->n_maxalpha = 0;
  st->n_unsafe = st->n_slow = st->n_ties = st->n_launches = 0;
  st->window_ms = 0; st->n_dup_cells = st->n_ep_saved = 0; st->busy_ms = 0; st->n_split_retry = 0;
  for (l = 0; l < D.n_dev; l++) {
    fsclg_stats_t g;
    if (fsclg_get_stats(D.ctx[l], &g) != FSCLG_OK) continue;
    st->kernel_ms += g.kernel_ms;
    st->n_terms += g.n_terms; st->n_null += g.n_null; st->n_walks += g.n_walks; st->n_maxalpha += g.n_maxalpha;
    st->n_unsafe += g.n_unsafe; st->n_slow += g.n_slow; st->n_ties += g.n_ties; st->n_launches += g.n_launches;
    st->window_ms += g.window_ms;
    st->n_dup_cells += g.n_dup_cells; st->n_ep_saved += g.n_ep_saved;
    st->busy_ms += g.busy_ms;
    st->n_split_retry += g.n_split_retry;
    if (l == 0) {
      st->cache_iv0 = g.cache_iv0; st->cache_n_iv = g.cache_n_iv; st->cache_n_rows = g.cache_n_rows;
      st->cache_cover = g.cache_cover;
    }
  }
  if (DI.ctx) {  /* the drop-in search_maxalpha's own context */
    fsclg_stats_t g;
    if (fsclg_get_stats(DI.ctx, &g) == FSCLG_OK) {
      st->kernel_ms += g.kernel_ms;
      st->n_terms += g.n_terms; st->n_walks += g.n_walks; st->n_maxalpha += g.n_maxalpha;
      st->n_launches += g.n_launches;
      st->busy_ms += g.busy_ms;
    }
  }
  st->n_devices = D.n_dev;
}

void fscl_amd_reset_stats(void) {
  int l;
  memset(&D.st, 0, sizeof D.st);
  for (l = 0; l < D.n_dev; l++) fsclg_reset_stats(D.ctx[l]);
  if (DI.ctx) fsclg_reset_stats(DI.ctx);
}

void fscl_amd_shutdown(void) {
  fh_pool_drop();
  fh_spec_stop();
  dev_close_all();
  if (DI.ctx) fsclg_close(DI.ctx);
  free(DI.null_full); free(DI.null_seen); free(DI.pos); free(DI.row); free(DI.tpos); free(DI.trow);
  free_rowmap(&DI.rm);
  memset(&DI, 0, sizeof DI);
  free(D.row); free(D.pos); free(D.chr_start); free(D.chr_n); free(D.nullrow); free(D.rowp);
  D.rowp = NULL;
  D.row = NULL; D.pos = NULL; D.chr_start = NULL; D.chr_n = NULL; D.nullrow = NULL;
  free_rowmap(&D.rm);
  if (D.sim) { fclose(D.sim); D.sim = NULL; }
}
