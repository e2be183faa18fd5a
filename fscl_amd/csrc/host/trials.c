/* trials.c -- everything that permutes rows: the block-permutation tests of scan.c's scans
 * (scan_permute: pipelined with speculation, lockstep, throughput mode; the grid permutation test)
 * and the unpruned family-wise pass.  scan_internal.h declares what it takes from scan.c.
 */
#define _GNU_SOURCE
#include <limits.h>
#include <math.h>
#include <pthread.h>
#include <sched.h>
#include <signal.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <unistd.h>

#include <omp.h>

#include "scan_internal.h"

/* OpenMP threads of the main thread's whole-chromosome null sums (a speculation miss): with the
   node leader's permutations the other ranks' main threads hold W - 1 of the usable CPUs, and
   an OpenMP team larger than what is left spins in its barriers */
static int g_null_nt = 0;
int fh_null_threads(void) { return g_null_nt > 0 ? g_null_nt : omp_get_max_threads(); }

/* The block permutation's geometry (perm.c: the 1 Mb extension's end of every site, for the
   scan's sites and scan_width_mb) and the device plan mode: when no trial reads
   a whole-chromosome null sum -- every chromosome longer than its window, C5 -- the host needs
   no permuted rows, and each trial's permutation goes to the devices as its plan
   (fsclg_slot_set_rows_plan): ~16 B per block instead of rb bytes per site, and the host's part
   is drawing the blocks (~50 ns each) instead of an O(n) copy and swap pass. */
typedef struct { int32_t n_ent, n_grp, ok, pad; } plan_hdr_t;
static struct {
  int32_t *ext;        /* fh_ext_table of D's sites for ext_width */
  double ext_width;
  int ext_n;
  uint64_t ext_key;    /* D.key (the sites' content hash) the table was built for */
  fh_perm_geom_t G;
  int on;              /* plan mode in the current permute_pipelined call */
  int ecap, gcap;      /* a plan buffer's capacity: entries, groups */
  size_t bytes;        /* a plan buffer's size */
} PM;

static void perm_geom(double width_mb) {
  if (!PM.ext || PM.ext_n != D.n_snps_key || PM.ext_width != width_mb || PM.ext_key != D.key) {
    free(PM.ext);
    PM.ext = fh_malloc(sizeof(int32_t) * (size_t)(D.n_snps_key ? D.n_snps_key : 1), "extension table");
    fh_ext_table(PM.ext, D.pos, D.chr_start, D.chr_n, D.n_chr, width_mb);
    PM.ext_n = D.n_snps_key; PM.ext_width = width_mb; PM.ext_key = D.key;
  }
  PM.G.n = D.n_snps_key; PM.G.n_chr = D.n_chr; PM.G.chr_start = D.chr_start; PM.G.chr_n = D.chr_n;
  PM.G.pos = D.pos; PM.G.ext = PM.ext;
}

static int32_t *plan_grp(void *buf) { return (int32_t *)((char *)buf + sizeof(plan_hdr_t)); }
static fsclg_swap_t *plan_ent(void *buf) {
  return (fsclg_swap_t *)((char *)buf + sizeof(plan_hdr_t) + ((sizeof(int32_t) * (size_t)(PM.gcap + 1) + 15) & ~(size_t)15));
}

/* one trial's plan into a plan buffer from rand() state *g (advanced); 0, -1 cancelled, -2 it did
   not fit (hdr->ok = 0: the trial's rows are built on the host instead) */
static int plan_into(void *buf, fh_plan_t *P, double nbp, double width_mb, fh_rand_t *g, unsigned long long *negj,
                     const volatile unsigned *gen, unsigned my_gen) {
  plan_hdr_t *h = buf;
  const int r = fh_plan_build(P, &PM.G, nbp, width_mb, g, negj, plan_ent(buf), PM.ecap, plan_grp(buf), PM.gcap,
                              &h->n_ent, &h->n_grp, gen, my_gen);
  h->ok = r == 0;
  return r;
}

/* block_permute and chr_null_sums_1t at each staging width: rows_impl.h (scan-chromosome.c:336-389, 92-94), and
   their dispatch on D.rb */
#define ROW_TRIALS
#include "rows_impl.h"

static int block_permute(void *prow, const void *row, int n, double nbp, double width_mb, fh_rand_t *g,
                         unsigned long long *negj, const volatile unsigned *gen, unsigned my_gen) {
  if (D.rb == 1) return block_permute_8(prow, row, n, nbp, width_mb, g, negj, gen, my_gen);
  if (D.rb == 2) return block_permute_16(prow, row, n, nbp, width_mb, g, negj, gen, my_gen);
  return block_permute_32(prow, row, n, nbp, width_mb, g, negj, gen, my_gen);
}

static int chr_null_sums_1t(const void *row, double *out, const volatile unsigned *gen, unsigned my_gen) {
  if (D.rb == 1) return chr_null_sums_1t_8(row, out, gen, my_gen);
  if (D.rb == 2) return chr_null_sums_1t_16(row, out, gen, my_gen);
  return chr_null_sums_1t_32(row, out, gen, my_gen);
}

/* ------------------------------------------------------------ permutation */

/* one trial's rows (in D.stage[slot]) and null sums to the slot on every local device;
   waits until the slot's previous upload has read the staging before it is rewritten */
static void *slot_stage(int slot) {
  int l;
  for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_slot_wait(D.ctx[l], slot), "slot wait");
  return D.stage[slot];
}

static void slot_upload_buf(int slot, const void *rows, const double *nul) {
  int l;
  for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_slot_set_rows_packed(D.ctx[l], slot, rows, D.rb, nul), "set rows");
}

static void slot_upload(int slot, const double *nul) { slot_upload_buf(slot, D.stage[slot], nul); }

/* plan mode: the trial's plan (a plan buffer) to the slot on every local device */
static void slot_upload_plan(int slot, void *buf, const double *nul) {
  const plan_hdr_t *h = buf;
  int l;
  for (l = 0; l < D.n_dev; l++)
    fh_dev_check(fsclg_slot_set_rows_plan(D.ctx[l], slot, plan_ent(buf), plan_grp(buf), h->n_grp, nul), "set rows (plan)");
}

static volatile sig_atomic_t g_sigint = 0;
static struct timeval g_last_dump;
static double g_sigint_window = 10.;  /* seconds; FSCL_AMD_SIGINT_WINDOW_MS (tests) shortens it */
static void on_sigint(int sig) { /* scan-chromosome.c:557-569 */
  struct timeval now;
  (void)sig;
  gettimeofday(&now, NULL);
  if ((now.tv_sec - g_last_dump.tv_sec) + (now.tv_usec - g_last_dump.tv_usec) / 1e6 < g_sigint_window) {
    static const char msg[] = "\nanother interrupt signal received, aborting permutation\n";
    if (write(2, msg, sizeof msg - 1) < 0) {}
    _exit(255);
  }
  g_sigint = 1;
}

/* whether to dump now: with several ranks the dump is collective -- every rank drains its
   bulk batches and dumps at the same trial, so they keep making the same exchanges.  Each
   rank's flag goes into one exchange made at the same point of every trial (round); all ranks
   act on the OR.  A signal that arrives after this trial's exchange counts at the next. */
static int sigint_agreed(void) {
  unsigned f = g_sigint ? 1u : 0u;
  if (D.world <= 1 || D.sim) return (int)f;
  if (D.shm) {
    char dummy = 0;
    if (fh_shm_allgather_flags(D.shm, &dummy, 1, 0, 0, 0, &f) != 0) logmsg(MSG_FATAL, "fscl_amd: rank exchange failed");
    return f != 0;
  }
  {
    long long v = f;
    if (D.xfn(&v, 1, D.xctx) != 0) logmsg(MSG_FATAL, "fscl_amd: rank exchange failed");
    return v != 0;
  }
}

/* scan-chromosome.c:553-560, taken between trials: the current table and null distributions
   (one writer: rank 0); every rank restarts its 10-second window, so a second interrupt
   ends all ranks alike */
static void sigint_dump(scan_t *s, int n_perm) {
  const char *fn, *lb;
  fh_dump_target(&fn, &lb);
  g_sigint = 0;
  if (D.rank == 0) {
    scan_output((char *)fn, s, 0, n_perm, (char *)lb);
    if (fn) fh_output_clr_null_distribution(fn, s);
  }
  gettimeofday(&g_last_dump, NULL);
}

/* ------------------------------------------------ speculative permutations
   (SURVEY §8(f) row 1).  The reference builds each trial's permutation serially from the
   rand() stream after the previous trial's prune draws (scan-chromosome.c:441-456, 488-498),
   and so does this host: trial t+1's permutation starts at the state S left by trial t's own
   permutation, advanced by d_t draws -- one per hit of a point whose permute_p is already
   >= 19.  d_t is known only when trial t's results are in, but its distribution is
   predictable from those points' hit rates.  So while the GPUs evaluate trial t, worker
   threads build the permutations (and whole-chromosome null sums) for the most likely d_t,
   each from its own copy of S; when d_t is known the matching candidate is taken (its end
   state becomes the stream's) and the others are cancelled; a miss builds it on the main
   thread as before.  The stream, and so every result, is unchanged.  Before any point can
   draw (the first 19 trials) d_t = 0 is certain: one candidate, never a miss. */
#define SPEC_MAX 32
#define PB_FREE (-1)
#define PB_CAND (-2)
#define PB_HELD (-3)
#define PB_PRE (-4)   /* a candidate a spare device slot is being prepared from (pre-staging) */

typedef struct {
  void *buf;       /* one trial's rows (D.rb bytes each), pinned: every local device's upload reads it */
  double *nul;     /* its whole-chromosome null sums */
  int owner;       /* the row slot whose upload reads it, or PB_FREE / PB_CAND / PB_HELD */
} pbuf_t;

static struct {
  pthread_t th[SPEC_MAX];
  int n_th;
  pthread_mutex_t mu;
  pthread_cond_t cv, done;
  volatile unsigned gen;  /* bumped to cancel the posted candidates */
  int stop;
  fh_rand_t base;         /* the posted job: S, and the draw counts to build */
  int n_job, next, running;
  int n_keep;             /* workers with an index >= n_keep exit (spec_start shrinking the team) */
  int d[SPEC_MAX], bi[SPEC_MAX], state[SPEC_MAX];  /* 0 queued, 1 running, 2 done, 3 cancelled */
  fh_rand_t end[SPEC_MAX];
  unsigned long long negj[SPEC_MAX];
  const snp_t *snps;      /* the permutation's inputs (fixed while a job is posted) */
  int n;
  double nbp, width_mb;
  pbuf_t pb[FSCLG_N_SLOTS + 3 * SPEC_MAX + 1];
  int n_pb, pb_cap, pb_nchr, pb_rb;
  size_t pb_bytes;        /* one buffer: a trial's rows (rb bytes per site) or, in plan mode, its plan */
  fh_plan_t plan[SPEC_MAX + 1];  /* each worker's plan scratch; [SPEC_MAX]: the main thread's */
  int pb_in_pool;         /* the buffers are the leader's pool's (not owned here) */
} SP = {.mu = PTHREAD_MUTEX_INITIALIZER, .cv = PTHREAD_COND_INITIALIZER, .done = PTHREAD_COND_INITIALIZER,
        .n_keep = SPEC_MAX};

static void *spec_worker(void *arg) {
  const int w = (int)(intptr_t)arg;
  pthread_mutex_lock(&SP.mu);
  for (;;) {
    while (!SP.stop && w < SP.n_keep && SP.next >= SP.n_job) pthread_cond_wait(&SP.cv, &SP.mu);
    if (SP.stop || w >= SP.n_keep) break;
    {
      const int c = SP.next++;
      const unsigned my = SP.gen;
      const int d = SP.d[c];
      pbuf_t *b = SP.pb + SP.bi[c];
      fh_rand_t r = SP.base;
      unsigned long long negj = 0;
      int t, ok;
      SP.state[c] = 1;
      SP.running++;
      pthread_mutex_unlock(&SP.mu);
      const double t0 = fh_now();
      for (t = 0; t < d; t++) (void)fh_rand(&r);
      if (PM.on) { /* the plan only (no whole-chromosome null sums are read in plan mode) */
        ok = plan_into(b->buf, SP.plan + w, SP.nbp, SP.width_mb, &r, &negj, &SP.gen, my) == 0;
        memset(b->nul, 0, sizeof(double) * (size_t)(D.n_chr ? D.n_chr : 1));
      } else
        ok = block_permute(b->buf, D.rowp, SP.n, SP.nbp, SP.width_mb, &r, &negj, &SP.gen, my) == 0 &&
             chr_null_sums_1t(b->buf, b->nul, &SP.gen, my) == 0;
      pthread_mutex_lock(&SP.mu);
      SP.running--;
      if (ok && SP.gen == my) {
        SP.state[c] = 2; SP.end[c] = r; SP.negj[c] = negj;
        D.st.spec_gen_s += fh_now() - t0;
        D.st.spec_done++;
      }
      else { /* cancelled: its buffer is free again (index c may already belong to a newer job) */
        if (SP.gen == my) SP.state[c] = 3;
        b->owner = PB_FREE;
      }
      pthread_cond_broadcast(&SP.done);
    }
  }
  pthread_mutex_unlock(&SP.mu);
  return NULL;
}

/* CPUs this process may use (affinity, capped by the cgroup v2 quota) */
static int usable_cpus(void) {
  cpu_set_t cs;
  int n = 1;
  FILE *f;
  if (sched_getaffinity(0, sizeof cs, &cs) == 0) n = CPU_COUNT(&cs);
  if ((f = fopen("/sys/fs/cgroup/cpu.max", "r"))) {
    char q[32];
    long per = 0;
    if (fscanf(f, "%31s %ld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
      const long c = atol(q) / per;
      if (c >= 1 && c < n) n = (int)c;
    }
    fclose(f);
  }
  return n;
}

/* The node leader's permutations (one process per GPU, parity mode): rank 0 builds every
   trial's permutation once, with speculation on the node's spare CPUs, into a shared pool
   that every rank's devices read (ranks.c, fh_pool_*); the other ranks take each trial's
   rows and rand() state from it instead of replaying the permutation and its speculation.
   FSCL_AMD_PERM_LEADER=0 turns it off (every rank builds its own, as before). */
static struct {
  int on;            /* in the current permute_pipelined call */
  int sizing;        /* the leader's CPU sizing (on, or rank 0 of a rehearsal replay, FSCL_AMD_SIM) */
  fh_pool_t *pool;
  int registered;    /* this rank's devices read the pool directly (else: a copy into D.stage) */
} PL;

static int perm_leader_wanted(void) {
  const char *e = getenv("FSCL_AMD_PERM_LEADER");
  return D.world > 1 && D.shm && !D.sim && (!e || atoi(e) != 0);
}

/* the rehearsal (FSCL_AMD_SIM replay as rank 0 of world) sizes its threads as the leader would */
static int perm_leader_sizing(void) {
  const char *e = getenv("FSCL_AMD_PERM_LEADER");
  return perm_leader_wanted() || (D.sim && D.sim_replay && D.world > 1 && D.rank == 0 && (!e || atoi(e) != 0));
}

/* worker threads: FSCL_AMD_SPEC, else this process's share of the usable CPUs (one process
   per GPU shares the node: LOCAL_WORLD_SIZE) less the main thread.  With the node leader's
   permutations: the leader takes every CPU the ranks' main threads leave, the others none */
static int spec_threads_wanted(void) {
  const char *e = getenv("FSCL_AMD_SPEC"), *lw = getenv("LOCAL_WORLD_SIZE");
  const int local = lw && atoi(lw) > 0 ? atoi(lw) : PL.sizing ? D.world : 1;
  int n;
  if (PL.on && D.rank != 0) return 0;
  n = e ? atoi(e) : PL.sizing ? usable_cpus() - local : usable_cpus() / local - 1;
  return n < 0 ? 0 : n > SPEC_MAX ? SPEC_MAX : n;
}

static void spec_start(void) {
  const int want = spec_threads_wanted();
  if (SP.n_th > want) {  /* a layout with fewer workers than the last call's (no job is posted here) */
    int t;
    pthread_mutex_lock(&SP.mu);
    SP.n_keep = want;
    pthread_cond_broadcast(&SP.cv);
    pthread_mutex_unlock(&SP.mu);
    for (t = want; t < SP.n_th; t++) {
      pthread_join(SP.th[t], NULL);
      fh_plan_free(SP.plan + t);  /* the joined worker's plan scratch */
    }
    SP.n_th = want;
    SP.n_keep = SPEC_MAX;
  }
  while (SP.n_th < want) {
    if (pthread_create(&SP.th[SP.n_th], NULL, spec_worker, (void *)(intptr_t)SP.n_th) != 0) break;
    SP.n_th++;
  }
}

void fh_spec_stop(void) {
  int t;
  pthread_mutex_lock(&SP.mu);
  SP.stop = 1;
  SP.gen++;
  pthread_cond_broadcast(&SP.cv);
  pthread_mutex_unlock(&SP.mu);
  for (t = 0; t < SP.n_th; t++) pthread_join(SP.th[t], NULL);
  for (t = 0; t <= SPEC_MAX; t++) fh_plan_free(SP.plan + t);  /* workers' and the main thread's plan scratch */
  SP.n_th = 0;
  SP.stop = 0;
  if (!SP.pb_in_pool)
    for (t = 0; t < SP.n_pb; t++) { fsclg_host_free(SP.pb[t].buf); free(SP.pb[t].nul); }
  SP.n_pb = SP.pb_cap = SP.pb_nchr = SP.pb_rb = SP.pb_in_pool = 0;
  SP.pb_bytes = 0;
}

/* candidates posted per trial: two per worker thread (a C4 candidate takes ~0.7 ms of one
   thread, a tail trial at 8 GPUs ~1.5-2.5 ms, so each thread builds two or three; the most
   likely are posted first), at most SPEC_MAX */
static int spec_ncand(void) { return SP.n_th * 2 < SPEC_MAX ? SP.n_th * 2 : SPEC_MAX; }

/* buffers: K slots, the posted candidates, the cancelled ones still running (one per thread)
   and the main thread's own (no job posted) */
static int pb_count(int K) { return K + spec_ncand() + SP.n_th + 1; }

/* one buffer's bytes: a trial's rows, or its plan in plan mode */
static size_t pb_item_bytes(int n_snps) { return PM.on ? PM.bytes : (size_t)D.rb * (size_t)(n_snps ? n_snps : 1); }

/* buffers for K slots, the candidates and the main thread's own (no job posted) */
static void pb_reserve(int n_snps, int K) {
  const int want = pb_count(K);
  const size_t item = pb_item_bytes(n_snps);
  int b;
  if (SP.pb_in_pool) { SP.n_pb = 0; SP.pb_in_pool = 0; SP.pb_cap = 0; }
  if (SP.pb_cap < n_snps || SP.pb_nchr < D.n_chr || SP.pb_rb != D.rb || SP.pb_bytes != item) {
    for (b = 0; b < SP.n_pb; b++) { fsclg_host_free(SP.pb[b].buf); free(SP.pb[b].nul); }
    SP.n_pb = 0;
    SP.pb_cap = n_snps;
    SP.pb_nchr = D.n_chr;
    SP.pb_rb = D.rb;
    SP.pb_bytes = item;
  }
  for (; SP.n_pb < want; SP.n_pb++) {
    pbuf_t *p = SP.pb + SP.n_pb;
    p->buf = fsclg_host_alloc(item);
    if (!p->buf) logmsg(MSG_FATAL, "fscl_amd: row staging: %s", fsclg_last_error());
    p->nul = fh_malloc(sizeof(double) * (SP.pb_nchr ? SP.pb_nchr : 1), "null sums");
  }
  for (b = 0; b < SP.n_pb; b++) SP.pb[b].owner = PB_FREE;
}

static int pb_get(void) {
  int b;
  for (b = 0; b < SP.n_pb; b++)
    if (SP.pb[b].owner == PB_FREE) { SP.pb[b].owner = PB_HELD; return b; }
  logmsg(MSG_FATAL, "fscl_amd: no free permutation buffer");
  return -1;
}

/* the slot's last upload has read its buffer on every local device: free it (the leader's
   pool: once every rank has released the slot too; the releases are counted per rank, and
   every rank makes the same sequence of them) */
static void slot_release(int slot) {
  int l, b;
  for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_slot_wait(D.ctx[l], slot), "slot wait");
  if (PL.on) {
    fh_pool_release(PL.pool);
    if (D.rank == 0 && fh_pool_wait_released(PL.pool) != 0)
      logmsg(MSG_FATAL, "fscl_amd: permutation pool: a rank stopped releasing its row slots");
  }
  for (b = 0; b < SP.n_pb; b++) if (SP.pb[b].owner == slot) SP.pb[b].owner = PB_FREE;
}

/* collective: a pool large enough for the leader's buffers (K slots, two per worker thread, one
   for the main thread), then (leader) the buffers carved from it */
static void pool_setup(int n_snps, int K) {
  const size_t rows = (pb_item_bytes(n_snps) + 4095) & ~(size_t)4095;  /* rows, or a plan */
  const size_t nulb = ((sizeof(double) * (size_t)(D.n_chr ? D.n_chr : 1)) + 255) & ~(size_t)255;
  const int nbuf = pb_count(K);
  const size_t want = (size_t)nbuf * (rows + nulb);
  unsigned f = D.rank == 0 && (!PL.pool || fh_pool_bytes(PL.pool) < want) ? 1u : 0u;
  char dummy = 0;
  int b;
  if (fh_shm_allgather_flags(D.shm, &dummy, 1, 0, 0, 0, &f) != 0) logmsg(MSG_FATAL, "fscl_amd: rank exchange failed");
  if (f) {  /* the leader needs a new pool: every rank drops the old one and maps the new one */
    if (PL.pool) {
      if (PL.registered) fsclg_host_unregister(fh_pool_data(PL.pool));
      fh_pool_close(PL.pool);
    }
    PL.pool = fh_pool_open(D.shm, want);
    PL.registered = 0;
    if (!PL.pool) {  /* collective: every rank builds its own permutations this time */
      PL.on = 0;
      PL.sizing = 0;
      g_null_nt = 0;
      spec_start();
      D.st.spec_threads = SP.n_th;
      pb_reserve(n_snps, K);
      return;
    }
    /* FSCL_AMD_POOL_COPY=1 (tests): the fallback taken when page-locking fails, on purpose */
    PL.registered = !getenv("FSCL_AMD_POOL_COPY") &&
                    fsclg_host_register(fh_pool_data(PL.pool), fh_pool_bytes(PL.pool)) == FSCLG_OK;
    if (!PL.registered && !getenv("FSCL_AMD_POOL_COPY"))
      logmsg(MSG_WARN, "fscl_amd: the permutation pool could not be page-locked (%s): rows are copied to the "
                       "device staging\n", fsclg_last_error());
  }
  if (D.rank != 0) return;
  if (!SP.pb_in_pool)
    for (b = 0; b < SP.n_pb; b++) { fsclg_host_free(SP.pb[b].buf); free(SP.pb[b].nul); }
  for (b = 0; b < nbuf; b++) {
    char *base = fh_pool_data(PL.pool) + (size_t)b * (rows + nulb);
    SP.pb[b].buf = base;
    SP.pb[b].nul = (double *)(base + rows);
    SP.pb[b].owner = PB_FREE;
  }
  SP.n_pb = nbuf;
  SP.pb_in_pool = 1;
  SP.pb_cap = n_snps; SP.pb_nchr = D.n_chr; SP.pb_rb = D.rb; SP.pb_bytes = pb_item_bytes(n_snps);
}

void fh_pool_drop(void) {
  if (!PL.pool) return;
  if (SP.pb_in_pool) { SP.n_pb = 0; SP.pb_in_pool = 0; SP.pb_cap = 0; }
  if (PL.registered) fsclg_host_unregister(fh_pool_data(PL.pool));
  fh_pool_close(PL.pool);
  PL.pool = NULL;
  PL.registered = 0;
}

/* no candidate running (cancelled ones included): the buffers are the caller's again */
static void spec_quiesce(void) {
  pthread_mutex_lock(&SP.mu);
  SP.gen++;
  SP.n_job = SP.next = 0;
  while (SP.running) pthread_cond_wait(&SP.done, &SP.mu);
  pthread_mutex_unlock(&SP.mu);
}

/* build candidates for the draw counts dl[0..nd) from stream state *g */
static void spec_post(const fh_rand_t *g, const int *dl, int nd) {
  int c;
  pthread_mutex_lock(&SP.mu);
  SP.base = *g;
  for (c = 0; c < nd; c++) {
    int b;
    for (b = 0; b < SP.n_pb && SP.pb[b].owner != PB_FREE; b++) {}
    if (b == SP.n_pb) break;
    SP.pb[b].owner = PB_CAND;
    SP.d[c] = dl[c]; SP.bi[c] = b; SP.state[c] = 0;
  }
  SP.next = 0;
  SP.n_job = c;
  SP.gen++;
  pthread_cond_broadcast(&SP.cv);
  pthread_mutex_unlock(&SP.mu);
  D.st.spec_posted++;
  D.st.spec_cands += (unsigned long long)c;
}

/* the candidate for d draws (its end state into *g), or -1; the others are cancelled and
   their buffers freed */
static int spec_take(int d, fh_rand_t *g) {
  int c, hit = -1, bi = -1;
  pthread_mutex_lock(&SP.mu);
  for (c = 0; c < SP.n_job; c++) if (SP.d[c] == d) hit = c;
  if (hit >= 0) D.st.spec_rank[hit < 7 ? hit : 7]++;  /* the draw count's rank among the candidates posted */
  if (hit >= 0 && SP.state[hit] == 0) {
    /* not started (the workers are still on likelier ones): building it here is faster than
       waiting for a worker to get to it; the caller builds it (its buffer is freed below) */
    D.st.spec_claimed++;
    hit = -1;
  }
  if (hit >= 0) {
    const double t0 = fh_now();
    while (SP.state[hit] < 2) pthread_cond_wait(&SP.done, &SP.mu);
    D.st.spec_wait_s += fh_now() - t0;
    if (SP.state[hit] == 2) {
      *g = SP.end[hit];
      D.st.negj += SP.negj[hit];
      bi = SP.bi[hit];
      SP.pb[bi].owner = PB_HELD;
      D.st.spec_hits++;
    }
  }
  /* cancel the rest without waiting: a running one frees its buffer when it stops */
  for (c = 0; c < SP.n_job; c++)
    if (c != hit && SP.state[c] != 1 && SP.pb[SP.bi[c]].owner == PB_CAND) SP.pb[SP.bi[c]].owner = PB_FREE;
  SP.gen++;
  SP.n_job = SP.next = 0;
  pthread_mutex_unlock(&SP.mu);
  return bi;
}

/* ------------------------------------------------ pipelined permutation trials
   scan-chromosome.c:582-652 with --n-threads=1 pruning semantics, K trials in flight
   (FSCL_AMD_DEPTH, default 4, at most FSCLG_N_SLOTS).  What orders the trials is the rand() stream: trial t+1's permutation depends on
   the draws of trial t, and a point draws only on a hit that takes its permute_p to >= 20
   (scan-chromosome.c:488-498); only those points can be pruned.  Each point keeps a queue of
   its results by trial, applied strictly in trial order; u = permute_p + queued results is an
   upper bound of permute_p before the next trial.
     * points with u >= 20 - K ("near-critical") form the trial's blocking batch, on the
       high-priority stream; the next permutation is built once it has been applied;
     * the rest form a bulk batch on a normal stream, waited only when its row slot comes
       round again (K trials later).
   A point with u <= 19 cannot draw in any queued trial (its permute_p stays <= 19 through
   them), so results may be applied late without changing a draw.  A point enters the
   near-critical class at u = 20 - K and can draw no earlier than K - 1 trials later, by when
   its bulk results have been waited for: each trial's draws happen in point order after its
   own permutation, as in the lockstep loop (a violation is caught and the pending batches
   are drained first; never seen, counted in stats).  Results are identical to the lockstep
   order (FSCL_AMD_LOCKSTEP=1). */
#define PQ (FSCLG_N_SLOTS + 2)
typedef struct {
  int trial;
  int have;
  double clr, lalpha;
  int start_pos;
} pres_t;
typedef struct {
  pres_t e[PQ];
  int head, n;
} pqueue_t;

typedef struct {
  int batch;              /* device batch */
  int trial;
  int n, cap;
  int *pt;                /* scan point of each cell, ascending */
  fsclg_cell_t *cells;
  fsclg_point_t *out;
  int submitted;
  int lo[FH_MAX_DEV], hi[FH_MAX_DEV];  /* the local devices' shares, fixed at submission */
} trial_batch_t;

/* per scan point: its permutation cell's cost in the last trial that evaluated it
   (snp_likelihood terms / 1024, from the completed results, so identical on every rank);
   0 = not yet measured */
static double *g_pcost;

/* a point's cell in a permutation trial */
static void trial_cell(const scan_pt_t *q, int large_grid_sp, fsclg_cell_t *cl) {
  cl->chr = q->chr;
  cl->start_pos = q->sweep_pos - (q->sweep_pos % large_grid_sp); /* Q5: G-aligned, unclipped */
  cl->end_pos = cl->start_pos + large_grid_sp;
  cl->pad = 0;
}

static void tb_reserve(trial_batch_t *b, int n) {
  if (n <= b->cap) return;
  b->cap = n;
  b->pt = fh_realloc(b->pt, sizeof(int) * n, "batch");
  b->cells = fh_realloc(b->cells, sizeof(fsclg_cell_t) * n, "batch");
  b->out = fh_realloc(b->out, sizeof(fsclg_point_t) * (n + 1), "batch");  /* + the exchange's flag word */
}

static void tb_free(trial_batch_t *b) { free(b->pt); free(b->cells); free(b->out); memset(b, 0, sizeof *b); }

/* the most cells any device (of every rank) would get if batch B joined batch A: the devices'
   shares are the cost-balanced contiguous split of tb_plan, over the merged ascending point list */
static int merged_max_share(const scan_t *s, const trial_batch_t *A, const trial_batch_t *B, int eval_range) {
  const int T = D.world * D.n_dev, n = A->n + B->n;
  double *cost;
  int ia = 0, ib = 0, k, g, mx = 0;
  if (T <= 1) return n;
  cost = fh_malloc(sizeof(double) * (size_t)n, "cost");
  for (k = 0; k < n; k++) {
    const int pt = (ib >= B->n || (ia < A->n && A->pt[ia] < B->pt[ib])) ? A->pt[ia++] : B->pt[ib++];
    cost[k] = g_pcost && g_pcost[pt] > 0 ? g_pcost[pt] : fh_window_cost(s->scan_pts[pt].chr, eval_range) / 32.0;
  }
  for (g = 0; g < T; g++) {
    int lo, hi;
    fscl_amd_partition(cost, n, g, T, &lo, &hi);
    if (hi - lo > mx) mx = hi - lo;
  }
  free(cost);
  return mx;
}

/* the local devices' shares of a batch, fixed at planning */
static void tb_plan(trial_batch_t *b, int eval_range) {
  double *cost = NULL;
  int i;
  if (D.world * D.n_dev > 1) {
    /* a point's measured cell cost from its last trial, else its window size (~32 terms /
       1024 per window site) */
    cost = fh_malloc(sizeof(double) * (b->n ? b->n : 1), "cost");
    for (i = 0; i < b->n; i++)
      cost[i] = g_pcost && g_pcost[b->pt[i]] > 0 ? g_pcost[b->pt[i]] : fh_window_cost(b->cells[i].chr, eval_range) / 32.0;
  }
  fh_dev_shares(cost, b->n, b->lo, b->hi);
  free(cost);
}

/* each local device's window null sums for its shares of a trial's two batches, before their
   submits (the pruned tail: only the few active cells' windows) */
static void trial_windows(int slot, const trial_batch_t *a, const trial_batch_t *b, int eval_range) {
  fsclg_cell_t *tmp = NULL;
  int l;
  for (l = 0; l < D.n_dev; l++) {
    const int na = a->hi[l] - a->lo[l], nb = b->hi[l] - b->lo[l];
    tmp = fh_realloc(tmp, sizeof(fsclg_cell_t) * (na + nb ? na + nb : 1), "cells");
    memcpy(tmp, a->cells + a->lo[l], sizeof(fsclg_cell_t) * (size_t)na);
    memcpy(tmp + na, b->cells + b->lo[l], sizeof(fsclg_cell_t) * (size_t)nb);
    fh_dev_check(fsclg_slot_windows(D.ctx[l], slot, tmp, na + nb, eval_range), "window sums");
  }
  free(tmp);
}

static void tb_submit(trial_batch_t *b, int slot, int eval_range, int bp_resl) {
  int l;
  for (l = 0; l < D.n_dev; l++) {
    fh_dev_check(fsclg_search_submit(D.ctx[l], b->batch, slot, b->cells + b->lo[l], b->hi[l] - b->lo[l], eval_range,
                                  bp_resl),
              "search submit");
    D.st.gp_evals += (unsigned long long)(b->hi[l] - b->lo[l]);
  }
  b->submitted = 1;
}

/* wait for a batch and file each result in its point's queue; `flags`: see exchange_points_flags */
static void tb_wait_flags(trial_batch_t *b, pqueue_t *pq, unsigned *flags) {
  int k, l;
  double tw = fh_now();
  if (!b->submitted) return;
  for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_search_wait(D.ctx[l], b->batch, b->out + b->lo[l]), "search wait");
  b->submitted = 0;
  D.st.wait_s += fh_now() - tw;
  fh_exchange_points_flags(b->out, b->n, b->lo[0], b->hi[D.n_dev - 1], flags);
  if (g_pcost)
    for (k = 0; k < b->n; k++) g_pcost[b->pt[k]] = (double)b->out[k].cost;
  for (k = 0; k < b->n; k++) {
    pqueue_t *q = pq + b->pt[k];
    int j;
    for (j = 0; j < q->n; j++) {
      pres_t *e = q->e + (q->head + j) % PQ;
      if (e->trial == b->trial) {
        e->have = 1; e->clr = b->out[k].clr; e->lalpha = b->out[k].lalpha; e->start_pos = b->cells[k].start_pos;
        break;
      }
    }
    if (j == q->n) logmsg(MSG_FATAL, "fscl_amd: permutation pipeline lost a result");
  }
}

static void tb_wait(trial_batch_t *b, pqueue_t *pq) { tb_wait_flags(b, pq, NULL); }

/* apply point i's queued results in trial order, up to trial `upto`; only trial `draw`
   may draw rand() (scan-chromosome.c:488-502) */
static unsigned long long g_draws;  /* rand() draws of the pruning pass so far */

typedef struct { int trial, draw; fh_rand_t *g; } pq_draw_t;
static int pq_draw(void *ctx) {
  const pq_draw_t *d = ctx;
  if (d->trial != d->draw) logmsg(MSG_FATAL, "fscl_amd: permutation pipeline: out-of-order rand draw");
  g_draws++;
  return fh_rand(d->g);
}

static void pq_flush(scan_t *s, pqueue_t *pq, int i, int upto, int draw, fh_rand_t *g, int save) {
  pqueue_t *q = pq + i;
  while (q->n > 0) {
    pres_t *e = q->e + q->head;
    pq_draw_t d = {e->trial, draw, g};
    if (!e->have || e->trial > upto) break;
    fh_trial_apply(s->scan_pts + i, e->clr, e->lalpha, e->start_pos, save, pq_draw, &d);
    q->head = (q->head + 1) % PQ;
    q->n--;
  }
}

/* the most likely draw counts of the trial whose blocking batch is A (into dl, at most nmax):
   every point that may draw hits with probability ~ its hit rate so far; d is their sum, taken
   as normal -- a window of integers around the mean, 3.3 sigma each side */
static int spec_candidates(const scan_t *s, const pqueue_t *pq, const trial_batch_t *A, int nmax, int *dl) {
  double mu = 0., var = 0.;
  int m = 0, k, lo, nd;
  for (k = 0; k < A->n; k++) {
    const scan_pt_t *q = s->scan_pts + A->pt[k];
    if (q->permute_p + pq[A->pt[k]].n >= 20) {
      const double h = (q->permute_p + 1.0) / (q->permute_n + 2.0);
      mu += h;
      var += h * (1. - h);
      m++;
    }
  }
  if (m == 0) { dl[0] = 0; return 1; }
  nd = 2 * (int)ceil(3.3 * sqrt(var)) + 1;
  if (nd > nmax) nd = nmax;
  if (nd > m + 1) nd = m + 1;
  lo = (int)floor(mu + 0.5) - nd / 2;
  if (lo + nd - 1 > m) lo = m - nd + 1;
  if (lo < 0) lo = 0;
  for (k = 0; k < nd; k++) dl[k] = lo + k;
  for (k = 1; k < nd; k++) { /* most likely first: free workers take them in this order */
    const int v = dl[k];
    int b = k;
    for (; b > 0 && fabs(dl[b - 1] - mu) > fabs(v - mu); b--) dl[b] = dl[b - 1];
    dl[b] = v;
  }
  return nd;
}

/* plan mode for this permute_pipelined call (PM.on): only when no chromosome's whole-chromosome
   null sum is read (the host never needs the permuted rows);
   the buffers are sized from one plan drawn from a copy of the stream (every rank draws the same).
   FSCL_AMD_PLAN=0: never; FSCL_AMD_PLAN_ECAP=m (tests): buffers of m entries, so that a plan can
   fail to fit and the trial falls back to rows built on the host */
static int plan_mode_setup(double nbp, double width_mb, const fh_rand_t *g) {
  const char *e = getenv("FSCL_AMD_PLAN"), *ec = getenv("FSCL_AMD_PLAN_ECAP");
  const int n = D.n_snps_key, ecap0 = n + n / 4096 + 16, gcap0 = 1 << 16;
  fh_rand_t r = *g;
  unsigned long long nj = 0;
  fsclg_swap_t *ent;
  int32_t *grp;
  int ne = 0, ng = 0, st;
  if ((e && atoi(e) == 0) || !D.chr_list || D.n_chr_list > 0 || n <= 0) return 0;
  ent = fh_malloc(sizeof(fsclg_swap_t) * (size_t)ecap0, "plan");
  grp = fh_malloc(sizeof(int32_t) * (size_t)(gcap0 + 1), "plan");
  st = fh_plan_build(SP.plan + SPEC_MAX, &PM.G, nbp, width_mb, &r, &nj, ent, ecap0, grp, gcap0, &ne, &ng, NULL, 0);
  free(ent); free(grp);
  if (st != 0) return 0;
  PM.ecap = 2 * ne + 4096 < ecap0 ? 2 * ne + 4096 : ecap0;
  PM.gcap = 2 * ng + 1024;
  if (ec) PM.ecap = atoi(ec) > 0 ? atoi(ec) : 1;
  PM.bytes = sizeof(plan_hdr_t) + ((sizeof(int32_t) * (size_t)(PM.gcap + 1) + 15) & ~(size_t)15) +
             sizeof(fsclg_swap_t) * (size_t)PM.ecap;
  if (PM.bytes > (size_t)D.rb * (size_t)D.stage_cap) {  /* small genomes: the slots' staging holds a plan too */
    const int cap = (int)((PM.bytes + (size_t)D.rb - 1) / (size_t)D.rb);
    int k;
    for (k = 0; k < FSCLG_N_SLOTS; k++) {
      fsclg_host_free(D.stage[k]);
      D.stage[k] = fsclg_host_alloc((size_t)D.rb * (size_t)cap);
      if (!D.stage[k]) logmsg(MSG_FATAL, "fscl_amd: row staging: %s", fsclg_last_error());
    }
    D.stage_cap = cap;
  }
  return 1;
}

/* what permute_pipelined's loop carries between trials */
typedef struct {
  scan_t *s;
  int n_perm, eval_range, bp_resl, large_grid_sp, save;
  double nbp, width_mb;
  fh_rand_t *g;
  int K, S;                             /* trials in flight; row slots (and bulk batches) */
  int n_pre, no_merge;
  trial_batch_t A, Bt[FSCLG_N_SLOTS];   /* the blocking batch; each row slot's bulk batch */
  double *nul[FSCLG_N_SLOTS];           /* each row slot's whole-chromosome null sums */
  pqueue_t *pq;
  int *act, n_act;
  int pre_bi[FSCLG_N_SLOTS];  /* the candidate buffer spare slot S + i was prepared from (owner PB_PRE), or -1 */
  int posted;                 /* candidates for the next trial were posted */
  unsigned long long draw_mark;
  int trial, done;            /* the current trial; the last one applied */
  FILE *tt;                   /* FSCL_AMD_TRIAL_TRACE (development aid) */
} pipe_t;

/* a trial's permutation: the rows (or plan) and null sums, and where they are */
typedef struct {
  void *rows;
  double *nul;
  int from_spec;  /* the null sums come with it */
  int rows_here;  /* plan mode: this trial's rows were built on the host into D.stage[slot] */
  int use_pre;    /* it was pre-staged in spare slot use_pre (>= S), to be swapped in */
} trial_perm_t;

static void pipe_setup(pipe_t *P, scan_t *s, int n_perm, double permute_nbp, int eval_range, int bp_resl,
                       int large_grid_sp, double scan_width_mb, fh_rand_t *g, int save) {
  /* the bulk batches' cells get up to FSCL_AMD_BULK_SPLIT workgroups each when they are few (the
     pruned tail), so that a bulk batch is done before its slot comes round again */
  const int bulk_split = fh_env_int("FSCL_AMD_BULK_SPLIT", 4, 1, INT_MAX);
  const int n = s->n_scan_pts ? s->n_scan_pts : 1;
  int i, k, l;
  memset(P, 0, sizeof *P);
  P->s = s; P->n_perm = n_perm; P->nbp = permute_nbp; P->eval_range = eval_range; P->bp_resl = bp_resl;
  P->large_grid_sp = large_grid_sp; P->width_mb = scan_width_mb; P->g = g; P->save = save;
  P->K = fh_env_int("FSCL_AMD_DEPTH", 4, 2, FSCLG_N_SLOTS);
  /* row slots (and bulk batches): S >= K trials' rows on the devices (FSCL_AMD_SLOTS, at most FSCLG_N_SLOTS).
     The blocking class keeps the margin K; a bulk batch is waited only when its slot comes round, S
     trials later, and a point that may draw before its bulk results are in drains them first. */
  P->S = fh_env_int("FSCL_AMD_SLOTS", P->K, P->K, FSCLG_N_SLOTS);
  P->no_merge = getenv("FSCL_AMD_NO_MERGE") != NULL;  /* read once: every rank must decide alike */
  P->n_act = s->n_scan_pts; P->trial = P->done = -1;
  P->A.batch = 0; /* high-priority stream */
  for (k = 0; k < P->S; k++) {
    P->Bt[k].batch = 2 + k;
    P->nul[k] = fh_malloc(sizeof(double) * (D.n_chr ? D.n_chr : 1), "null sums");
    for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_set_batch_split(D.ctx[l], P->Bt[k].batch, bulk_split), "batch split");
  }
  P->act = fh_malloc(sizeof(int) * n, "active points");
  P->pq = fh_calloc(n, sizeof(pqueue_t), "result queues");
  if (D.world * D.n_dev > 1) g_pcost = fh_calloc(n, sizeof(double), "point costs");
  tb_reserve(&P->A, n);
  for (k = 0; k < P->S; k++) tb_reserve(&P->Bt[k], n);
  for (i = 0; i < P->n_act; i++) P->act[i] = i;
  P->tt = getenv("FSCL_AMD_TRIAL_TRACE") ? fopen(getenv("FSCL_AMD_TRIAL_TRACE"), "w") : NULL;
  PL.on = perm_leader_wanted();
  PL.sizing = perm_leader_sizing();
  if (PL.sizing) {
    const char *lw = getenv("LOCAL_WORLD_SIZE");
    const int local = lw && atoi(lw) > 0 ? atoi(lw) : D.world;
    g_null_nt = usable_cpus() - local + 1;
    if (g_null_nt < 1) g_null_nt = 1;
  }
  PM.on = plan_mode_setup(permute_nbp, scan_width_mb, g);
  D.st.plan_mode = PM.on;
  /* the switches every rank's batches and collectives follow must agree (an environment variable
     set on one rank only would otherwise diverge the exchanges) */
  fh_ranks_agree("FSCL_AMD_DEPTH / FSCL_AMD_SLOTS / FSCL_AMD_NO_MERGE / FSCL_AMD_PERM_LEADER / FSCL_AMD_PLAN*",
              (uint64_t)P->K | (uint64_t)P->S << 4 | (uint64_t)P->no_merge << 8 | (uint64_t)PL.on << 9 |
              (uint64_t)PM.on << 10 | (uint64_t)(PM.on ? PM.ecap : 0) << 11 | (uint64_t)(PM.on ? PM.gcap : 0) << 40);
  spec_start();
  D.st.spec_threads = SP.n_th;
  if (PL.on) pool_setup(s->n_snps, P->S);
  else pb_reserve(s->n_snps, P->S);
  D.st.perm_leader = PL.on;
  SP.snps = s->snps; SP.n = s->n_snps; SP.nbp = permute_nbp; SP.width_mb = scan_width_mb;
  /* pre-staging (plan mode, one process of one rank): while trial t's blocking batch runs, each of
     the likeliest candidates for trial t + 1 that a worker has finished by then is applied to a
     spare device slot with its window sums; when one is taken, its slot is swapped in and the
     trial's upload chain (plan kernels, window sums) is off its critical path.  Not with several
     ranks (the leader's candidates are not the other ranks').  FSCL_AMD_PRESTAGE=n: the n
     likeliest, in spare slots S .. S + n - 1 (0: off) */
  P->n_pre = fh_env_int("FSCL_AMD_PRESTAGE", 2, INT_MIN, INT_MAX);  /* 2: C5 one chromosome 15.1 s against 15.4 s with 1, 15.3 s with 3 */
  if (P->n_pre > FSCLG_N_SLOTS - P->S) P->n_pre = FSCLG_N_SLOTS - P->S;
  if (!(PM.on && D.world == 1 && !PL.on && SP.n_th > 0)) P->n_pre = 0;
  if (P->n_pre < 0) P->n_pre = 0;
  for (k = 0; k < FSCLG_N_SLOTS; k++) P->pre_bi[k] = -1;
}

static void pipe_teardown(pipe_t *P) {
  int i, k, l;
  for (i = 0; i < P->s->n_scan_pts; i++)
    if (P->pq[i].n) logmsg(MSG_FATAL, "fscl_amd: permutation pipeline: unapplied results");
  for (k = 0; k < P->n_pre; k++) {  /* the spare slots' last uploads have read their buffers (a trial that did
                                       not come, or one taken just before the last trial ended the loop) */
    for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_slot_wait(D.ctx[l], P->S + k), "slot wait");
    if (P->pre_bi[k] >= 0 && SP.pb[P->pre_bi[k]].owner == PB_PRE) SP.pb[P->pre_bi[k]].owner = PB_FREE;
  }
  for (k = 0; k < P->S; k++) slot_release(k);  /* every upload has read its buffer */
  spec_quiesce();
  PL.on = 0;
  PL.sizing = 0;
  PM.on = 0;
  g_null_nt = 0;
  if (P->tt) fclose(P->tt);
  tb_free(&P->A);
  for (k = 0; k < P->S; k++) {
    for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_set_batch_split(D.ctx[l], P->Bt[k].batch, 1), "batch split");
    tb_free(&P->Bt[k]);
    free(P->nul[k]);
  }
  free(P->act); free(P->pq);
  free(g_pcost); g_pcost = NULL;
}

/* the oldest bulk batch still in flight of a trial before `before_trial`, or NULL */
static trial_batch_t *oldest_bulk(pipe_t *P, int before_trial) {
  trial_batch_t *old = NULL;
  int k;
  for (k = 0; k < P->S; k++)
    if (P->Bt[k].submitted && P->Bt[k].trial < before_trial && (!old || P->Bt[k].trial < old->trial)) old = &P->Bt[k];
  return old;
}

/* wait a bulk batch in flight and apply its points' results up to trial `upto` (no draws among them) */
static void wait_flush_bulk(pipe_t *P, trial_batch_t *b, int upto) {
  int k;
  if (!b->submitted) return;
  tb_wait(b, P->pq);
  for (k = 0; k < b->n; k++) pq_flush(P->s, P->pq, b->pt[k], upto, -1, P->g, P->save);
}

/* the next trial's permutation, for row slot `slot`: a follower takes the leader's from the pool;
   otherwise the candidate for the previous trial's draw count, else it is built here; a plan that
   does not fit falls back to rows built on the host */
static trial_perm_t trial_permutation(pipe_t *P, int slot) {
  const scan_t *s = P->s;
  fh_rand_t *g = P->g;
  trial_perm_t t = {NULL, NULL, 0, 0, 0};
  int k;
  if (PL.on && D.rank != 0) {
    /* the leader's permutation of this trial: its rows, its null sums, and the rand() state
       after it (the prune draws that follow are this rank's own, the same as the leader's) */
    size_t ro, no;
    unsigned long long nj;
    fh_rand_t g0 = *g;
    if (fh_pool_take(PL.pool, &ro, &no, g, &nj) != 0) logmsg(MSG_FATAL, "fscl_amd: permutation pool: no leader");
    t.rows = fh_pool_data(PL.pool) + ro;
    t.nul = (double *)(fh_pool_data(PL.pool) + no);
    t.from_spec = 1;
    if (PM.on && !((plan_hdr_t *)t.rows)->ok) {  /* a plan that did not fit: the rows, from this rank's own stream */
      unsigned long long nj2 = 0;
      block_permute(D.stage[slot], D.rowp, s->n_snps, P->nbp, P->width_mb, &g0, &nj2, NULL, 0);
      if (memcmp(&g0, g, sizeof g0) != 0 || nj2 != nj) logmsg(MSG_FATAL, "fscl_amd: permutation pool: stream mismatch");
      t.rows_here = 1;
      D.st.plan_fallback++;
    }
    D.st.negj += nj;
  } else {
    const unsigned long long negj0 = D.st.negj;
    int bi = P->posted ? spec_take((int)(g_draws - P->draw_mark), g) : -1;
    t.from_spec = bi >= 0;
    for (k = 0; k < P->n_pre; k++) {
      if (P->pre_bi[k] < 0) continue;
      if (bi == P->pre_bi[k]) t.use_pre = P->S + k;  /* this spare slot holds the trial */
      else {  /* not taken: free its buffer once the spare's upload has read it */
        int l;
        for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_slot_wait(D.ctx[l], P->S + k), "slot wait");
        if (SP.pb[P->pre_bi[k]].owner == PB_PRE) SP.pb[P->pre_bi[k]].owner = PB_FREE;
      }
      P->pre_bi[k] = -1;
    }
    if (bi < 0) {
      bi = pb_get();
      if (PM.on) {
        const fh_rand_t g0 = *g;
        unsigned long long nj = 0;
        if (plan_into(SP.pb[bi].buf, SP.plan + SPEC_MAX, P->nbp, P->width_mb, g, &nj, NULL, 0) == 0)
          D.st.negj += nj;
        else {  /* the plan did not fit its buffer: this trial's rows on the host (hdr.ok = 0 tells the ranks) */
          *g = g0;
          block_permute(D.stage[slot], D.rowp, s->n_snps, P->nbp, P->width_mb, g, &D.st.negj, NULL, 0);
          t.rows_here = 1;
          D.st.plan_fallback++;
        }
      } else
        block_permute(SP.pb[bi].buf, D.rowp, s->n_snps, P->nbp, P->width_mb, g, &D.st.negj, NULL, 0);
    }
    SP.pb[bi].owner = slot;
    t.rows = SP.pb[bi].buf;
    t.nul = SP.pb[bi].nul;
    if (PL.on) {  /* the leader: complete and publish it */
      if (!t.from_spec) {
        if (PM.on) memset(t.nul, 0, sizeof(double) * (D.n_chr ? D.n_chr : 1));
        else fh_chr_null_sums(t.rows, t.nul);
      }
      t.from_spec = 1;
      if (fh_pool_publish(PL.pool, (size_t)((char *)t.rows - fh_pool_data(PL.pool)),
                          (size_t)((char *)t.nul - fh_pool_data(PL.pool)), g, D.st.negj - negj0) != 0)
        logmsg(MSG_FATAL, "fscl_amd: permutation pool: a rank stopped taking permutations");
    }
  }
  return t;
}

/* the trial's null sums completed, and its permutation on the devices in row slot `slot`: host
   rows, a swapped-in spare slot, a plan, or the rows (a pool that is not page-locked: through the
   slot's own staging) */
static void trial_upload(pipe_t *P, int slot, trial_perm_t *t) {
  double tp = fh_now();
  int l;
  if (!t->from_spec && !PM.on) fh_chr_null_sums(t->rows, t->nul);  /* a candidate carries its own; plan mode reads none */
  if (!t->from_spec && PM.on) memset(t->nul, 0, sizeof(double) * (D.n_chr ? D.n_chr : 1));
  D.st.host_null_s += fh_now() - tp;
  memcpy(P->nul[slot], t->nul, sizeof(double) * (D.n_chr ? D.n_chr : 1));
  tp = fh_now();
  if (t->rows_here) slot_upload_buf(slot, D.stage[slot], P->nul[slot]);
  else if (t->use_pre) {
    for (l = 0; l < D.n_dev; l++) fh_dev_check(fsclg_slot_swap(D.ctx[l], slot, t->use_pre), "slot swap");
    D.st.prestage_hits++;
  } else {
    if (PL.on && !PL.registered) {
      memcpy(D.stage[slot], t->rows, PM.on ? PM.bytes : (size_t)D.rb * (size_t)P->s->n_snps);
      t->rows = D.stage[slot];
    }
    if (PM.on) slot_upload_plan(slot, t->rows, P->nul[slot]);
    else slot_upload_buf(slot, t->rows, P->nul[slot]);
  }
  D.st.host_upload_s += fh_now() - tp;
}

/* the trial's two batches: near-critical points into the blocking batch A, the rest into the
   slot's bulk batch B; each point's queue gets the trial's entry */
static void trial_batches(pipe_t *P, trial_batch_t *B) {
  const scan_t *s = P->s;
  trial_batch_t *A = &P->A;
  pqueue_t *pq = P->pq;
  int i;
  A->n = B->n = 0;
  A->trial = B->trial = P->trial;
  for (i = 0; i < P->n_act; i++) {
    const int a = P->act[i];
    const scan_pt_t *q = s->scan_pts + a;
    trial_batch_t *b = q->permute_p + pq[a].n >= 20 - P->K ? A : B;
    pres_t *e = pq[a].e + (pq[a].head + pq[a].n) % PQ;
    if (pq[a].n == PQ) logmsg(MSG_FATAL, "fscl_amd: permutation pipeline queue overflow");
    trial_cell(q, P->large_grid_sp, b->cells + b->n);
    b->pt[b->n++] = a;
    e->trial = P->trial; e->have = 0;
    pq[a].n++;
  }
  /* a small bulk batch joins the blocking batch when the blocking batch's cells keep their full
     split (8 members within 256 workgroups, half the launch budget, HISTORY.md §11.11): the
     early-prune tail's few bulk cells -- the most significant points, which never reach the
     blocking class -- would otherwise run one workgroup per cell and hold up the host K trials
     later.  Merged in ascending point order (the blocking batch's draws go in that order; the
     merged points cannot draw).  The decision depends only on the counts: the same on every
     rank.  FSCL_AMD_NO_MERGE=1: never. */
  if (B->n > 0 && A->n + B->n <= 32 * D.world * D.n_dev && !P->no_merge &&
      merged_max_share(s, A, B, P->eval_range) <= 32) {
    int ia = A->n - 1, ib = B->n - 1, o = A->n + B->n - 1;
    while (ib >= 0) {  /* merge from the back, in place in A (its capacity holds every active point) */
      if (ia >= 0 && A->pt[ia] > B->pt[ib]) { A->pt[o] = A->pt[ia]; A->cells[o] = A->cells[ia]; ia--; }
      else { A->pt[o] = B->pt[ib]; A->cells[o] = B->cells[ib]; ib--; }
      o--;
    }
    D.st.n_merged += (unsigned long long)B->n;
    A->n += B->n;
    B->n = 0;
  }
  D.st.n_crit += (unsigned long long)A->n;
}

/* while the blocking batch runs: each of the n_pre likeliest candidates for the next trial that a
   worker finishes before the batch is done goes to a spare slot, with its window sums */
static void prestage_candidates(pipe_t *P, trial_batch_t *B) {
  int k;
  for (k = 0; P->n_pre > 0 && P->posted && P->A.n > 0 && k < P->n_pre; k++) {
    /* the k-th likeliest candidate, if a worker finishes it before the blocking batch is done */
    int st0 = 0, b0 = -1, done = 0;
    for (;;) {
      int l;
      pthread_mutex_lock(&SP.mu);
      if (SP.n_job > k) { st0 = SP.state[k]; b0 = SP.bi[k]; } else st0 = 3;
      if (st0 == 2) SP.pb[b0].owner = PB_PRE;  /* spec_take's cancelling leaves it alone */
      pthread_mutex_unlock(&SP.mu);
      if (st0 >= 2) break;
      for (done = 1, l = 0; l < D.n_dev && done; l++) done = fsclg_search_done(D.ctx[l], P->A.batch) > 0;
      if (done) break;
      sched_yield();
    }
    if (st0 != 2) break;
    slot_upload_plan(P->S + k, SP.pb[b0].buf, SP.pb[b0].nul);
    trial_windows(P->S + k, &P->A, B, P->eval_range);
    P->pre_bi[k] = b0;
    D.st.prestaged++;
  }
}

/* wait the blocking batch and apply it, its draws in ascending point order; returns the ranks'
   agreed SIGINT flag.  tr[4..7]: the trace's stamps and counts */
static unsigned trial_apply(pipe_t *P, double *tr) {
  const scan_t *s = P->s;
  const trial_batch_t *A = &P->A;
  const pqueue_t *pq = P->pq;
  trial_batch_t *old;
  unsigned sig;
  int drain = 0, m = 0, i, k;
  for (k = 0; k < A->n; k++) m += s->scan_pts[A->pt[k]].permute_p + pq[A->pt[k]].n >= 20;
  tr[4] = fh_now();
  /* the blocking batch's exchange (made every trial, even for no cells) carries each rank's
     SIGINT flag: every rank gets the OR, so all dump at the same trial (no extra collective) */
  sig = g_sigint ? 1u : 0u;
  tb_wait_flags(&P->A, P->pq, &sig);
  if (D.world <= 1 || D.sim) sig = g_sigint ? 1u : 0u;
  tr[5] = fh_now();
  /* a point that may draw in this trial needs every earlier result applied first */
  for (k = 0; k < A->n && !drain; k++) {
    const int a = A->pt[k];
    if (s->scan_pts[a].permute_p + pq[a].n >= 20)
      for (i = 0; i < pq[a].n; i++)
        if (!pq[a].e[(pq[a].head + i) % PQ].have) drain = 1;
  }
  if (drain) { /* never expected: wait the bulk batches in trial order */
    D.st.n_drain++;
    while ((old = oldest_bulk(P, P->trial))) wait_flush_bulk(P, old, P->trial - 1);
  }
  for (k = 0; k < A->n; k++) pq_flush(P->s, P->pq, A->pt[k], P->trial, P->trial, P->g, P->save);
  tr[6] = m; tr[7] = (double)(g_draws - P->draw_mark);
  return sig;
}

/* the schedule in the comment above PQ, one trial a turn */
static void permute_pipelined(scan_t *s, int n_perm, double permute_nbp, int eval_range, int bp_resl,
                              int large_grid_sp, double scan_width_mb, fh_rand_t *g, int save) {
  pipe_t P;
  trial_batch_t *old;
  double tr[8], tp;
  int i, k;
  pipe_setup(&P, s, n_perm, permute_nbp, eval_range, bp_resl, large_grid_sp, scan_width_mb, g, save);
  for (;;) {
    const int slot = (P.trial + 1) % P.S;
    trial_batch_t *B = &P.Bt[slot];
    trial_perm_t pm;
    unsigned sig;
    tp = fh_now();
    tr[0] = tp;
    wait_flush_bulk(&P, B, P.done);  /* the slot's previous trial: its bulk results */
    D.st.search_s += fh_now() - tp;
    tp = fh_now();
    tr[1] = tp;
    slot_release(slot);
    pm = trial_permutation(&P, slot);
    D.st.host_perm_s += fh_now() - tp;
    P.trial++;
    for (i = k = 0; i < P.n_act; i++)
      if (!s->scan_pts[P.act[i]].permute_finished) P.act[k++] = P.act[i];
    P.n_act = k;
    cr_logmsg(MSG_STATUS, "Scanning snp block permutations... %7d (%d scan pts remaining)        ", P.trial, P.n_act);
    if (P.n_act == 0 || P.trial > n_perm) break;
    tr[2] = fh_now();
    trial_upload(&P, slot, &pm);
    tp = fh_now();
    trial_batches(&P, B);
    /* both batches always go through submit / wait (an empty share is a no-op), so that
       every rank takes part in the same exchanges */
    tr[3] = fh_now();
    tb_plan(&P.A, eval_range);
    tb_plan(B, eval_range);
    trial_windows(slot, &P.A, B, eval_range);
    tb_submit(&P.A, slot, eval_range, bp_resl);
    tb_submit(B, slot, eval_range, bp_resl);
    /* while the GPUs work: the next trial's permutation for this trial's likely draw counts */
    P.posted = SP.n_th > 0 && !(PL.on && D.rank != 0);  /* with the leader's permutations only the leader speculates */
    if (P.posted) {
      int dl[SPEC_MAX];
      spec_post(g, dl, spec_candidates(s, P.pq, &P.A, spec_ncand(), dl));
    }
    P.draw_mark = g_draws;
    prestage_candidates(&P, B);
    sig = trial_apply(&P, tr);
    P.done = P.trial;
    D.st.search_s += fh_now() - tp;
    D.st.trials++;
    if (P.tt) /* trial, active, blocking cells, bulk cells; us: bulk wait, permute, null sums + upload + build,
                 submit, blocking wait, flush; points that could draw, draws */
      fprintf(P.tt, "%d %d %d %d %.0f %.0f %.0f %.0f %.0f %.0f %.0f %.0f\n", P.trial, P.n_act, P.A.n, B->n,
              (tr[1] - tr[0]) * 1e6, (tr[2] - tr[1]) * 1e6, (tr[3] - tr[2]) * 1e6, (tr[4] - tr[3]) * 1e6,
              (tr[5] - tr[4]) * 1e6, (fh_now() - tr[5]) * 1e6, tr[6], tr[7]);
    if (sig) {
      /* the dump shows every trial up to this one: the bulk results still in flight first
         (no draws among them) */
      while ((old = oldest_bulk(&P, INT_MAX))) wait_flush_bulk(&P, old, P.trial);
      sigint_dump(s, n_perm);
    }
  }
  /* the bulk batches still in flight, oldest first */
  for (tp = fh_now(); (old = oldest_bulk(&P, INT_MAX)); tp = fh_now()) {
    wait_flush_bulk(&P, old, P.done);
    D.st.search_s += fh_now() - tp;
  }
  pipe_teardown(&P);
}

/* ------------------------------------------------ throughput mode (non-parity)
   The reference's trials are serial because one rand() stream feeds every permutation and
   every prune draw (scan-chromosome.c:441-456, 488-498).  In throughput mode the randomness
   is counter-based instead, so no trial depends on another:
     * trial t's permutation is block_permute driven by its own generator, the glibc TYPE_3
       stream seeded with tp_trial_seed(seed, t);
     * point i's prune draw in trial t is tp_prune_rand(seed, t, i);
     * a point's results are applied in trial order (hits, the p >= 20 prune test with the
       pre-increment count, the saved null CLRs) and it stops at its first prune, exactly as
       in the reference; results of later trials that were already evaluated are dropped.
   Each point's outcome is then a function of (seed, point) alone: identical for any number
   of GPUs, ranks, trials in flight or worker threads, and restated by the oracle
   (--throughput-seed).  Not bit-identical to the reference (different random numbers), but
   the same procedure: every trial is an independent block permutation, so the p-values have
   the reference's distribution.
   Schedule: rounds of Q = world * n_dev trials, trial r*Q + rank*n_dev + l on local device l;
   up to K rounds in flight (one row slot and one batch per round and device); round r
   evaluates the points still active after every round <= r - K is applied.  Worker threads
   build the permutations (and whole-chromosome null sums) of the next trials ahead, in any
   order, into a ring of pinned buffers. */
static int g_pmode = FSCL_AMD_PERMUTE_PARITY;
static unsigned long long g_pseed = 0xFD821A6ull;

int fscl_amd_set_permute_mode(int mode, unsigned long long seed) {
  if (mode != FSCL_AMD_PERMUTE_PARITY && mode != FSCL_AMD_PERMUTE_THROUGHPUT) return -1;
  g_pmode = mode;
  g_pseed = seed;
  return 0;
}

static uint64_t mix64(uint64_t z) { /* splitmix64's output function */
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static unsigned tp_trial_seed(uint64_t seed, long t) { return (unsigned)(mix64(seed ^ mix64((uint64_t)t + 1)) >> 32); }
static int tp_prune_rand(uint64_t seed, long t, int i) { /* 31 bits, as rand() */
  return (int)(mix64(mix64(seed ^ 0x632BE59BD9B4E019ull) ^ ((uint64_t)(uint32_t)t << 32 | (uint32_t)i)) >> 33);
}

typedef struct { long t; int i; } tp_draw_t;  /* point i's prune draw in trial t */
static int tp_draw(void *ctx) {
  const tp_draw_t *d = ctx;
  return tp_prune_rand(g_pseed, d->t, d->i);
}

static struct {
  pthread_t th[SPEC_MAX];
  int n_th;
  pthread_mutex_t mu;
  pthread_cond_t cv, done;
  int stop;
  long next, limit, total;  /* local trials j: the next to build; build only j < limit, j < total */
  int nb;                   /* ring of buffers: trial j in buf[j % nb] */
  void **buf;
  double **nul;
  long *built;              /* the trial each buffer holds, -1 none */
  long q, rank_off, n_perm; /* local trial j -> global trial (j / n_dev) * q + rank_off + j % n_dev */
  int n_dev;
  const snp_t *snps;
  int n;
  double nbp, width_mb;
  unsigned long long negj;
  double gen_s;
} TB = {.mu = PTHREAD_MUTEX_INITIALIZER, .cv = PTHREAD_COND_INITIALIZER, .done = PTHREAD_COND_INITIALIZER};

static long tb_trial(long j) { return j / TB.n_dev * TB.q + TB.rank_off + j % TB.n_dev; }

static void tb_build(long j) {
  static const unsigned zero = 0;
  const int b = (int)(j % TB.nb);
  const long t = tb_trial(j);
  unsigned long long negj = 0;
  if (t <= TB.n_perm) {
    fh_rand_t g;
    fh_srand(&g, tp_trial_seed(g_pseed, t));
    block_permute(TB.buf[b], D.rowp, TB.n, TB.nbp, TB.width_mb, &g, &negj, NULL, 0);
    chr_null_sums_1t(TB.buf[b], TB.nul[b], &zero, 0);
  }
  pthread_mutex_lock(&TB.mu);
  TB.negj += negj;
  TB.built[b] = j;
  pthread_cond_broadcast(&TB.done);
  pthread_mutex_unlock(&TB.mu);
}

static void *tb_worker(void *arg) {
  (void)arg;
  pthread_mutex_lock(&TB.mu);
  for (;;) {
    while (!TB.stop && !(TB.next < TB.limit && TB.next < TB.total)) pthread_cond_wait(&TB.cv, &TB.mu);
    if (TB.stop) break;
    {
      const long j = TB.next++;
      double t0;
      pthread_mutex_unlock(&TB.mu);
      t0 = fh_now();
      tb_build(j);
      pthread_mutex_lock(&TB.mu);
      TB.gen_s += fh_now() - t0;
    }
  }
  pthread_mutex_unlock(&TB.mu);
  return NULL;
}

/* start the builders of `total` local trials, trial j of global number tb_trial(j) (built while
   <= n_perm), for K rounds in flight: one ring buffer per trial in flight and per worker, plus a
   round ahead */
static void tb_start(int n_dev, long q, long rank_off, long n_perm, long total, int K, const scan_t *s, double nbp,
                     double width_mb) {
  const int want = spec_threads_wanted();
  int i;
  TB.n_dev = n_dev; TB.q = q; TB.rank_off = rank_off; TB.n_perm = n_perm;
  TB.snps = s->snps; TB.n = s->n_snps; TB.nbp = nbp; TB.width_mb = width_mb;
  TB.total = total; TB.next = 0; TB.negj = 0; TB.gen_s = 0.;
  TB.nb = (K + 1) * n_dev + want;
  TB.limit = TB.nb;
  TB.buf = fh_calloc((size_t)TB.nb, sizeof(void *), "permutation ring");
  TB.nul = fh_calloc((size_t)TB.nb, sizeof(double *), "permutation ring");
  TB.built = fh_malloc(sizeof(long) * (size_t)TB.nb, "permutation ring");
  for (i = 0; i < TB.nb; i++) {
    TB.buf[i] = fsclg_host_alloc((size_t)D.rb * (s->n_snps ? s->n_snps : 1));
    if (!TB.buf[i]) logmsg(MSG_FATAL, "fscl_amd: row staging: %s", fsclg_last_error());
    TB.nul[i] = fh_malloc(sizeof(double) * (D.n_chr ? D.n_chr : 1), "null sums");
    TB.built[i] = -1;
  }
  for (TB.n_th = 0; TB.n_th < want; TB.n_th++)
    if (pthread_create(&TB.th[TB.n_th], NULL, tb_worker, NULL) != 0) break;
}

/* trial j's buffer index, once it is built (by the main thread when there are no workers) */
static int tb_get(long j) {
  const int b = (int)(j % TB.nb);
  if (TB.n_th == 0) {
    if (TB.built[b] != j) tb_build(j);
    return b;
  }
  pthread_mutex_lock(&TB.mu);
  while (TB.built[b] != j) pthread_cond_wait(&TB.done, &TB.mu);
  pthread_mutex_unlock(&TB.mu);
  return b;
}

/* every trial below j has been read by its upload: their buffers may take later trials */
static void tb_release(long j) {
  pthread_mutex_lock(&TB.mu);
  if (j + TB.nb > TB.limit) TB.limit = j + TB.nb;
  pthread_cond_broadcast(&TB.cv);
  pthread_mutex_unlock(&TB.mu);
}

static void tb_stop(void) {
  int t;
  pthread_mutex_lock(&TB.mu);
  TB.stop = 1;
  pthread_cond_broadcast(&TB.cv);
  pthread_mutex_unlock(&TB.mu);
  for (t = 0; t < TB.n_th; t++) pthread_join(TB.th[t], NULL);
  for (t = 0; t < TB.nb; t++) { fsclg_host_free(TB.buf[t]); free(TB.nul[t]); }
  free(TB.buf); free(TB.nul); free(TB.built);
  TB.buf = NULL; TB.nul = NULL; TB.built = NULL;
  TB.n_th = TB.nb = 0;
  TB.stop = 0;
}

typedef struct {
  long r;
  int n, cap;
  int *pt;               /* the round's active points, ascending */
  fsclg_cell_t *cells;   /* their G-aligned cells (Q5), the same for every trial of the round */
  fsclg_point_t *out;    /* [Q][n]: trial q of the round at out + q * n */
  size_t out_cap;
  int live[FH_MAX_DEV];  /* local device l submitted its trial */
} tp_round_t;

static void permute_throughput(scan_t *s, int n_perm, double permute_nbp, int eval_range, int bp_resl,
                               int large_grid_sp, double scan_width_mb, int save) {
  /* rounds in flight: about 8 trials in all (at least 2 rounds), so that a pruned point's
     evaluations past its prune stay few; FSCL_AMD_DEPTH overrides */
  const int nd = D.n_dev, Q = D.world * nd;
  const int K = fh_env_int("FSCL_AMD_DEPTH", Q >= 4 ? 2 : FSCLG_N_SLOTS / Q, 1, FSCLG_N_SLOTS);
  const long R = ((long)n_perm + Q) / Q; /* rounds holding trials 0 .. n_perm */
  tp_round_t rd[FSCLG_N_SLOTS];
  long r_sub = 0, r_done = 0;
  int stop_sub = 0, i, k, l;
  memset(rd, 0, sizeof rd);
  tb_start(nd, Q, (long)D.rank * nd, n_perm, R * nd, K, s, permute_nbp, scan_width_mb);
  D.st.spec_threads = TB.n_th;
  while (r_done < r_sub || (!stop_sub && r_sub < R)) {
    if (!stop_sub && r_sub < R && r_sub - r_done < K) {
      tp_round_t *b = rd + r_sub % K;
      const int slot = (int)(r_sub % K);
      double tp = fh_now();
      b->n = 0;
      if (b->cap < s->n_scan_pts) {
        b->cap = s->n_scan_pts;
        b->pt = fh_realloc(b->pt, sizeof(int) * (size_t)(b->cap ? b->cap : 1), "round");
        b->cells = fh_realloc(b->cells, sizeof(fsclg_cell_t) * (size_t)(b->cap ? b->cap : 1), "round");
      }
      for (i = 0; i < s->n_scan_pts; i++) {
        const scan_pt_t *q = s->scan_pts + i;
        if (q->permute_finished) continue;
        trial_cell(q, large_grid_sp, b->cells + b->n);
        b->pt[b->n++] = i;
      }
      if (b->n == 0) { stop_sub = 1; continue; }
      if (b->out_cap < (size_t)Q * b->n) {
        b->out_cap = (size_t)Q * b->n;
        b->out = fh_realloc(b->out, sizeof(fsclg_point_t) * b->out_cap, "round");
      }
      b->r = r_sub;
      cr_logmsg(MSG_STATUS, "Scanning snp block permutations... %7ld (%d scan pts remaining)        ", r_sub * Q, b->n);
      for (l = 0; l < nd; l++) {
        const long j = r_sub * nd + l;
        int bi;
        b->live[l] = tb_trial(j) <= n_perm;
        if (!b->live[l]) continue;
        tp = fh_now();
        bi = tb_get(j);
        D.st.host_perm_s += fh_now() - tp;
        tp = fh_now();
        fh_dev_check(fsclg_slot_set_rows_packed(D.ctx[l], slot, TB.buf[bi], D.rb, TB.nul[bi]), "set rows");
        D.st.host_upload_s += fh_now() - tp;
        fh_dev_check(fsclg_slot_windows(D.ctx[l], slot, b->cells, b->n, eval_range), "window sums");
        fh_dev_check(fsclg_search_submit(D.ctx[l], 2 + slot, slot, b->cells, b->n, eval_range, bp_resl), "search submit");
        D.st.gp_evals += (unsigned long long)b->n;
      }
      r_sub++;
    } else {
      tp_round_t *b = rd + r_done % K;
      const int lo = D.rank * nd;
      double tw = fh_now();
      for (l = 0; l < nd; l++)
        if (b->live[l])
          fh_dev_check(fsclg_search_wait(D.ctx[l], 2 + (int)(r_done % K), b->out + (size_t)(lo + l) * b->n), "search wait");
        else
          memset(b->out + (size_t)(lo + l) * b->n, 0, sizeof(fsclg_point_t) * (size_t)b->n);
      D.st.wait_s += fh_now() - tw;
      fh_exchange_points(b->out, Q * b->n, lo * b->n, (lo + nd) * b->n);
      tb_release((r_done + 1) * nd); /* the round's uploads ran before its searches */
      tw = fh_now();
      for (k = 0; k < Q; k++) { /* the round's trials in order, each point in ascending order */
        const long t = r_done * Q + k;
        const fsclg_point_t *o = b->out + (size_t)k * b->n;
        int any = 0;
        if (t > n_perm) break;
        for (i = 0; i < b->n; i++) {
          scan_pt_t *p = s->scan_pts + b->pt[i];
          tp_draw_t d = {t, b->pt[i]};
          if (p->permute_finished) continue; /* pruned in an earlier trial: later results dropped */
          any = 1;
          fh_trial_apply(p, o[i].clr, o[i].lalpha, b->cells[i].start_pos, save, tp_draw, &d);
        }
        D.st.trials += any;
      }
      D.st.prune_s += fh_now() - tw;
      r_done++;
      if (sigint_agreed()) sigint_dump(s, n_perm); /* every trial applied so far */
    }
  }
  D.st.negj += TB.negj;
  D.st.spec_gen_s += TB.gen_s;
  tb_stop();
  for (k = 0; k < FSCLG_N_SLOTS; k++) { free(rd[k].pt); free(rd[k].cells); free(rd[k].out); }
}

/* what every trial's rows need (the permutation tests and the family-wise pass): the chromosomes
   whose whole-chromosome null sums a trial reads, and the permutation geometry */
static void trial_rows_begin(int eval_range, double scan_width_mb) {
  int i;
  /* a trial's whole-chromosome null sums are read only where the window is the whole chromosome
     (scan-chromosome.c:75-94): the other chromosomes' sums are not computed */
  D.chr_list = fh_malloc(sizeof(int) * (D.n_chr ? D.n_chr : 1), "chromosomes");
  D.n_chr_list = 0;
  for (i = 0; i < D.n_chr; i++)
    if ((long long)D.chr_n[i] <= 2ll * eval_range + 1) D.chr_list[D.n_chr_list++] = i;
  perm_geom(scan_width_mb);
}

/* ... and their end: the original rows are back on every device */
static void trial_rows_end(void) {
  free(D.chr_list);
  D.chr_list = NULL;
  D.n_chr_list = 0;
  fh_set_original_rows();
}

/* entry of a permutation test, after the caller's own refusals and fh_prepare(): the SIGINT window
   and handler, the trials' rows (trial_rows_begin), and (g != NULL: the parity stream) the single
   thread's usleep() draw */
static void permute_begin(int eval_range, double scan_width_mb, fh_rand_t *g) {
  const char *e = getenv("FSCL_AMD_SIGINT_WINDOW_MS");
  struct sigaction sa;
  g_sigint_window = e ? atof(e) / 1e3 : 10.;
  memset(&sa, 0, sizeof sa);
  sa.sa_handler = on_sigint;
  sigemptyset(&sa.sa_mask);
  gettimeofday(&g_last_dump, NULL);
  sigaction(SIGINT, &sa, NULL);
  trial_rows_begin(eval_range, scan_width_mb);
  if (g) (void)fh_rand(g); /* scan-chromosome.c:440 */
}

/* exit of a permutation test begun at time t0 */
static void permute_end(double t0) {
  cr_logmsg(MSG_STATUS, "Scanning snp block permutations... finished.\n");
  signal(SIGINT, SIG_DFL);
  trial_rows_end();
  D.st.permute_s += fh_now() - t0;
}

static int stream_draw(void *g) { return fh_rand(g); }


/* lockstep trials: permute -> rows and null sums to slot 0 of every device -> every active cell ->
   count and prune (scan-chromosome.c:441-502).  all == NULL: a point's trial cell, searched
   (eval_cells); else the grid test: cell all[point], its maximum over the small_grid_sp grid */
static void permute_lockstep(scan_t *s, int n_perm, double permute_nbp, int eval_range, int bp_resl, int large_grid_sp,
                             double scan_width_mb, fh_rand_t *g, int save, const fsclg_cell_t *all, int small_grid_sp) {
  int n_act = s->n_scan_pts, i, k, trial = -1;
  int *act = fh_malloc(sizeof(int) * (n_act ? n_act : 1), "active points");
  fsclg_cell_t *cells = fh_malloc(sizeof(fsclg_cell_t) * (n_act ? n_act : 1), "cells");
  fsclg_point_t *out = fh_malloc(sizeof(fsclg_point_t) * (n_act ? n_act : 1), "points");
  double *nul = fh_malloc(sizeof(double) * (D.n_chr ? D.n_chr : 1), "null sums");
  for (i = 0; i < n_act; i++) act[i] = i;
  for (;;) {
    double tp = fh_now();
    void *prow = slot_stage(0);
    block_permute(prow, D.rowp, s->n_snps, permute_nbp, scan_width_mb, g, &D.st.negj, NULL, 0);
    D.st.host_perm_s += fh_now() - tp;
    trial++;
    for (i = k = 0; i < n_act; i++)
      if (!s->scan_pts[act[i]].permute_finished) act[k++] = act[i];
    n_act = k;
    cr_logmsg(MSG_STATUS, "Scanning snp block permutations... %7d (%d scan pts remaining)        ", trial, n_act);
    if (n_act == 0 || trial > n_perm) break;
    tp = fh_now();
    fh_chr_null_sums(prow, nul);
    D.st.host_null_s += fh_now() - tp;
    tp = fh_now();
    slot_upload(0, nul);
    D.st.host_upload_s += fh_now() - tp;
    for (i = 0; i < n_act; i++) {
      if (all) cells[i] = all[act[i]];
      else trial_cell(s->scan_pts + act[i], large_grid_sp, cells + i);
    }
    tp = fh_now();
    if (all) fh_eval_cell_maxima(0, cells, n_act, small_grid_sp, eval_range, out);
    else fh_eval_cells(cells, n_act, eval_range, bp_resl, out);
    D.st.search_s += fh_now() - tp;
    tp = fh_now();
    D.st.trials++;
    for (i = 0; i < n_act; i++) /* ascending point order */
      fh_trial_apply(s->scan_pts + act[i], out[i].clr, out[i].lalpha, cells[i].start_pos, save, stream_draw, g);
    D.st.prune_s += fh_now() - tp;
    if (sigint_agreed()) sigint_dump(s, n_perm);
  }
  free(act); free(cells); free(out); free(nul);
}

/* scan-chromosome.c:582-652 (with --n-threads=1 pruning semantics) */
void scan_permute(scan_t *s, sm_ptable_t *sm, int n_perm, double permute_nbp, double alpha_factor, int n_threads,
                  int eval_range, int bp_resl, int large_grid_sp, double scan_width_mb) {
  fh_rand_t *g = fh_perm_rng();
  const int save = CLR_NULL_DIST_SAVE; /* scan-chromosome.c:496 */
  const char *e = getenv("FSCL_AMD_PERMUTE"); /* throughput[:seed] overrides the mode set by the API */
  const double t0 = fh_now();
  int i;
  (void)alpha_factor; (void)n_threads; /* -a is inert in the reference too (scan-chromosome.c:584) */
  fh_prepare(s, sm);
  for (i = 0; i < s->n_scan_pts; i++) /* points a caller built without scan_chromosome */
    if (!s->scan_pts[i].permute_clr) s->scan_pts[i].permute_clr = fh_malloc(sizeof(float) * save, "permute_clr");
  if (e && !strncmp(e, "throughput", 10))
    fscl_amd_set_permute_mode(FSCL_AMD_PERMUTE_THROUGHPUT, e[10] == ':' ? strtoull(e + 11, NULL, 0) : g_pseed);
  if (g_pmode == FSCL_AMD_PERMUTE_THROUGHPUT) { /* the rand() stream is not used */
    permute_begin(eval_range, scan_width_mb, NULL);
    permute_throughput(s, n_perm, permute_nbp, eval_range, bp_resl, large_grid_sp, scan_width_mb, save);
  } else {
    permute_begin(eval_range, scan_width_mb, g);
    if (!getenv("FSCL_AMD_LOCKSTEP"))
      permute_pipelined(s, n_perm, permute_nbp, eval_range, bp_resl, large_grid_sp, scan_width_mb, g, save);
    else
      permute_lockstep(s, n_perm, permute_nbp, eval_range, bp_resl, large_grid_sp, scan_width_mb, g, save, NULL, 0);
  }
  permute_end(t0);
}

/* scan-chromosome.c:441-502 with a cell's search_maxpos replaced by its grid maximum on the
   permuted rows, in lockstep: permute -> rows and null sums to slot 0 of every device -> the
   grid maximum of every active cell -> count and prune.  The trial's cell is the point's own
   cell (by cell index): the positions the original statistic was maximised over */
void fscl_amd_scan_permute_grid(scan_t *s, sm_ptable_t *sm, int n_perm, double permute_nbp, int eval_range,
                                int small_grid_sp, int large_grid_sp, double scan_width_mb) {
  fh_rand_t *g = fh_perm_rng();
  const char *e = getenv("FSCL_AMD_PERMUTE");
  const double t0 = fh_now();
  fsclg_cell_t *all;
  int n_cells = 0;
  if (D.world > 1)
    logmsg(MSG_FATAL, "fscl_amd: the grid permutation test runs in one process (not with %d ranks)", D.world);
  if (g_pmode == FSCL_AMD_PERMUTE_THROUGHPUT || (e && !strncmp(e, "throughput", 10)))
    logmsg(MSG_FATAL, "fscl_amd: the grid permutation test runs on the parity stream only (not in throughput mode)");
  fh_prepare(s, sm);
  if (!fh_grid_points_are(s, small_grid_sp, large_grid_sp))
    logmsg(MSG_FATAL, "fscl_amd: the grid permutation test needs the points of fscl_amd_scan_chromosome_grid with the "
                      "same spacings (-g %d -G %d)", small_grid_sp, large_grid_sp);
  all = fh_scan_cells(s, large_grid_sp, &n_cells);
  if (n_cells != s->n_scan_pts) logmsg(MSG_FATAL, "fscl_amd: grid permutation test: %d cells, %d points", n_cells, s->n_scan_pts);
  permute_begin(eval_range, scan_width_mb, g);
  permute_lockstep(s, n_perm, permute_nbp, eval_range, 0, large_grid_sp, scan_width_mb, g, CLR_NULL_DIST_SAVE, all,
                   small_grid_sp);
  free(all);
  permute_end(t0);
}

/* ------------------------------------------------------ family-wise adjusted p-values (--familywise-file)
   Unpruned permutation trials (the throughput mode's permutations, every point in every trial) and
   their reduction by fsclg_maxt_submit on the first device.  The host-only pieces are in
   familywise.c. */
static double g_fw_ms;
double fscl_amd_familywise_last_ms(void) { return g_fw_ms; }

static int familywise_refuse(int code, const char *fmt, ...) {
  char msg[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof msg, fmt, ap);
  va_end(ap);
  fh_familywise_set_error(msg);
  return code;
}

/* The reduction of T, chunk by chunk, on batch 0 of the first device: a full chunk is submitted (the
   shim copies it, so its buffer is free again) and waited for only before the next one is submitted
   or at the end, so that the trials go on meanwhile.  The maxima land at their trials; the counts of
   the chunks are added (integers: any chunking gives the same sums). */
typedef struct {
  int m, G;
  const double *obs;
  const int32_t *order, *group;
  double *gmax, *grp_max;
  int32_t *garg, *grp_arg, *c_single, *c_chr, *c_step;
  int32_t *tmp;     /* [3 m]: one chunk's counts */
  int pending, t0;  /* a chunk is submitted: its first trial */
} maxt_acc_t;

static int maxt_drain(maxt_acc_t *A) {
  const size_t m = (size_t)A->m;
  size_t i;
  int r;
  if (!A->pending) return FSCLG_OK;
  A->pending = 0;
  r = fsclg_maxt_wait(D.ctx[0], 0, A->gmax + A->t0, A->garg + A->t0, A->grp_max + (size_t)A->t0 * (size_t)A->G,
                      A->grp_arg + (size_t)A->t0 * (size_t)A->G, A->tmp, A->tmp + m, A->tmp + 2 * m);
  g_fw_ms += fsclg_maxt_last_ms(D.ctx[0], 0);
  if (r != FSCLG_OK) return r;
  for (i = 0; i < m; i++) {
    A->c_single[i] += A->tmp[i];
    A->c_chr[i] += A->tmp[m + i];
    A->c_step[i] += A->tmp[2 * m + i];
  }
  return FSCLG_OK;
}

static int maxt_push(maxt_acc_t *A, const double *chunk, int t0, int n) {
  int r = maxt_drain(A);
  if (r != FSCLG_OK) return r;
  r = fsclg_maxt_submit(D.ctx[0], 0, chunk, n, A->m, A->obs, A->order, A->group, A->G);
  if (r == FSCLG_OK) { A->pending = 1; A->t0 = t0; }
  return r;
}

int fscl_amd_familywise_runs(const double *clr, int n_trials, int m, const double *obs, const int32_t *order,
                             const int32_t *group, int n_groups, double *gmax, int32_t *garg, double *grp_max,
                             int32_t *grp_arg, int32_t *c_single, int32_t *c_chr, int32_t *c_step) {
  maxt_acc_t A;
  int B, t0, r = FSCLG_OK;
  fh_familywise_set_error("");
  g_fw_ms = 0.0;
  if (n_trials < 0 || m < 0 || n_groups < 0 || (m && (!obs || !order || !group || !c_single || !c_chr || !c_step)) ||
      (n_trials && (!gmax || !garg || (m && !clr))) || (n_trials && n_groups && (!grp_max || !grp_arg)))
    return familywise_refuse(FSCLG_E_ARG, "a NULL argument or a negative size");
  if (m) { memset(c_single, 0, sizeof(int32_t) * (size_t)m); memset(c_chr, 0, sizeof(int32_t) * (size_t)m); memset(c_step, 0, sizeof(int32_t) * (size_t)m); }
  if (n_trials == 0) return FSCLG_OK;
  B = fscl_amd_familywise_chunk(m, n_trials, fscl_amd_familywise_cap());
  if (B < 1)
    return familywise_refuse(FSCLG_E_ARG, "one trial of %d points does not fit in FSCL_AMD_FWER_CAP=%zu bytes", m, fscl_amd_familywise_cap());
  fh_dev_open();
  memset(&A, 0, sizeof A);
  A.m = m; A.G = n_groups; A.obs = obs; A.order = order; A.group = group;
  A.gmax = gmax; A.garg = garg; A.grp_max = grp_max; A.grp_arg = grp_arg;
  A.c_single = c_single; A.c_chr = c_chr; A.c_step = c_step;
  A.tmp = fh_malloc(sizeof(int32_t) * 3 * (size_t)(m ? m : 1), "familywise counts");
  for (t0 = 0; t0 < n_trials && r == FSCLG_OK; t0 += B)
    r = maxt_push(&A, clr + (size_t)t0 * (size_t)m, t0, n_trials - t0 < B ? n_trials - t0 : B);
  if (r == FSCLG_OK) r = maxt_drain(&A);
  else (void)maxt_drain(&A);
  free(A.tmp);
  if (r != FSCLG_OK) familywise_refuse(r, "%s", fsclg_last_error());
  return r;
}

int fscl_amd_familywise(scan_t *s, sm_ptable_t *sm, int trials, unsigned long long seed, double permute_nbp,
                        int eval_range, int bp_resl, int large_grid_sp, double scan_width_mb, int keep_matrix,
                        fscl_amd_familywise_t *out) {
  const double t_begin = fh_now();
  const unsigned long long seed_saved = g_pseed;
  maxt_acc_t A;
  fsclg_cell_t *cells;
  fsclg_point_t *pts;
  double *obs, *chunk;
  int32_t *group;
  long r_sub = 0, r_done = 0, R;
  int m, G, B, nd, K, i, l, c0 = 0, rc = FSCLG_OK;
  if (!s || !sm || !out) return FSCLG_E_ARG;
  memset(out, 0, sizeof *out);
  fh_familywise_set_error("");
  g_fw_ms = 0.0;
  if (trials < 1) return familywise_refuse(FSCLG_E_ARG, "--familywise-trials must be at least 1");
  if (large_grid_sp < 1) return familywise_refuse(FSCLG_E_ARG, "the coarse grid spacing must be positive");
  if (D.world > 1) return familywise_refuse(FSCLG_E_STATE, "--familywise-file runs in one process (not with %d ranks)", D.world);
  m = s->n_scan_pts > 0 ? s->n_scan_pts : 0;
  G = s->n_chromosomes > 0 ? s->n_chromosomes : 0;
  if (G > FSCLG_MAXT_MAX_GROUPS)
    return familywise_refuse(FSCLG_E_ARG, "%d chromosomes: more than the %d the family-wise maxima take", G, FSCLG_MAXT_MAX_GROUPS);
  B = fscl_amd_familywise_chunk(m, trials, fscl_amd_familywise_cap());
  if (B < 1)
    return familywise_refuse(FSCLG_E_ARG, "one trial of %d points does not fit in FSCL_AMD_FWER_CAP=%zu bytes", m, fscl_amd_familywise_cap());
  fh_prepare(s, sm);
  nd = D.n_dev;
  K = fh_env_int("FSCL_AMD_DEPTH", nd >= 4 ? 2 : FSCLG_N_SLOTS / nd, 1, FSCLG_N_SLOTS);
  R = ((long)trials + nd - 1) / nd; /* rounds: trial r * nd + l on local device l */
  out->n = m; out->n_groups = G; out->trials = trials; out->seed = seed;
  out->order = fh_malloc(sizeof(int32_t) * (size_t)(m ? m : 1), "familywise order");
  out->c_single = fh_calloc((size_t)(m ? m : 1), sizeof(int32_t), "familywise counts");
  out->c_chr = fh_calloc((size_t)(m ? m : 1), sizeof(int32_t), "familywise counts");
  out->c_step = fh_calloc((size_t)(m ? m : 1), sizeof(int32_t), "familywise counts");
  out->gmax = fh_malloc(sizeof(double) * (size_t)trials, "familywise maxima");
  out->garg = fh_malloc(sizeof(int32_t) * (size_t)trials, "familywise maxima");
  out->chr_max = fh_malloc(sizeof(double) * (size_t)trials * (size_t)(G ? G : 1), "familywise maxima");
  out->chr_arg = fh_malloc(sizeof(int32_t) * (size_t)trials * (size_t)(G ? G : 1), "familywise maxima");
  if (keep_matrix) out->matrix = fh_malloc(sizeof(double) * (size_t)trials * (size_t)(m ? m : 1), "familywise matrix");
  obs = fh_malloc(sizeof(double) * (size_t)(m ? m : 1), "familywise observed");
  group = fh_malloc(sizeof(int32_t) * (size_t)(m ? m : 1), "familywise groups");
  cells = fh_malloc(sizeof(fsclg_cell_t) * (size_t)(m ? m : 1), "cells");
  chunk = fh_malloc(sizeof(double) * (size_t)B * (size_t)(m ? m : 1), "familywise chunk");
  pts = fh_malloc(sizeof(fsclg_point_t) * (size_t)K * (size_t)nd * (size_t)(m ? m : 1), "points");
  for (i = 0; i < m; i++) {
    const scan_pt_t *q = s->scan_pts + i;
    obs[i] = q->clr;
    group[i] = q->chr;
    trial_cell(q, large_grid_sp, cells + i); /* the same in every trial */
  }
  fscl_amd_familywise_order(obs, m, out->order);
  memset(&A, 0, sizeof A);
  A.m = m; A.G = G; A.obs = obs; A.order = out->order; A.group = group;
  A.gmax = out->gmax; A.garg = out->garg; A.grp_max = out->chr_max; A.grp_arg = out->chr_arg;
  A.c_single = out->c_single; A.c_chr = out->c_chr; A.c_step = out->c_step;
  A.tmp = fh_malloc(sizeof(int32_t) * 3 * (size_t)(m ? m : 1), "familywise counts");
  /* the throughput mode's builders under this pass's seed: trial t is its trial t */
  g_pseed = seed;
  trial_rows_begin(eval_range, scan_width_mb);
  tb_start(nd, nd, 0, (long)trials - 1, R * nd, K, s, permute_nbp, scan_width_mb);
  while (r_done < r_sub || r_sub < R) {
    if (r_sub < R && r_sub - r_done < K) { /* a round's trials: rows, window sums and every cell, per device */
      const int slot = (int)(r_sub % K);
      cr_logmsg(MSG_STATUS, "Family-wise maxima: unpruned permutation trials... %7ld of %d        ", r_sub * nd, trials);
      for (l = 0; l < nd; l++) {
        const long j = r_sub * nd + l;
        int bi;
        if (j >= trials) continue;
        bi = tb_get(j);
        fh_dev_check(fsclg_slot_set_rows_packed(D.ctx[l], slot, TB.buf[bi], D.rb, TB.nul[bi]), "set rows");
        fh_dev_check(fsclg_slot_windows(D.ctx[l], slot, cells, m, eval_range), "window sums");
        fh_dev_check(fsclg_search_submit(D.ctx[l], 2 + slot, slot, cells, m, eval_range, bp_resl), "search submit");
      }
      r_sub++;
    } else { /* the oldest round, its trials in order: each one's CLRs are a row of the chunk */
      const int slot = (int)(r_done % K);
      fsclg_point_t *o = pts + (size_t)slot * (size_t)nd * (size_t)(m ? m : 1);
      for (l = 0; l < nd; l++)
        if (r_done * nd + l < trials) fh_dev_check(fsclg_search_wait(D.ctx[l], 2 + slot, o + (size_t)l * (size_t)m), "search wait");
      tb_release((r_done + 1) * nd); /* the round's uploads ran before its searches */
      for (l = 0; l < nd; l++) {
        const long t = r_done * nd + l;
        double *row;
        if (t >= trials) continue;
        row = chunk + (size_t)(t - c0) * (size_t)m;
        for (i = 0; i < m; i++) row[i] = o[(size_t)l * (size_t)m + i].clr;
        if (out->matrix && m) memcpy(out->matrix + (size_t)t * (size_t)m, row, sizeof(double) * (size_t)m);
        if (t - c0 + 1 == B || t == trials - 1) {
          if (rc == FSCLG_OK) rc = maxt_push(&A, chunk, c0, (int)(t - c0 + 1));
          c0 = (int)t + 1;
        }
      }
      r_done++;
    }
  }
  if (rc == FSCLG_OK) rc = maxt_drain(&A);
  else (void)maxt_drain(&A);
  cr_logmsg(MSG_STATUS, "Family-wise maxima: unpruned permutation trials... finished.\n");
  tb_stop();
  g_pseed = seed_saved;
  trial_rows_end();
  free(A.tmp); free(obs); free(group); free(cells); free(chunk); free(pts);
  out->kernel_ms = g_fw_ms;
  if (rc != FSCLG_OK) {
    familywise_refuse(rc, "%s", fsclg_last_error());
    fscl_amd_familywise_free(out);
  }
  out->wall_s = fh_now() - t_begin;
  return rc;
}
