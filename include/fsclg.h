/*
 * fsclg.h -- device shim C-ABI of the MI355X (gfx950) CLR scan kernels.
 *
 * Plain C, plain pointers and sizes, int status returns, no exceptions and no
 * torch types cross this boundary.  One context per process per GPU.  It sits
 * below the fscl.h-compatible host library (include/fscl_amd.h): the host C
 * code (scan_chromosome / scan_permute) calls these; a maintainer can also
 * bind them directly (ctypes stub in INTEGRATION.md).
 *
 * Reference interfaces each entry replaces (all in /root/reference):
 *   fsclg_search_maxpos  -> search_maxpos() batch, scan-chromosome.c:126-139
 *                           (with init_scan_result :58-101, search_maxalpha
 *                           sm-search.c:269-300, sm_likelihood :105-150)
 *   fsclg_search_points  -> search_maxalpha() on caller-initialised points,
 *                           sm-search.c:269-300 (fscl.h:105)
 *   fsclg_set_rows       -> the permuted snp array of one trial,
 *                           scan-chromosome.c:443 (snp_block_permute output)
 *   fsclg_slot_set_rows  -> the same for one of FSCLG_N_SLOTS trials in flight
 *   fsclg_slot_set_rows_plan -> snp_block_permute itself (scan-chromosome.c:336-389)
 *                           applied on the device from the host's block plan
 *   fsclg_search_submit/ -> the per-trial search_maxpos calls of
 *   fsclg_search_wait       scan_permute_thread (scan-chromosome.c:478-487),
 *                           split so that consecutive trials overlap on the GPU
 *   fsclg_upload_tables  -> sm_ptable_t spline tables (fscl.h:64-76) and
 *                           log_table (sm-search.c:14-26)
 *   fsclg_upload_snps    -> snp_t positions + chr_limits_t (fscl.h:7-33)
 */
#ifndef FSCLG_H
#define FSCLG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FSCLG_OK = 0,
  FSCLG_E_ARG = -1,        /* bad argument / shape */
  FSCLG_E_HIP = -2,        /* HIP runtime error (message in fsclg_last_error) */
  FSCLG_E_STATE = -3,      /* tables / snps not uploaded */
  FSCLG_E_UNSUPPORTED = -4,/* a window narrower than its chromosome (chromosome > 2*eval_range+1 SNPs) */
  FSCLG_E_KERNEL = -5      /* device-side failure flag (e.g. position bisection did not converge) */
};

typedef struct fsclg_ctx fsclg_ctx;

/* one coarse grid cell: search_maxpos(chr, start_pos, end_pos) */
typedef struct {
  int32_t chr, start_pos, end_pos, pad;
} fsclg_cell_t;

/* one evaluated scan point (the fields of scan_pt_t the path produces) */
typedef struct {
  int32_t chr, nearest_snp, sweep_pos, n_snps, window_start, window_end, flags;
  uint32_t cost;  /* out: snp_likelihood terms / 1024 spent on this point's cell (scheduling hint) */
  double lalpha, null_logl, sm_logl, clr;
} fsclg_point_t;

/* cumulative device counters (reset by fsclg_reset_stats) */
typedef struct {
  unsigned long long n_terms;      /* snp_likelihood evaluations */
  unsigned long long n_null;       /* window null-sum elements (reference-equivalent count) */
  unsigned long long n_walks;      /* sm_likelihood walks */
  unsigned long long n_maxalpha;   /* search_maxalpha evaluations */
  unsigned long long n_unsafe;     /* walks whose integer-ulp sum left its binade */
  unsigned long long n_slow;       /* walks re-summed sequentially to settle an argmax */
  unsigned long long n_ties;       /* round-half-even ties resolved by prefix parity */
  unsigned long long n_cells;      /* search_maxpos evaluations */
  double kernel_ms;                /* summed duration of the search kernels (HIP events) */
  unsigned long long n_launches;
  int cache_iv0, cache_n_iv, cache_n_rows;  /* LDS coefficient window: intervals, device rows */
  double cache_cover;              /* its planned share of the terms */
  double window_ms;                /* summed duration of the window null-sum kernels (HIP events) */
  unsigned long long n_dup_cells;  /* cells answered by an identical cell of the same launch */
  unsigned long long n_ep_saved;   /* endpoint evaluations saved by sharing between neighbouring cells */
  double busy_ms;                  /* union of the search batches' kernel intervals (overlapping batches
                                      counted once): the GPU time the search kernels occupied */
  unsigned long long n_split_retry; /* split launches whose members were not resident together (a
                                       member waited > ~1 s), re-run with one workgroup per cell */
} fsclg_stats_t;

/* trials in flight: row slots (one permuted row array + null sums each) and launch batches
   (cells and outputs each).  Batches 0 and 1 run on one high-priority stream, batches
   2 .. FSCLG_N_BATCHES-1 on two normal-priority streams (even / odd batch): with the upload
   stream, four streams, one per hardware queue (GPU_MAX_HW_QUEUES = 4) */
#define FSCLG_N_SLOTS 8
#define FSCLG_N_BATCHES 10

int fsclg_open(int device, fsclg_ctx **out);
int fsclg_close(fsclg_ctx *c);
const char *fsclg_last_error(void);
int fsclg_device_count(void);

/* log_table: 65536 doubles (log_table[0] = 0, log_table[i] = log(i));
   coef: n_rows * n_iv * 4 doubles, row-major [row][interval][c0..c3];
   nullrow: n_rows doubles (null_logl of a site with that row);
   log_ad_step = (LOG_AD_MAX - LOG_AD_MIN) / (spline_pts + 1) */
int fsclg_upload_tables(fsclg_ctx *c, const double *log_table, const double *coef, int n_rows, int n_iv,
                        const double *nullrow, double log_ad_step);

/* pos: n_snps int32 sorted within each chromosome; row: n_snps uint32 (spline row of each site);
   chr_start/chr_n: first index and SNP count of each chromosome */
int fsclg_upload_snps(fsclg_ctx *c, const int32_t *pos, const uint32_t *row, int n_snps,
                      const int32_t *chr_start, const int32_t *chr_n, int n_chr);

/* replace the per-site rows (one permutation trial); NULL restores the uploaded rows */
/* a pinned host buffer of n_snps rows owned by the context (valid until the next
   fsclg_upload_snps / fsclg_close): a caller that permutes into it saves one copy in
   fsclg_set_rows (the buffer may be rewritten once fsclg_set_rows's search has returned) */
uint32_t *fsclg_row_buffer(fsclg_ctx *c);
int fsclg_set_rows(fsclg_ctx *c, const uint32_t *row);

/* asynchronous trials.  A row slot holds one trial's rows on the device; a batch is one
   search_maxpos launch over the rows of one slot.  fsclg_slot_row_buffer returns the slot's
   pinned staging buffer (NULL while a batch submitted on the slot is not waited for);
   fsclg_slot_set_rows uploads it (or row, or the uploaded rows when row is NULL) and, when
   chr_null is not NULL, the slot's whole-chromosome null sums; both are asynchronous and
   fail with FSCLG_E_STATE while the slot is in use.  fsclg_search_submit queues a batch
   (cells are copied; the batch must be idle) and returns at once; fsclg_search_wait blocks
   until its points are in out[n_cells] (input order).  Slot 0 and batch 0 are also what the
   synchronous calls (fsclg_set_rows, fsclg_search_maxpos) use. */
uint32_t *fsclg_slot_row_buffer(fsclg_ctx *c, int slot);
int fsclg_slot_set_rows(fsclg_ctx *c, int slot, const uint32_t *row, const double *chr_null);
/* the window null sums (chromosomes above 2*eval_range+1 SNPs) for the cells that the slot's
   next batches will evaluate, given before the slot's first submit of a trial: only those
   windows when they are few, every window otherwise.  A submit checks its cells against what
   was summed and sums any window still missing (also without this call), so a batch may
   submit other cells too, at the cost of a second window launch. */
int fsclg_slot_windows(fsclg_ctx *c, int slot, const fsclg_cell_t *cells, int n_cells, int eval_range);
int fsclg_search_submit(fsclg_ctx *c, int batch, int slot, const fsclg_cell_t *cells, int n_cells, int eval_range,
                        int bp_resl);
int fsclg_search_wait(fsclg_ctx *c, int batch, fsclg_point_t *out);

/* Several devices fed from one host buffer.  fsclg_host_alloc returns pinned host memory that
   every device's kernels read directly (portable, mapped, coherent); fsclg_slot_set_rows_host
   uploads a slot's rows straight from such a buffer (no copy into the context's own staging,
   no range check: every row must be < the n_rows of fsclg_upload_tables) and returns at once;
   the caller keeps the buffer unchanged until fsclg_slot_wait(c, slot) has returned on every
   context it was handed to (the slot's last upload has read it). */
void *fsclg_host_alloc(size_t bytes);
void fsclg_host_free(void *p);
/* The same for memory the caller mapped itself (a POSIX shared-memory segment that several
   processes map: one node leader builds each trial's rows once, every rank's devices read
   them): page-locks [p, p + bytes) for every device (portable, mapped).  Returns FSCLG_OK only
   if the devices address the memory by the same pointer (the pointer can go to
   fsclg_slot_set_rows_packed as it is); fsclg_host_unregister undoes it. */
int fsclg_host_register(void *p, size_t bytes);
int fsclg_host_unregister(void *p);
int fsclg_slot_wait(fsclg_ctx *c, int slot);
/* exchange two slots' device state (rows, window sums, their upload events): a trial prepared in
   a spare slot ahead of time becomes slot a.  Neither slot may have a batch not waited for. */
int fsclg_slot_swap(fsclg_ctx *c, int a, int b);
/* 1 if the batch's last submit has completed (or none is pending), 0 if it is still running:
   fsclg_search_wait would not block */
int fsclg_search_done(fsclg_ctx *c, int batch);
int fsclg_slot_set_rows_host(fsclg_ctx *c, int slot, const uint32_t *row, const double *chr_null);
/* the same with rows of row_bytes = 1, 2 or 4 bytes each (1: n_rows <= 256, 2: n_rows <= 65536):
   a narrower staging is fewer PCIe bytes for every device's upload of every trial */
int fsclg_slot_set_rows_packed(fsclg_ctx *c, int slot, const void *row, int row_bytes, const double *chr_null);

/* A trial's block permutation as a plan, applied on the device (scan-chromosome.c:336-389:
   snp_block_permute's swaps, from the rand() stream, on the uploaded rows).  The host draws the
   blocks and groups them (fh_plan_build, fscl_amd/csrc/host/perm.c); the device copies the
   uploaded rows into the slot and applies the groups in order.  Within a group the entries touch
   disjoint sites, so they run in any order.  kind 0: rows[i + t] <-> rows[j + t] for t < len, the
   two ranges disjoint (a block, or a piece of one).  kind 1: a block whose ranges overlap,
   |i - j| < len, the reference's sequential element swaps (a rotation of [min(i,j), min(i,j) +
   len + |i - j|)), alone in its group.  ent and grp (n_grp + 1 offsets into ent) are host
   memory the devices read directly (fsclg_host_alloc or fsclg_host_register) and must stay
   unchanged until fsclg_slot_wait(c, slot) returns; only the chr_null values are copied.
   Validation is at call time only, on the buffers as they are then: every range is checked
   against n_snps, and a kind-0 entry's own two ranges for disjointness.  That the entries of one
   group touch disjoint sites is the CALLER's contract (fh_plan_build guarantees it by
   construction); entries that overlap across a group race on those sites without an error,
   though never outside [0, n_snps). */
typedef struct {
  int32_t i, j, len, kind;
} fsclg_swap_t;
int fsclg_slot_set_rows_plan(fsclg_ctx *c, int slot, const fsclg_swap_t *ent, const int32_t *grp, int n_grp,
                             const double *chr_null);

/* sequential window null sums (init_scan_result's sum from 0.0) for each chromosome's
   whole-chromosome window, for the rows currently set */
int fsclg_set_chr_null(fsclg_ctx *c, const double *chr_null);

/* alpha grids: coarse (11 values of the for-loop at sm-search.c:277) and, for each
   coarse argmax index c in [0, n_coarse), the refine values of sm-search.c:283-295
   (max 16 each, row-major [c][16]); row n_coarse holds the refine values around
   LOG_AD_MAX, used when no candidate beats the initial -DBL_MAX (sm-search.c:272) */
int fsclg_set_alpha_grid(fsclg_ctx *c, const double *coarse, int n_coarse, const double *refine,
                         const int32_t *n_refine);

/* Split cells: a launch of batch `batch` with few cells gives each cell up to max_members
   (<= 8) workgroups that share its walks' segments (default 1).  For latency, not throughput:
   the pipeline's blocking batch, whose result orders the next trial.  A launch takes at most
   512 workgroups ($FSCLG_SPLIT_BUDGET), the device's resident slots, so the members of a cell
   run together once the workgroups ahead of them finish; a cell whose members were not all
   resident within ~1 s is re-run with one workgroup (counted, n_split_retry). */
int fsclg_set_batch_split(fsclg_ctx *c, int batch, int max_members);

/* batched search_maxpos over n_cells cells; blocks until out[] is written */
int fsclg_search_maxpos(fsclg_ctx *c, const fsclg_cell_t *cells, int n_cells, int eval_range, int bp_resl,
                        fsclg_point_t *out);

/* search_maxalpha on points whose chr/nearest_snp/sweep_pos/window/null_logl are
   already set (init_scan_result done by the caller); fills lalpha/sm_logl/clr */
int fsclg_search_points(fsclg_ctx *c, fsclg_point_t *pts, int n_pts);

/* Likelihood profile: init_scan_result + search_maxalpha at every position of dense runs
   (the reference's disabled fine-grid loop, scan-chromosome.c:269-327).  A run is the positions
   start_pos + k * step, k < count, of one chromosome; out holds sum(count) points in run order,
   then position order, each what init_scan_result(chr, pos) followed by search_maxalpha gives on
   the UPLOADED rows (the call restores them into slot 0; the whole-chromosome null sums are the
   caller's, fsclg_set_chr_null, the window null sums are summed here).  sweep_pos is the
   position after init_scan_result's de-collision; cost is the terms / 1024 the point's chunk
   had spent when the point was stored.  The profile kernel gives one workgroup a chunk of
   fsclg_profile_chunk() consecutive positions of a run ($FSCLG_PROFILE_CHUNK, default 16).
   Synchronous, on batch 0 and slot 0 like fsclg_search_points; fsclg_profile_submit /
   fsclg_profile_wait are its two halves (several devices at once).  FSCLG_E_ARG: step < 1,
   count < 0, a bad chr, a position past the int range; FSCLG_E_STATE: tables or SNPs not
   uploaded, batch 0 pending.  fsclg_profile_last_ms: the profile kernel's own time (HIP
   events) of the context's last profile; the device counters accumulate as for any launch. */
typedef struct {
  int32_t chr, start_pos, step, count;
} fsclg_run_t;
int fsclg_profile(fsclg_ctx *c, const fsclg_run_t *runs, int n_runs, int eval_range, fsclg_point_t *out);
int fsclg_profile_submit(fsclg_ctx *c, const fsclg_run_t *runs, int n_runs, int eval_range);
int fsclg_profile_wait(fsclg_ctx *c, fsclg_point_t *out);
int fsclg_profile_chunk(void);
double fsclg_profile_last_ms(fsclg_ctx *c);

/* Cell maxima: the first position of strictly greatest clr of each run (the reference's disabled
   fine-grid loops: the scan's, scan-chromosome.c:269-296, `>` at :287, and the trial's, :505-523),
   on the rows a slot HOLDS -- whatever fsclg_slot_set_rows* put there, e.g. one trial's
   permutation -- with the slot's whole-chromosome null sums; the window null sums are summed
   here, for the slot's rows.  out holds n_runs points in run order, each the point
   fsclg_profile gives at that position on the same rows; a run with count == 0 yields a zeroed
   point (n_snps = 0).  The kernel takes fsclg_profile's chunks (fsclg_profile_chunk() positions,
   one workgroup each) and stores one point per chunk, the chunk's first strict maximum; the wait
   folds a run's chunk maxima in chunk order with the same `>`.  cost is the terms / 1024 of the
   run's chunks.  Asynchronous, like fsclg_search_submit / fsclg_search_wait, on any batch and
   slot (runs are copied; the batch must be idle; several devices: submit to all, then wait).
   FSCLG_E_ARG: step < 1, count < 0, a bad chr, batch or slot, a position past the int range;
   FSCLG_E_STATE: tables or SNPs not uploaded, the batch pending (submit), no cell maxima
   submitted on it (wait).  fsclg_cellmax_last_ms: the kernel's own time (HIP events) of the
   batch's last launch; the device counters accumulate as for any launch. */
int fsclg_cellmax_submit(fsclg_ctx *c, int batch, int slot, const fsclg_run_t *runs, int n_runs, int eval_range);
int fsclg_cellmax_wait(fsclg_ctx *c, int batch, fsclg_point_t *out);
double fsclg_cellmax_last_ms(fsclg_ctx *c, int batch);

/* Alpha likelihood curves: every composite likelihood search_maxalpha (sm-search.c:269-300)
   evaluates at a position -- the 11 coarse alphas, then the refine list around the coarse winner
   (or around LOG_AD_MAX when no coarse candidate beat the initial -DBL_MAX) -- in the
   reference's evaluation order.  sm[k] is what sm_likelihood (sm-search.c:105-150) returns for
   la[k]: the null sum plus the terms in walk order, the exact sequential sum for every entry,
   also for the candidates whose value the argmax never needed exactly; entries past
   n_coarse + n_refine are zero.  pt is the point fsclg_profile gives at the position, on the
   same rows, bit for bit: the first strict maximum of sm[] in order, from the reference's
   -DBL_MAX / LOG_AD_MAX state, is (pt.sm_logl, pt.lalpha).
   fsclg_curve_submit / fsclg_curve_wait take runs, batches, slots and window null sums exactly
   as fsclg_cellmax_submit / fsclg_cellmax_wait do, and give one record per position, in run
   order, then position order (out holds sum(count) records).  Further errors: FSCLG_E_ARG for an
   alpha grid with more than 11 coarse values.  fsclg_curve_last_ms: the kernel's own time (HIP
   events) of the batch's last curve launch.  fsclg_curve_forced: the walks summed sequentially
   only because a curve wants every value exact (beyond n_slow, which still counts those an
   argmax needed), since fsclg_open or fsclg_reset_stats. */
#define FSCLG_CURVE_MAX 27 /* 11 coarse + 16 refine candidates at most */
typedef struct {
  fsclg_point_t pt;
  int32_t n_coarse, n_refine;
  double la[FSCLG_CURVE_MAX];
  double sm[FSCLG_CURVE_MAX];
} fsclg_curve_t;
int fsclg_curve_submit(fsclg_ctx *c, int batch, int slot, const fsclg_run_t *runs, int n_runs, int eval_range);
int fsclg_curve_wait(fsclg_ctx *c, int batch, fsclg_curve_t *out);
double fsclg_curve_last_ms(fsclg_ctx *c, int batch);
unsigned long long fsclg_curve_forced(fsclg_ctx *c);

/* Likelihood surfaces: the composite likelihood at every position of dense runs for every log alpha
   of a list, no alpha search.  Run i has its own list la[i * n_la .. (i + 1) * n_la), 1 <= n_la <= 64
   values, strictly ascending, each finite and in [LOG_AD_MIN, LOG_AD_MAX] = [-20, 4].
   sm[p * n_la + k] (position-major; p counts the positions in run order, then position order) is what
   sm_likelihood (sm-search.c:105-150) returns for la[k] at position p: the null sum plus the walk's
   terms added one by one in walk order -- the nearest SNP, then leftwards, then rightwards, cut where
   log(alpha d) > LOG_AD_MAX -- bit for bit; an empty walk gives null_logl.  pts[p] is what
   init_scan_result gives at the position on the slot's rows (the de-collided sweep_pos, nearest_snp,
   the window, n_snps, null_logl) with (lalpha, sm_logl) the first strict maximum of the position's
   row in list order from the reference's (LOG_AD_MAX, -DBL_MAX) state -- a row of NaN alone leaves
   that state -- clr = 2 * (sm_logl - null_logl), and cost the terms / 1024 of the row's walks.  Every
   byte of pts[0 .. sum(count)) and sm[0 .. sum(count) * n_la) is written.
   fsclg_surface_submit / fsclg_surface_wait take runs, batches, slots and window null sums exactly as
   fsclg_curve_submit / fsclg_curve_wait do (any batch and slot; the runs and lists are copied; several
   devices: submit to all, then wait).  The same input gives the same bytes on every batch and slot
   and however the kernel chunks the runs (every sum has a fixed order, nothing is accumulated across
   workgroups).  FSCLG_E_ARG: n_la outside [1, 64], an alpha outside the range, NaN, or not above its
   predecessor, step < 1, count < 0, a bad chr, batch or slot, a position past the int range;
   FSCLG_E_STATE: tables or SNPs not uploaded, the batch pending (submit), no surfaces submitted on
   it (wait).  fsclg_surface_last_ms: the kernel's own time (HIP events) of the batch's last surface
   launch.  The device counters count the walks (n_terms, n_null, n_walks); the alpha grid of
   fsclg_set_alpha_grid is not used. */
int fsclg_surface_submit(fsclg_ctx *c, int batch, int slot, const fsclg_run_t *runs, int n_runs,
                         const double *la /* [n_runs][n_la] */, int n_la, int eval_range);
int fsclg_surface_wait(fsclg_ctx *c, int batch, fsclg_point_t *pts /* sum(count) */,
                       double *sm /* sum(count) * n_la, position-major */);
double fsclg_surface_last_ms(fsclg_ctx *c, int batch);

/* Block sums of the surface: the surface's terms summed per contiguous genomic block, the input of a
   delete-one-block jackknife.  Runs, alpha lists, batch, slot, eval_range and window null sums are
   fsclg_surface_submit's; run i also has blk[i]: block_bp >= 1, a first block id b0 >= 0 and a block
   count nb in [1, 1024].  A site at position x belongs to block j = clamp(x / block_bp - b0, 0, nb - 1)
   (integer division): the first and the last block absorb whatever lies beyond them, no term is ever
   dropped.  With item(p, j) = (the (position, block) pairs of the positions before p, runs in order) +
   j, and cell(p, j, k) = item(p, j) * n_la + k -- position-major, then block, then alpha --
     bs[cell]   the strictly sequential sum, from +0.0 and in ascending site index, of the terms of the
                walk of sm_likelihood at position p and la[k] whose sites lie in block j (+0.0: none);
     cnt[cell]  the number of those terms;
     pts[p]     what init_scan_result gives at the position, with (lalpha, sm_logl) the first strict
                maximum, in list order from the reference's (LOG_AD_MAX, -DBL_MAX) state, of V[p][k] +
                null_logl, V[p][k] the sum of bs[p][0 .. nb)[k] in ascending j from +0.0, clr = 2 V at
                that maximum (2 (sm_logl - null_logl) when nothing beat the state), cost the terms /
                1024 of the position's walks.
   The terms are the values fsclg_sites_wait stores for the same walk, and the walk's sites are its
   [nearest - nl, nearest + nr]; an alpha whose nearest SNP is already outside log(alpha d) <=
   LOG_AD_MAX has cnt = 0 everywhere.  Every byte of the three outputs is written.  The same input
   gives the same bytes on every batch and slot and however the kernel chunks the runs (every sum has
   a fixed order, nothing is accumulated across workgroups, no atomic is on the result path).
   Error codes as fsclg_surface_submit's, and FSCLG_E_ARG for block_bp < 1, b0 < 0, nb outside
   [1, 1024] or more cells than an int of bytes addresses; FSCLG_E_STATE from the wait when the batch
   holds no block sums.  fsclg_blocks_last_ms: the kernel's own time of the batch's last launch. */
typedef struct {
  int32_t block_bp, b0, nb, pad;
} fsclg_blocks_t;
int fsclg_blocks_submit(fsclg_ctx *c, int batch, int slot, const fsclg_run_t *runs, int n_runs,
                        const double *la /* [n_runs][n_la] */, int n_la, const fsclg_blocks_t *blk /* [n_runs] */,
                        int eval_range);
int fsclg_blocks_wait(fsclg_ctx *c, int batch, fsclg_point_t *pts /* sum(count) */,
                      double *bs /* sum(count * nb) * n_la */, uint32_t *cnt /* as bs */);
double fsclg_blocks_last_ms(fsclg_ctx *c, int batch);

/* The conditional sweep scan: the surface with every walk cut to the sites a candidate sweep owns.
   Runs, alpha lists, batch, slot, eval_range and window null sums are fsclg_surface_submit's; there is
   one more argument, clip[2 * sum(count)]: per position, runs in order, a pair (lo, hi) of global site
   indices (copied, like the runs; any int32, lo > hi: empty).  sm[p * n_la + k] is the position's
   null_logl plus the terms of the walk of la[k] whose site index lies in [lo, hi], in the reference's
   walk order (the nearest SNP if inside, then leftwards, then rightwards: sm-search.c:105-150), added
   strictly in that order; an alpha whose nearest SNP is past its own cut has an empty walk whatever the
   clip holds.  With [lo, hi] covering the window, points and values are fsclg_surface_wait's byte for
   byte; with an empty interval every value is null_logl.  The point is the row's first strict maximum
   as there; the device counters count the clipped walks' terms.  The same input gives the same bytes
   on every batch and slot and for every chunking.  FSCLG_E_ARG for a NULL clip with positions; the
   other error codes are fsclg_surface_submit's (FSCLG_E_STATE from the wait when the batch holds no
   conditional scan).  fsclg_cond_last_ms: the kernel's own time of the batch's last launch. */
int fsclg_cond_submit(fsclg_ctx *c, int batch, int slot, const fsclg_run_t *runs, int n_runs,
                      const double *la /* [n_runs][n_la] */, int n_la, const int32_t *clip /* 2 * sum(count) */,
                      int eval_range);
int fsclg_cond_wait(fsclg_ctx *c, int batch, fsclg_point_t *pts /* sum(count) */,
                    double *sm /* sum(count) * n_la, position-major */);
double fsclg_cond_last_ms(fsclg_ctx *c, int batch);

/* Per-site likelihood terms: the data axis of a sweep position.  A request is one walk of
   sm_likelihood (sm-search.c:105-150) -- a chromosome, a position and a log alpha, any double
   >= LOG_AD_MIN (-20), not only a value of the alpha grid -- on the rows a slot holds.  Its header's
   pt is what init_scan_result(chr, pos) gives on those rows (nearest_snp, the de-collided sweep_pos,
   the window, n_snps, null_logl; cost 0) with lalpha the request's, sm_logl the exact sequential sum
   null_logl + t_0 + t_1 + ... and clr = 2 * (sm_logl - null_logl).  terms[off + k], k < len, is what
   snp_likelihood (sm-search.c:85-103) returns for the walk's k-th site in walk order: the nearest
   SNP (k = 0), then leftwards (site nearest_snp - k, k <= nl), then rightwards (site nearest_snp +
   k - nl); folding them one by one from pt.null_logl in that order gives pt.sm_logl bit for bit.
   Only the doubles are stored: the site of term k follows from the header.  A walk whose nearest
   SNP is already outside log(alpha d) <= LOG_AD_MAX has len = nl = nr = 0 and sm_logl = null_logl;
   otherwise len = 1 + nl + nr.  The walks' terms lie one after another in request order (off is
   the running sum of len).
   fsclg_sites_submit / fsclg_sites_wait take batches, slots and window null sums exactly as
   fsclg_curve_submit / fsclg_curve_wait do (any batch and slot; the window sums of the slot's rows
   are summed here, one covering cell per request; several devices: submit to all, then wait).
   The submit launches the headers (one workgroup per request) and returns at once; the wait forms
   the offsets on the host and launches the terms into a pinned staging area of
   fsclg_sites_cap() terms ($FSCLG_SITES_CAP, default 4194304 = 32 MiB), as many launches as the
   walks need -- a walk longer than the area is cut across launches -- copying each launch's terms
   into terms[]; the result does not depend on the cut.  *n_terms (if not NULL) is set to the sum of
   len.  If terms_cap is below it (or terms is NULL), the wait returns FSCLG_E_ARG, writes neither
   hdr nor terms, and the batch STAYS submitted: a caller may wait with terms_cap = 0 to size its
   buffer and wait again.  A NULL hdr is FSCLG_E_ARG in the same way.  Any other return ends the
   batch.  Further errors: FSCLG_E_ARG for a bad chr, batch or
   slot, a position above INT_MAX - 64, a lalpha that is NaN or below LOG_AD_MIN;
   FSCLG_E_STATE for tables or SNPs not uploaded, a batch not waited for (submit), no sites
   submitted on the batch (wait).  fsclg_sites_last_ms: the summed time (HIP events) of the batch's
   last header launch and term launches; the device counters of fsclg_stats_t do not count these
   walks (kernel_ms, n_launches and busy_ms do). */
typedef struct {
  int32_t chr, pos;
  double lalpha;
} fsclg_site_req_t;
typedef struct {
  fsclg_point_t pt;
  int32_t nl, nr, len, pad;  /* terms left / right of the nearest SNP; len = 0 or 1 + nl + nr; pad 0 */
  uint64_t off;              /* index of the walk's first term in terms[] */
} fsclg_site_hdr_t;
int fsclg_sites_submit(fsclg_ctx *c, int batch, int slot, const fsclg_site_req_t *req, int n_req, int eval_range);
int fsclg_sites_wait(fsclg_ctx *c, int batch, fsclg_site_hdr_t *hdr, double *terms, size_t terms_cap, size_t *n_terms);
double fsclg_sites_last_ms(fsclg_ctx *c, int batch);
size_t fsclg_sites_cap(void);

/* Sweep-model sampler: one replicate of derived counts under the model the scan fits, at the
   positions and chromosome limits of fsclg_upload_snps.
   fsclg_sample_tables uploads the sampler's own tables (the scan's hold only the rows some site
   uses): coef_t, every unfolded row f = 1 .. n-1 of every depth, interval-major
   [depth][interval][f][c0..c3] (depth d starts after the 4 * n_iv * (depth_n[e] - 1) doubles of
   the depths e < d), and neutral, per depth the neutral probabilities fsp[1 .. n-1] one depth
   after another (sum of depth_n[d] - 1 doubles).  n_iv and log_ad_step must be those of
   fsclg_upload_tables, whose interval thresholds and log table the sampler shares (FSCLG_E_STATE
   before it, FSCLG_E_ARG when they differ; a depth_n below 2 or above 8192 is FSCLG_E_ARG).
   fsclg_sample_submit draws site i (the index of fsclg_upload_snps), of depth index
   depth_of_site[i] and sample size n:
     1. the nearest sweep among those of the site's chromosome: least |pos_i - sweep pos|, a tie to
        the lower sweep position, then to the first in sweeps[];
     2. log_ad = logt(|pos_i - sweep pos|) + lalpha with the search kernels' three-branch logt
        (logt(0) = 0);
     3. p_f = fsp[f] if the chromosome has no sweep or log_ad > LOG_AD_MAX, else exp(spline_f(log_ad))
        with the scan's interval (clamped to 0 below LOG_AD_MIN, log_ad itself not clamped); a p_f
        that is NaN, negative or infinite counts as 0;
     4. u = (mix64(mix64(seed ^ 0x9E3779B97F4A7C15) ^ ((uint64)(uint32)rep << 32 | (uint32)i)) >> 11)
        * 2^-53, mix64 splitmix64's output function: no state, a function of (seed, rep, i);
     5. with S = sum p_f and t = u * S the least f whose cumulative sum C_f > t and whose p_f > 0
        (the greatest f with p_f > 0 if rounding leaves none): an f of probability 0 is never drawn;
     6. S zero or not finite: the site is degenerate, freq_out[i] = -1.
   The cumulative sums are formed in a fixed order (a wave scan per 64 counts), with no atomics:
   the same build, seed and rep give the same bytes; the neutral sites read a per-depth prefix table
   summed sequentially on the host.  A site whose t lies within rounding of a C_f may differ from a
   sequential restatement.  Asynchronous like fsclg_sites_submit / fsclg_sites_wait on any batch
   (no slot: the positions are the uploaded ones); depth_of_site and sweeps are copied.
   fsclg_sample_wait stores the n_snps derived counts (1 .. n-1, or -1) and the number of degenerate
   sites.  Errors: FSCLG_E_ARG for a bad batch, a depth index outside the tables, n_sweeps < 0 or
   above 4096, a sweep chromosome out of range, a lalpha that is NaN; FSCLG_E_STATE for tables or
   SNPs not uploaded, a batch not waited for (submit), no sample submitted on it (wait).
   fsclg_sample_last_ms: the kernel's own time (HIP events) of the batch's last sample. */
typedef struct {
  int32_t chr, pos;
  double lalpha;
} fsclg_sweep_t;
int fsclg_sample_tables(fsclg_ctx *c, const double *coef_t, const double *neutral, const int32_t *depth_n, int n_depths,
                        int n_iv, double log_ad_step);
int fsclg_sample_submit(fsclg_ctx *c, int batch, const int32_t *depth_of_site, const fsclg_sweep_t *sweeps, int n_sweeps,
                        unsigned long long seed, int rep);
int fsclg_sample_wait(fsclg_ctx *c, int batch, int32_t *freq_out, unsigned long long *n_degenerate);
double fsclg_sample_last_ms(fsclg_ctx *c, int batch);

/* Projected tail of a null record: a noncentral chi-square fit per point.
   Point p holds the counts[p] floats samples[offsets[p] ..]; m = counts[p].  Its positive
   samples -- x > 0 and finite; zero, negative, NaN and infinite ones count in m alone -- are
   modelled as noncentral chi-square with df = 2 h degrees of freedom (df even, >= 2) and
   noncentrality lambda >= 0, the density being the Poisson mixture
     f(x) = sum_j e^-a a^j / j! * b^(h+j-1) e^-b / (2 (h+j-1)!),   a = lambda / 2, b = x / 2,
   summed outward from its largest term (j (j + h - 1) ~ a b), scaled by that term.
     m_pos < max(min_n, 1):   flag FSCLG_TAIL_NOFIT; lambda, logl, log10_q are NaN;
     mean of the positive samples <= df:  flag FSCLG_TAIL_CENTRAL, lambda = 0;
     otherwise FSCLG_TAIL_FIT: lambda is the root of the score 1/2 sum (f_{df+2} / f_df - 1), by
       60 bisection steps in a bracket [0, hi], hi = max(1, 2 (mean - df)) doubled until the score
       there is not positive.
   logl = sum log f(x_i; df, lambda) over the positive samples; mean and variance (n - 1 in the
   denominator; NaN below two positive samples) are theirs too.  log10_q = log10 Q(x0[p]), Q the
   upper tail of the fitted distribution at x0, for even df the Poisson double sum
     Q = e^(-a - b0) sum_j a^j / j! sum_{i < h + j} b0^i / i!,   b0 = x0 / 2,
   formed in the log domain throughout (finite where e^-b0 underflows); x0 <= 0 or NaN gives 0.
   Every sum has a fixed order (lanes stride over the samples, one wave per point): the same
   build and input give the same bytes.  Log-factorials are lgamma calls.  A density series that
   needs more than 4096 terms either way from its largest term (a b beyond about 1e10), or a
   tail sum of more than 2^20 terms, gives NaN in logl or log10_q.
   Asynchronous like fsclg_sample_submit / fsclg_sample_wait on any batch, and needs neither
   tables nor sites; the arrays are copied.  Errors: FSCLG_E_ARG for a bad batch, n_points < 0, an
   odd df or one below 2, a negative count, offsets + counts past n_samples; FSCLG_E_STATE for a
   batch not waited for (submit), no tail submitted on it (wait).
   fsclg_tail_last_ms: the kernel's own time (HIP events) of the batch's last tail call. */
enum { FSCLG_TAIL_FIT = 0, FSCLG_TAIL_CENTRAL = 1, FSCLG_TAIL_NOFIT = 2 };
typedef struct {
  int32_t m, m_pos;
  double mean, variance, lambda, logl, log10_q;
  int32_t flag, pad;
} fsclg_tail_t;
int fsclg_tail_submit(fsclg_ctx *c, int batch, const float *samples, size_t n_samples, const unsigned long long *offsets,
                      const int32_t *counts, const double *x0, int n_points, int df, int min_n);
int fsclg_tail_wait(fsclg_ctx *c, int batch, fsclg_tail_t *out);
double fsclg_tail_last_ms(fsclg_ctx *c, int batch);

/* Family-wise maxima of unpruned permutation trials (Westfall-Young maxT).
   clr[n_trials][m] holds every point's CLR in every trial of a chunk, obs[m] the observed CLRs,
   order[m] the points by observed CLR descending (ties by index ascending; any permutation of
   0 .. m-1 is accepted and defines the ranks), group[m] each point's group (its chromosome) in
   [0, n_groups).  A value enters a maximum as v + 0.0, so a maximum of zeros is +0.0; a NaN is never
   a maximum and never exceeds; a maximum over no value, or over NaN alone, is -inf.
   Per trial t:  gmax[t] the maximum over the points and garg[t] the least point index whose value
   equals it (-1 when there is none: no point, or NaN alone);  grp_max[t][g], grp_arg[t][g] the same
   over the points of group g.
   Per point i, over the chunk's trials, three counts:
     c_single[i] = #{t : gmax[t] >= obs[i]},
     c_chr[i]    = #{t : grp_max[t][group[i]] >= obs[i]},
     c_step[i]   = #{t : u_t(rank of i) >= obs[i]},  u_t(j) = max of clr[t][order[k]] over k >= j,
   the successive suffix maximum of the step-down procedure (a NaN obs[i] counts nothing).
   Everything is comparisons and integer adds: the result does not depend on the order of
   execution, and the counts of successive chunks add up to the counts of their union.
   One workgroup of FSCLG_MAXT_WG threads per trial; the suffix maxima run in tiles of
   FSCLG_MAXT_TILE ranks.  Asynchronous like fsclg_tail_submit / fsclg_tail_wait on any batch, and
   needs neither tables nor sites; the arrays are copied.  Errors: FSCLG_E_ARG for a bad batch,
   a negative size, n_groups above FSCLG_MAXT_MAX_GROUPS, a group outside [0, n_groups), an order
   that is no permutation, n_trials * (n_groups + 1) past an int, a NULL result (wait: the batch
   stays submitted); FSCLG_E_STATE for a batch not waited for (submit), no maxima submitted on it
   (wait).  fsclg_maxt_last_ms: the kernel's own time (HIP events) of the batch's last maxt call. */
#define FSCLG_MAXT_WG 256
#define FSCLG_MAXT_TILE 1024
#define FSCLG_MAXT_MAX_GROUPS 4096
int fsclg_maxt_submit(fsclg_ctx *c, int batch, const double *clr, int n_trials, int m, const double *obs,
                      const int32_t *order, const int32_t *group, int n_groups);
int fsclg_maxt_wait(fsclg_ctx *c, int batch, double *gmax, int32_t *garg, double *grp_max, int32_t *grp_arg,
                    int32_t *c_single, int32_t *c_chr, int32_t *c_step);
double fsclg_maxt_last_ms(fsclg_ctx *c, int batch);

/* Expected terms of a walk under the model: what the fitted spectrum itself predicts at a sweep.
   A request is a walk of fsclg_sites_submit (chr, pos; its lalpha field is not read); request r is evaluated at each of the
   n_la log alphas la[r * n_la ..], giving the tasks (r, k) in that order.  The sites of task (r, k)
   are exactly the sites whose terms fsclg_sites_submit returns for (chr, pos, la[r * n_la + k]) on
   the slot's rows -- the same nearest SNP, window limits and cut at log(alpha d) > LOG_AD_MAX -- in
   ascending site index [nearest - nl, nearest + nr]; an empty walk has no sites.
   fsclg_expect_tables uploads what the sampler's tables lack (fsclg_sample_tables first, whose
   unfolded coefficients are reused; FSCLG_E_STATE before it, FSCLG_E_ARG for other depths or another
   knot grid): fcoef, the folded rows [depth][interval][c][c0..c3], c = 1 .. n/2 (depth d starts after
   the 4 * n_iv * (depth_n[e] / 2) doubles of the depths e < d); neutral, fsp[1 .. n-1] per depth;
   null_unf, null_logl of an unfolded site of class f = 1 .. n-1 per depth; null_fold, null_logl of a
   folded site of class c = 1 .. n/2 per depth; row_class[n_rows of fsclg_upload_tables], per device
   row the depth index of the sites that carry it, bit 31 set for a folded row.  The device takes no log.
   For site i of depth n at x = logt(|d|) + lalpha (fsclg_sample_submit's logt and interval, with the
   clamp to interval 0), over the derived counts f = 1 .. n-1:
     p_f = exp(spline_f(x)), q_f = fsp[f]; a value that is not finite or not positive counts as 0;
     S = sum p_f, Q = sum q_f;
     the observed class of f is c = f, on a folded site c = min(f, n - f);
     t_f = spline_c(x) - null_unf[c], on a folded site fspline_c(x) - null_fold[c]: what
       snp_likelihood returns for the site observed in that class;
     f is usable iff p_f > 0, q_f > 0 and t_f is finite; Su, Qu are S, Q over the usable f;
     m1_s = sum (p_f / Su) t_f, m2_s = sum (p_f / Su) t_f^2; m1_0, m2_0 the same with q_f / Qu;
     lost_s = 1 - Su / S, lost_0 = 1 - Qu / Q.
   A site with no usable class, or with S, Q, Su or Qu not positive and finite, is degenerate: its
   moments and losses are stored as 0 and it adds nothing to the sums below but obs and the counts.
   Order of the class sums: lane l of the site's wave adds its classes f = 1 + l, 65 + l, 129 + l, ...
   in ascending f from +0.0 (the unnormalised sums sum p t, sum p t^2, ...), then the 64 lane sums are
   combined by an xor butterfly with lane distances 32, 16, 8, 4, 2, 1 in that order, and the
   quotients are taken last.  obs is the site's observed term, the value fsclg_sites_wait stores.
   tot[task * (n_bins + 1) + b], b < n_bins, covers the task's sites whose x falls into bin b of
   n_bins equal-width bins of [LOG_AD_MIN, LOG_AD_MAX]: b = (int)((x - LOG_AD_MIN) * n_bins / 24)
   clamped to [0, n_bins - 1] (x below the range goes to bin 0); entry b = n_bins covers all of the
   task's sites.  Each sum is a sequential fold over the sites in ascending site index from +0.0,
   var = max(m2 - m1^2, 0) per site; max_lost_* is the greatest loss of a site that is not degenerate
   (0 without one).  No atomic is on the result path: the same input gives the same bytes on every
   batch and slot, alone or among other requests.
   Asynchronous like fsclg_sites_submit / fsclg_sites_wait (any batch and slot; the window null sums
   are summed here).  The submit launches the walks' headers; fsclg_expect_count blocks for them and
   gives the number of (task, site) pairs; fsclg_expect_wait launches expect_kernel (phase 0: one wave
   per pair, the site's moments into device memory; phase 1: one workgroup per task folds them) and
   stores tot (n_req * n_la * (n_bins + 1) entries), hdr if not NULL (n_req * n_la headers as
   fsclg_sites_wait's, off the index of the task's first site record) and sites if not NULL (the
   site records, task after task; sites_cap below their number: FSCLG_E_ARG, the batch stays
   submitted).  Errors as fsclg_sites_submit's, and FSCLG_E_ARG for n_la outside [1, 64], n_bins
   outside [1, 64], a lalpha outside [LOG_AD_MIN, LOG_AD_MAX], more than 65535 tasks;
   FSCLG_E_STATE when the expect tables are not set for the uploaded tables.
   fsclg_expect_last_ms: the summed time (HIP events) of the batch's header launch and expect_kernel
   launches. */
typedef struct {
  int32_t site;              /* global site index */
  int16_t degenerate, bin;   /* 1: degenerate; the site's bin of x among the call's n_bins */
  double x, obs, m1_s, m2_s, m1_0, m2_0, lost_s, lost_0;
} fsclg_expect_site_t;
typedef struct {
  uint32_t n_sites, n_degenerate;
  double obs, e_s, v_s, e_0, v_0;  /* sums of obs, m1_s, var_s, m1_0, var_0 (log-likelihood scale) */
  double max_lost_s, max_lost_0;
} fsclg_expect_tot_t;
int fsclg_expect_tables(fsclg_ctx *c, const double *fcoef, const double *neutral, const double *null_unf,
                        const double *null_fold, const int32_t *depth_n, int n_depths, int n_iv, double log_ad_step,
                        const uint32_t *row_class, int n_rows);
int fsclg_expect_submit(fsclg_ctx *c, int batch, int slot, const fsclg_site_req_t *req, int n_req,
                        const double *la /* [n_req][n_la] */, int n_la, int n_bins, int eval_range);
int fsclg_expect_count(fsclg_ctx *c, int batch, size_t *n_sites);
int fsclg_expect_wait(fsclg_ctx *c, int batch, fsclg_expect_tot_t *tot, fsclg_site_hdr_t *hdr, fsclg_expect_site_t *sites,
                      size_t sites_cap);
double fsclg_expect_last_ms(fsclg_ctx *c, int batch);

/* the exact interval thresholds the kernel uses in place of spline_interpolate's
   division (sm-spline.c:52): thr[j] = least double x with
   (int)((x - LOG_AD_MIN) / log_ad_step) >= j, for j = 1..n_iv (thr has n_iv+1 slots) */
int fsclg_interval_thresholds(double log_ad_step, int n_iv, double *thr);

int fsclg_get_stats(fsclg_ctx *c, fsclg_stats_t *st);
int fsclg_reset_stats(fsclg_ctx *c);

#ifdef __cplusplus
}
#endif
#endif
