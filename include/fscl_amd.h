/*
 * fscl_amd.h -- drop-in C ABI for slowkoni/fscl's CLR scan + permutation path,
 * implemented on MI355X (gfx950).
 *
 * The data types are byte-compatible with the reference's fscl.h and the
 * entry points keep the reference's names, argument meaning and error
 * behaviour (fatal errors print and exit(1); OOM aborts).  A maintainer
 * replaces the reference objects scan-chromosome.o and sm-search.o (and, if
 * wanted, sm-spline.o background-fsp.o asc-bias.o snp-input.o logmsg.o) by
 * -lfscl_amd; fscl.c's main() links unchanged.  See INTEGRATION.md.
 *
 * Entry point -> reference interface it replaces (/root/reference):
 *   load_snp_input             fscl.h:87   snp-input.c:19-145
 *   background_fsp             fscl.h:91   background-fsp.c:182-316
 *   output_background_fs       fscl.h:93   background-fsp.c:318-336
 *   lchoose                    fscl.h:94   sm-spline.c:41-46
 *   compute_sweep_model_tables fscl.h:97   sm-spline.c:486-520
 *   spline_interpolate         fscl.h:101  sm-spline.c:48-60
 *   init_log_table             fscl.h:104  sm-search.c:14-26
 *   search_maxalpha            fscl.h:105  sm-search.c:269-300   (GPU)
 *   compute_snp_null_model     fscl.h:108  scan-chromosome.c:23-37
 *   scan_chromosome            fscl.h:109  scan-chromosome.c:228-329 (GPU)
 *   scan_permute               fscl.h:111  scan-chromosome.c:582-652 (GPU + host permutation)
 *   scan_output                fscl.h:115  scan-chromosome.c:666-750
 *   ms_openfile/ms_background/ms_next_block fscl.h:118-123 ms-input.c:11-151
 *   ascbias_adjust_background  fscl.h:126  asc-bias.c:27-95
 *   ascbias_adjust_expect      fscl.h:128  asc-bias.c:97-109
 *   configure_logmsg/logmsg/cr_logmsg fscl.h:134-136 logmsg.c:20-52
 */
#ifndef FSCL_AMD_H
#define FSCL_AMD_H

#include <stdint.h>

#include "fsclg.h"  /* fsclg_run_t, fsclg_point_t (fscl_amd_profile_runs) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- data model: same layout as fscl.h:7-76 -------------------------------- */
typedef struct {
  int chr;
  int pos;
  double null_logl;
  int obs_freq;
  int depth_p;
  int folded;
} snp_t;

typedef struct {
  int chr;
  char *name;
  int start_index;
  int n_snps;
  int start_pos;
  int bp_length;
} chr_limits_t;

typedef struct {
  int chr;
  int nearest_snp;
  int sweep_pos;
  int n_snps;
  int window_start;
  int window_end;
  double lalpha;
  double null_logl;
  double sm_logl;
  double clr;
  int permute_n;
  int permute_p;
  int permute_finished;
  int scan_running;
  float *permute_clr;
} scan_pt_t;

typedef struct {
  int n_snps;
  snp_t *snps;
  int n_depths;
  int *sample_depths;
  int n_scan_pts;
  scan_pt_t *scan_pts;
  chr_limits_t *chr_limits;
  int n_chromosomes;
} scan_t;

typedef struct {
  int n;
  double *knot_points;
  double **coef;
} spline_t;

typedef struct {
  spline_t **spline_func;
  spline_t **fspline_func;
  int sample_size;
  double **pbk;
  double *fsp;
} sm_ptable_t;

#define LOG_AD_MIN (-20.0)
#define LOG_AD_MAX (4.0)
#define N_SPLINE_KNOTS (200)

enum { MSG_FATAL = 0, MSG_ERROR, MSG_WARN, MSG_STATUS, MSG_DEBUG1, MSG_DEBUG2 };

/* Globals the reference's fscl.c defines (fscl.c:33-34).  The library holds
   weak defaults so it also works without fscl.c; fscl.c's definitions win. */
extern int spline_pts;
extern int n_permute;
extern char *output_fname;
extern char *prepend_label;

/* ---- reference entry points -------------------------------------------------- */
scan_t *load_snp_input(char *snp_fname, int include_invariant, int minimum_obs_depth);
double **background_fsp(scan_t *scan_obj, int force_neutral_spectrum, char *background_fsfname,
                        int include_invariant);
void output_background_fs(char *fname, scan_t *scan_obj, double **fsp);
double lchoose(int n, int k);
sm_ptable_t *compute_sweep_model_tables(scan_t *scan_obj, double **fsp, int asc_depth, int asc_min_freq,
                                        int ascbias_background_only, int include_invariant);
double spline_interpolate(spline_t *spf, double x);
void init_log_table(void);
void search_maxalpha(scan_pt_t *scan_pt, snp_t *snps, sm_ptable_t *sm_p);
void compute_snp_null_model(scan_t *scan_obj, double **fsp);
void scan_chromosome(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, int bp_resl, int large_grid_sp,
                     int n_threads);
void scan_permute(scan_t *scan_obj, sm_ptable_t *sm_p, int n_permute, double permute_nbp, double alpha_factor,
                  int n_threads, int eval_range, int bp_resl, int large_grid_sp, double scan_width_mb);
void scan_output(char *output_fname, scan_t *scan_obj, int maximum_only, int n_permute, char *prepend_label);
/* ms input block by block (fscl.h:118-123, ms-input.c; called at fscl.c:281-313),
   with fscl_amd_load_ms_input's semantics: ms_background = every block,
   ms_next_block = the next block as a one-chromosome scan_t, NULL at the end */
void ms_openfile(char *ms_fname);
scan_t *ms_background(char *ms_fname, int ms_segment_length, int ms_folded, int ms_sample_first,
                      int ms_sample_size);
scan_t *ms_next_block(int ms_segment_length, int ms_folded, int ms_sample_first, int ms_sample_size);
double *ascbias_adjust_background(double *bsf, int n, int asc_depth, int min_obs);
void ascbias_adjust_expect(double *fsp, int n, int min_obs, int d);
void configure_logmsg(int level);
void logmsg(int priority, volatile char *s, ...);
void cr_logmsg(int priority, volatile char *s, ...);

/* ---- MI355X extensions ------------------------------------------------------- */
/* ms input (defined semantics): every "//" block is one
   chromosome named by its 1-based block number, a site sits at
   (int)(x * segment_length), sites monomorphic in the chosen sample are
   dropped; returns the same scan_t as load_snp_input */
scan_t *fscl_amd_load_ms_input(const char *ms_fname, int segment_length, int ms_folded, int sample_first,
                               int sample_size);

/* the permutation rand() stream is process-wide and seeded once, as srand(0xFD821A6)
   in the reference's init_options (fscl.c:135): it continues across scan_permute calls.
   fscl_amd_srand restarts it (what a fresh process would see). */
void fscl_amd_srand(unsigned seed);

/* permutation mode of scan_permute.  FSCL_AMD_PERMUTE_PARITY (default): the reference's
   procedure on its rand() stream, results identical to the reference.
   FSCL_AMD_PERMUTE_THROUGHPUT (labelled non-parity): the same procedure with
   counter-based random numbers -- trial t's block permutation from the glibc stream seeded by a
   hash of (seed, t), point i's prune draw in trial t a hash of (seed, t, i) -- so trials run
   independently on every GPU and rank; results are a function of the seed alone (any number of
   GPUs), and match the oracle's --throughput-seed.  $FSCL_AMD_PERMUTE=throughput[:seed]
   overrides.  Returns 0, or -1 for an unknown mode. */
#define FSCL_AMD_PERMUTE_PARITY 0
#define FSCL_AMD_PERMUTE_THROUGHPUT 1
int fscl_amd_set_permute_mode(int mode, unsigned long long seed);

/* what a SIGINT during scan_permute writes (scan-chromosome.c:553-560): by default
   fscl.c's globals output_fname / prepend_label; a library caller sets them here */
void fscl_amd_set_dump_output(const char *fname, const char *label);

/* device selection.  Default: one device, $FSCL_AMD_DEVICE, else LOCAL_RANK, else 0.
   fscl_amd_set_devices(ids, n): this process drives n GPUs (ids NULL: 0 .. n-1; n = 0:
   every visible GPU) -- each batch of grid cells is split into cost-balanced contiguous
   shares, one per device, the host logic (permutation, pruning) runs once; results are
   identical to one device.  fscl_amd_n_devices: the devices opened (0 before the first scan). */
int fscl_amd_set_device(int device);
int fscl_amd_set_devices(const int *devices, int n);
int fscl_amd_n_devices(void);

/* Multi-process parity mode (one process per GPU).  Every rank runs the same
   host logic (rand() stream, block permutation, pruning) and evaluates a
   cost-balanced contiguous share of the grid cells / active points; the
   exchange callback must SUM-allreduce n int64 values across ranks (each slot
   is non-zero on exactly one rank, so the sum reproduces its 64-bit pattern
   exactly).  fn == NULL or world == 1: single process. */
typedef int (*fscl_amd_exchange_fn)(long long *buf, int n, void *ctx);
int fscl_amd_set_ranks(int rank, int world, fscl_amd_exchange_fn fn, void *ctx);

/* The same with the library's own exchange: the ranks share one node, and each batch's
   results are all-gathered through a POSIX shared-memory segment `name` (unique to the job,
   e.g. "/fscl_amd_<uuid>"; created by rank 0, unlinked once every rank has attached).
   Every rank calls it before its first scan; returns 0, or -1 if the ranks could not meet
   (within $FSCL_AMD_RANK_TIMEOUT seconds, default 600).  $FSCL_AMD_SHM_MB (default 64)
   bounds one exchange (64 B per grid cell of a batch). */
int fscl_amd_set_ranks_shm(int rank, int world, const char *name);

/* the cost-balanced contiguous split the ranks use: items [lo, hi) of n go to
   `rank` (costs: SNPs of the cell's chromosome, i.e. its window size) */
void fscl_amd_partition(const double *cost, int n, int rank, int world, int *lo, int *hi);

typedef struct {
  double scan_s;          /* wall seconds of scan_chromosome's evaluation */
  double permute_s;       /* wall seconds of scan_permute */
  double host_perm_s;     /* of which: host permutation generation */
  double kernel_ms;       /* summed GPU kernel time (HIP events) */
  unsigned long long gp_evals;   /* search_maxpos evaluations (grid points x trials) on this rank */
  unsigned long long n_terms, n_null, n_walks, n_maxalpha, n_unsafe, n_slow, n_ties, n_launches;
  unsigned long long negj; /* permutation blocks that hit the reference's negative-j bug (repaired) */
  int trials;             /* permutation trials run */
  int cache_iv0, cache_n_iv, cache_n_rows;  /* LDS coefficient window (fsclg_stats_t) */
  double cache_cover;
  double window_ms;       /* window null-sum kernels (chromosomes above 2*eval_range+1 SNPs) */
  double host_null_s;     /* scan_permute host phases: per-chromosome null sums */
  double host_upload_s;   /*   rows + null sums to the device */
  double search_s;        /*   cell evaluation (launch, kernel, results, rank exchange) */
  double prune_s;         /*   pruning and bookkeeping */
  unsigned long long n_dup_cells, n_ep_saved;  /* fsclg_stats_t: work shared between cells */
  double busy_ms;         /* fsclg_stats_t: union of the search kernels' intervals (overlap counted once) */
  double wait_s;          /* scan_permute: host time blocked on trial results */
  unsigned long long n_crit;  /* scan_permute: cells in the trials' blocking (near-critical) batches */
  unsigned long long n_drain; /* scan_permute: trials that had to wait for every bulk batch in flight */
  int n_devices;          /* local GPUs this process drives */
  int spec_threads;       /* scan_permute: permutation worker threads (0: no speculation) */
  unsigned long long spec_posted; /* trials whose next permutation was generated ahead, per draw count */
  unsigned long long spec_hits;   /*   of which the draw count was among the candidates */
  unsigned long long spec_cands;  /*   candidates generated */
  double spec_wait_s;     /* host time waiting for the chosen candidate to finish */
  unsigned long long spec_done; /* candidates completed (not cancelled) */
  double spec_gen_s;      /* worker seconds spent on the completed candidates */
  unsigned long long n_split_retry; /* fsclg_stats_t: split launches re-run unsplit */
  unsigned long long spec_claimed;  /* chosen candidates not started yet, built by the main thread instead */
  unsigned long long n_merged;      /* scan_permute: bulk cells evaluated in their trial's blocking batch */
  int perm_leader;        /* scan_permute: 1 if the node leader's shared permutation pool ran (one process
                             per GPU), 0 if this rank built its own permutations (single process, or the
                             pool's fallback when the shared segment could not be made) */
  int plan_mode;          /* scan_permute: 1 if the trials' permutations went to the devices as plans
                             (fsclg_slot_set_rows_plan), 0 as rows */
  unsigned long long plan_fallback; /* plan mode: trials whose plan did not fit its buffer (rows instead) */
  unsigned long long spec_rank[8];  /* speculation hits by the candidate's rank in the likeliest-first order
                                       (7: rank 7 or later): how many launched-ahead candidates would cover */
  unsigned long long prestaged;     /* plan mode, one process: trials whose likeliest candidate was applied to a
                                       spare device slot (with its window sums) while the trial before ran */
  unsigned long long prestage_hits; /*   of which it was the trial's permutation (its upload skipped) */
} fscl_amd_stats_t;
void fscl_amd_get_stats(fscl_amd_stats_t *st);
void fscl_amd_reset_stats(void);

/* ---- fine-grid CLR profile (-g) ------------------------------------------------
   The reference's disabled fine-grid loops (scan-chromosome.c:269-327): CLR and alpha at every
   small_grid_sp-spaced position, and the strict maximum over the fine positions of each coarse
   cell.  Each chromosome's grid covers the extent scan_chromosome's cells cover: from the first
   cell's start in steps of small_grid_sp to the last cell's (clipped) end, inclusive; an end the
   step does not land on is appended once.  small_grid_sp must divide large_grid_sp.
   grid_pos[i] is the requested position, pts[i] the point init_scan_result + search_maxalpha
   give there (sweep_pos after de-collision), cell[i] the index in scan_chromosome's cell order
   (= scan_obj->scan_pts order) of the cell whose [start, end] holds grid_pos[i]; a shared
   boundary belongs to the lower cell.  The profile is always of the data as loaded (also after
   scan_permute), on the device context scan_chromosome uses; with several local devices the
   kernel's chunks are dealt in contiguous cost-balanced shares (identical results); with
   several ranks, rank 0 alone evaluates (the others get NULL). */
typedef struct {
  int n_pts;
  scan_pt_t *pts;
  int *grid_pos;
  int *cell;
} fscl_amd_profile_t;
fscl_amd_profile_t *fscl_amd_scan_profile(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, int small_grid_sp,
                                          int large_grid_sp);
/* per coarse cell, the first grid point of strictly greatest clr among those with
   start <= grid_pos <= end (ascending), into out_max[n_scan_pts] (may be NULL); *n_missed: the
   cells whose grid maximum's clr exceeds scan_obj->scan_pts[cell].clr (the bisection's answer).
   Returns the number of cells, or -1 if scan_chromosome has not run.  scan_obj is not altered. */
int fscl_amd_profile_cell_max(const fscl_amd_profile_t *pf, const scan_t *scan_obj, scan_pt_t *out_max,
                              int *n_missed);
/* one line per grid point in scan_output's no-permutation row format (fname NULL: stdout) */
void fscl_amd_profile_output(const char *fname, const scan_t *scan_obj, const fscl_amd_profile_t *pf,
                             const char *prepend_label);
void fscl_amd_profile_free(fscl_amd_profile_t *pf);
/* the grid alone (no GPU): chromosome, position and cell of every grid point, malloc'd arrays
   (any may be NULL); returns the point count, -1 for a spacing that is not positive or does
   not divide large_grid_sp */
int fscl_amd_profile_grid(const scan_t *scan_obj, int small_grid_sp, int large_grid_sp, int **chr, int **grid_pos,
                          int **cell);
/* the evaluation alone, for any runs of positions (fsclg_profile over this process's devices):
   out holds sum(count) points; returns a fsclg status code.  fscl_amd_profile_last_ms: the
   profile kernel's milliseconds of the last evaluation (the slowest device's). */
int fscl_amd_profile_runs(scan_t *scan_obj, sm_ptable_t *sm_p, const fsclg_run_t *runs, int n_runs, int eval_range,
                          fsclg_point_t *out);
double fscl_amd_profile_last_ms(void);

/* ---- grid-maximum scan and permutation test (--scan-mode=grid) --------------------
   The statistic of the reference's disabled fine-grid loops (scan-chromosome.c:269-296 the
   scan, :505-523 the trial): a cell's point is the first grid position of strictly greatest
   clr among start + j * small_grid_sp, start <= pos <= end (fscl_amd_profile_grid's positions
   of the cell: the start shared with the lower cell included, a clipped end the step misses
   appended), found on the device by fsclg_cellmax_submit.

   fscl_amd_scan_chromosome_grid is scan_chromosome's counterpart: the same cells, one point per
   cell in cell order (which is (chromosome, position) order; not re-sorted), counters zeroed, a
   permute_clr buffer each; bit for bit fscl_amd_profile_cell_max(fscl_amd_scan_profile(...)).
   Fatal if small_grid_sp does not divide large_grid_sp.

   fscl_amd_scan_permute_grid is scan_permute's: the reference's trial loop
   (scan-chromosome.c:441-502 -- the rand() stream with its leading usleep draw, the block
   permutation, >= counting, the permute_p >= 20 prune draw, permute_clr saved as float, SIGINT)
   with a cell's search_maxpos replaced by its grid maximum on the permuted rows.  The trial's
   cell is the point's OWN cell, by cell index -- the positions the original statistic was
   maximised over -- not the G-aligned unclipped cell of the bisection path.  Several local
   devices share a trial's active cells (contiguous shares balanced by window size x positions);
   the results are those of one device.  Limits: one process, the parity stream only, trials in
   lockstep (no pipelining).  Fatal, with a message: several ranks, throughput permute mode,
   points that are not fscl_amd_scan_chromosome_grid's last result with the same spacings.
   The original rows are restored at the end. */
void fscl_amd_scan_chromosome_grid(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, int small_grid_sp,
                                   int large_grid_sp);
void fscl_amd_scan_permute_grid(scan_t *scan_obj, sm_ptable_t *sm_p, int n_permute, double permute_nbp,
                                int eval_range, int small_grid_sp, int large_grid_sp, double scan_width_mb);
/* fsclg_cellmax_submit / fsclg_cellmax_wait on the first device, for any runs (the device
   entry's test handle): out holds n_runs points.  rows NULL: on the uploaded rows (slot 0);
   else on `rows`, n_snps device rows (a rearrangement of fscl_amd_site_rows), set into slot 1
   with their whole-chromosome null sums.  Returns a fsclg status code.
   fscl_amd_cellmax_last_ms: the cell-maximum kernel's milliseconds of the last evaluation (the
   slowest device's); fscl_amd_site_rows: the device row of every site as uploaded, returns
   n_snps. */
int fscl_amd_cellmax_runs(scan_t *scan_obj, sm_ptable_t *sm_p, const fsclg_run_t *runs, int n_runs, int eval_range,
                          const uint32_t *rows, fsclg_point_t *out);
double fscl_amd_cellmax_last_ms(void);
int fscl_amd_site_rows(scan_t *scan_obj, sm_ptable_t *sm_p, uint32_t *out);

/* ---- alpha likelihood curves (--alpha-file) ---------------------------------------
   The alpha axis of the likelihood surface at a position: every composite likelihood
   search_maxalpha (sm-search.c:269-300) evaluates there, in its evaluation order -- la[k] the
   log alpha, sm[k] what sm_likelihood returns for it, k < n_coarse + n_refine (11 coarse values,
   then the refine list around the coarse winner); pt is the point init_scan_result +
   search_maxalpha give at the position (fscl_amd_profile_runs' point, bit for bit), and the first
   strict maximum of sm[] in order is (pt.sm_logl, pt.lalpha).  A record is fsclg_curve_t.

   fscl_amd_scan_curves: the curves at n (chromosome index, position) pairs, on the data as loaded
   (also after scan_permute), on the device context scan_chromosome uses; several local devices
   take contiguous shares balanced by window size (identical results); with several ranks, rank 0
   alone evaluates (the others return FSCLG_OK and leave out untouched).  Returns a fsclg status
   code.  fscl_amd_scan_point_curves: the curve of every scan point at its own sweep_pos, after
   scan_chromosome or fscl_amd_scan_chromosome_grid; out holds n_scan_pts records.

   fscl_amd_curve_support (host only): the evaluated alphas sorted, an alpha evaluated twice kept
   once; the connected run around the argmax whose sm >= sm_max - drop: *la_lo / *la_hi its least
   and greatest log alpha, *open_lo / *open_hi set when the run reaches the lowest / highest
   evaluated alpha (the interval may extend past the search range).  A NaN value breaks the run.
   Returns 1, 0 if no value beat the initial -DBL_MAX (all NaN: *la_lo = *la_hi = NaN), -1 for a
   NULL curve or a drop that is negative or NaN.  With drop = 2 the interval is the usual
   2-log-likelihood-unit support interval; the likelihood is a COMPOSITE one (sites are not
   independent), so it describes the curve's shape and is not a calibrated confidence interval.

   fscl_amd_curve_output (fname NULL: stdout): per curve, one row per distinct alpha, ascending:
     [label TAB] chromosome TAB position TAB alpha (%1.3e) TAB 2 * (sm - null_logl) (%1.2f) TAB mark
   mark is * on the argmax row and - elsewhere; then one summary row
     [label TAB] chromosome TAB position TAB support TAB alpha_lo TAB alpha_hi TAB open_lo TAB open_hi
   (alpha_lo, alpha_hi %1.3e, or NA NA 0 0 when there is no interval). */
typedef fsclg_curve_t fscl_amd_curve_t;
int fscl_amd_scan_curves(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, const int *chr, const int *pos, int n,
                         fscl_amd_curve_t *out);
int fscl_amd_scan_point_curves(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, fscl_amd_curve_t *out);
int fscl_amd_curve_support(const fscl_amd_curve_t *curve, double drop, double *la_lo, double *la_hi, int *open_lo,
                           int *open_hi);
void fscl_amd_curve_output(const char *fname, const scan_t *scan_obj, const fscl_amd_curve_t *curves, int n,
                           double drop, const char *prepend_label);
/* fsclg_curve_submit / fsclg_curve_wait on the first device, for any runs (the device entry's
   test handle): out holds sum(count) records; rows as for fscl_amd_cellmax_runs.
   fscl_amd_curve_last_ms: the curve kernel's milliseconds of the last evaluation (the slowest
   device's); fscl_amd_curve_forced: fsclg_curve_forced summed over the devices. */
int fscl_amd_curve_runs(scan_t *scan_obj, sm_ptable_t *sm_p, const fsclg_run_t *runs, int n_runs, int eval_range,
                        const uint32_t *rows, fscl_amd_curve_t *out);
double fscl_amd_curve_last_ms(void);
unsigned long long fscl_amd_curve_forced(void);

/* ---- position-by-alpha likelihood surfaces (--surface-file) --------------------------
   The surface whose position axis the profile gives (alpha maximised away) and whose alpha axis
   the curve gives (at one position): the composite likelihood at every position of a small grid
   around a centre, for every log alpha of one list, with no alpha search (fsclg_surface_submit).

   A request is (chromosome index, centre position, half-width bp, step bp, alpha list): its
   positions are centre + k * step for |k| <= halfwidth / step, those outside the chromosome's span
   [chr_limits.start_pos, chr_limits.bp_length] -- the span the profile's grid covers -- left out
   (fscl_amd_surface_run gives them as one run; -1 for a bad chromosome, step < 1 or halfwidth < 0).
   la[0 .. n_la) is strictly ascending, 1 <= n_la <= 64, each value in [LOG_AD_MIN, LOG_AD_MAX] =
   [-20, 4].  fscl_amd_surface_alphas builds such a list: the grid lo + i (hi - lo) / (n - 1), i < n
   (n = 1: lo = hi alone), its last value hi itself, with `fitted` inserted in order -- at either
   end when it lies outside [lo, hi]; not added when it equals a grid value, is NaN or lies outside
   [-20, 4]; returns the length (n or n + 1), or -1 for n outside [1, 63], endpoints outside
   [-20, 4], lo > hi, lo == hi with n > 1, or a grid whose neighbours are equal in double.

   A result owns its arrays (fscl_amd_surfaces_free; a zeroed one is empty).  Surface i has
   hdr[i]: its request, the run evaluated (start_pos, step, n_pos), the scan point it was centred
   on (point, -1: none), and where its n_pos points and n_pos * n_la values (position-major) start
   in pts[] and sm[].  pts and sm are fsclg_surface_wait's: sm[cell_off + p * n_la + k] is what
   sm_likelihood returns for la[k] at the p-th position, bit for bit; pts[pos_off + p] is the
   position's point with the row's first strict maximum.  n_terms: the walks' terms.

   fscl_amd_scan_surface: the surfaces of n requests, on the data as loaded (also after
   scan_permute), on the device context scan_chromosome uses; several local devices take
   contiguous shares of the requests balanced by window size x cells (identical results); with
   several ranks, rank 0 alone evaluates (the others return FSCLG_OK and an empty result).  Returns
   a fsclg status code (FSCLG_E_ARG: a NULL argument, n < 0, a request fscl_amd_surface_run or the
   device refuses).  fscl_amd_scan_point_surfaces: the `top` scan points of greatest CLR
   (fscl_amd_top_points with spacing = halfwidth and no predicate), in that order, each centred on
   its sweep_pos with fscl_amd_surface_alphas(la_lo, la_hi, n_grid, its fitted lalpha).

   fscl_amd_top_points (host only): the one peak selection of the --*-top options.  The indices of
   at most `top` scan points into idx_out[top], by descending CLR (ties in scan order, a NaN
   never); a point within `spacing` bp of one already chosen on its chromosome is skipped; a point
   `accept` (NULL: none) rejects is skipped too and does not block its neighbours.  Returns their
   number; -1 for a NULL scan, or a NULL idx_out with top > 0.

   fscl_amd_surface_region (host only), on sm[n_pos][n_la] and the positions' null sums: V = sm -
   null_logl per cell; M its maximum, the first in position order, then alpha order (max_ipos,
   max_ila, max_v = M); the joint region is the 4-connected component of the cells with V >= M -
   drop that holds the argmax (n_region cells; mark, if not NULL, gets 2 at the argmax, 1 inside the
   region, 0 elsewhere); the position interval [ipos_lo, ipos_hi] is the connected run, around the
   argmax position, of positions whose row maximum is >= M - drop, the alpha interval the same over
   columns; an open_* flag is 1 where its interval reaches the edge of the evaluated grid.  A NaN
   cell is never in a region.  Returns 1; 0 when every cell is NaN (indices -1, max_v NaN, flags
   0); -1 for a NULL array, an empty grid or a drop that is negative or NaN.  With drop = 2 the
   intervals match --alpha-file's; a joint two-parameter 95 % region under the chi-square reading
   would be about 3.0.  The likelihood is a COMPOSITE one (sites are not independent), so the
   region describes the surface's shape and is not a calibrated confidence region.

   fscl_amd_surface_output (fname NULL: stdout; 0, or -1 if the file cannot be opened or a header
   does not fit the arrays), per surface one row per cell, position-major:
     [label TAB] chromosome TAB centre_pos TAB pos TAB alpha (%1.3e) TAB 2 * (sm - null_logl) (%1.2f) TAB mark
   (pos: the point's sweep_pos; mark * at the argmax, + inside the joint region, - elsewhere), then
     [label TAB] chromosome TAB centre_pos TAB summary TAB n_pos TAB n_alpha TAB max_pos TAB max_alpha
       TAB max_clr TAB pos_lo TAB pos_hi TAB open_pos_lo TAB open_pos_hi TAB alpha_lo TAB alpha_hi
       TAB open_alpha_lo TAB open_alpha_hi TAB n_region
   with NA for the seven values and 0 for the flags and n_region when every cell is NaN. */
#define FSCL_AMD_SURFACE_MAX_LA 64
typedef struct {
  int32_t chr, centre_pos, halfwidth, step;
  int32_t n_la, point;  /* point: the scan point the request is centred on, -1: none */
  double la[FSCL_AMD_SURFACE_MAX_LA];
} fscl_amd_surface_req_t;
typedef struct {
  int32_t chr, centre_pos, halfwidth, step, n_la, point;
  int32_t start_pos, n_pos;  /* the run evaluated: start_pos + p * step, p < n_pos */
  uint64_t pos_off, cell_off;
  double la[FSCL_AMD_SURFACE_MAX_LA];
} fscl_amd_surface_hdr_t;
typedef struct {
  int n;  /* surfaces */
  fscl_amd_surface_hdr_t *hdr;
  fsclg_point_t *pts;
  double *sm;
  size_t n_pos, n_cells;
  unsigned long long n_terms;
} fscl_amd_surfaces_t;
typedef struct {
  int32_t n_pos, n_la, max_ipos, max_ila, ipos_lo, ipos_hi, ila_lo, ila_hi;
  int32_t open_pos_lo, open_pos_hi, open_la_lo, open_la_hi, n_region, pad;
  double max_v;
} fscl_amd_surface_region_t;
int fscl_amd_surface_alphas(double lo, double hi, int n, double fitted, double *out /* [64] */);
int fscl_amd_surface_run(const scan_t *scan_obj, const fscl_amd_surface_req_t *req, fsclg_run_t *run);
int fscl_amd_top_points(const scan_t *scan_obj, int top, int spacing, int (*accept)(const scan_pt_t *), int *idx_out);
int fscl_amd_scan_surface(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, const fscl_amd_surface_req_t *req, int n,
                          fscl_amd_surfaces_t *out);
int fscl_amd_scan_point_surfaces(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, int top, int halfwidth, int step,
                                 double la_lo, double la_hi, int n_grid, fscl_amd_surfaces_t *out);
void fscl_amd_surfaces_free(fscl_amd_surfaces_t *r);
int fscl_amd_surface_region(const double *sm, const double *null_logl, int n_pos, int n_la, double drop,
                            fscl_amd_surface_region_t *out, unsigned char *mark);
int fscl_amd_surface_output(const char *fname, const scan_t *scan_obj, const fscl_amd_surfaces_t *r, double drop,
                            const char *prepend_label);
/* fsclg_surface_submit / fsclg_surface_wait on the first device, for any runs (the device entry's
   test handle): la holds n_runs lists of n_la values, pts sum(count) points, sm sum(count) * n_la
   values; rows as for fscl_amd_cellmax_runs, batch any batch of the device (rows NULL: slot 0, else
   slot 1).  fscl_amd_surface_last_ms: the surface kernel's milliseconds of the last evaluation
   (the slowest device's, summed over its launches). */
int fscl_amd_surface_runs(scan_t *scan_obj, sm_ptable_t *sm_p, const fsclg_run_t *runs, int n_runs, const double *la,
                          int n_la, int eval_range, const uint32_t *rows, int batch, fsclg_point_t *pts, double *sm);
double fscl_amd_surface_last_ms(void);

/* ---- delete-one-block jackknife of sweep peaks (--jackknife-file) ---------------------
   An interval on a peak that respects linkage: the peak's footprint is cut into contiguous genomic
   blocks of block_bp, one block at a time is left out, the composite likelihood is re-maximised over
   the surface's position and alpha grid, and the spread of the re-estimates is read.  The device
   gives the surface's terms summed per block (fsclg_blocks_submit); the rest is host arithmetic.

   fscl_amd_scan_blocks: the block sums of n surface requests (fscl_amd_surface_req_t, positions by
   fscl_amd_surface_run) on the data as loaded, run as fscl_amd_scan_surface runs (slot 0; several
   local devices take contiguous shares balanced by window size x cells, all submitted to before the
   first wait; with several ranks, rank 0 alone evaluates).  A request's first block id b0 and block
   count nb come from the least window_start and the greatest window_end of its positions, taken
   from a surface evaluation of the same request, so the device's clamp never bites: block j holds
   the sites with b0 + j == pos / block_bp.  Before any device call it refuses (FSCLG_E_ARG, with a
   message naming the option to change) a request that needs more than 1024 blocks or a result
   above $FSCL_AMD_BLOCKS_CAP bytes (default 2^30; fscl_amd_blocks_cap), both judged with
   fscl_amd_blocks_bound: host only, the blocks of the widest windows the run's positions can have
   (the exact ones or one site more on either side); -1 for a bad argument.
   Result (owns its arrays; fscl_amd_blocks_free): hdr[i] the request, its run, block_bp, b0, nb and
   where its n_pos points and n_pos * nb * n_la cells (position-major, then block, then alpha) start;
   pts, bs, cnt are fsclg_blocks_wait's.

   fscl_amd_scan_point_jackknife: the `top` scan points of greatest CLR, chosen as
   fscl_amd_scan_point_surfaces chooses them, each centred on its sweep_pos with
   fscl_amd_surface_alphas(la_lo, la_hi, n_grid, its fitted lalpha).

   fscl_amd_jackknife_combine (host only) on bs / cnt [n_pos][nb][n_la], the positions' sweep_pos
   and the alphas: for every block b, V_b[p][k] = the sum of bs[p][j][k] over j != b in ascending j
   from +0.0; the block's estimate is the first strict maximum of V_b in position order, then alpha
   order (ipos, ila, v = V_b there; a NaN never wins; ipos = ila = -1 and v NaN when every cell is
   NaN), computed for the blocks that hold at least one term of some cell (has_terms; g of them).
   The full estimate (out->ipos, ila, v) is the same over every block.  blocks[b].n_terms is cnt at
   the full estimate's cell.  Over the g blocks, for theta in {sweep_pos, log alpha, CLR = 2 v}, with
   mean the plain mean of theta_b in block order: se^2 = (g - 1) / g * sum (theta_b - mean)^2, bias =
   (g - 1) (mean - theta_full); NaN (printed NA) when g < 2 or some delete-one surface is NaN alone.
   top_shift: the first block of greatest |pos_b - pos|; top_loss: the first of greatest CLR loss;
   n_edge_pos / n_edge_la: the delete-one maxima on the edge of the position / alpha grid (the
   open_* warning: the grid may be too small).  Returns 1; 0 when every cell of the full surface is
   NaN; -1 for a NULL or an empty array.

   The estimator is an argmax on a grid: an SE of 0 means "no block moves it by one step", and the
   jackknife of a non-smooth estimator is a guide, not a theorem.  The background spectrum and the
   tables are not re-estimated; the blocks are equal in bp and unweighted.

   fscl_amd_jackknife_output (fname NULL: stdout; 0, or -1 if the file cannot be opened or a header
   does not fit the arrays), per peak one row per block with terms:
     [label TAB] chromosome TAB centre_pos TAB block_start TAB block_end TAB n_terms TAB loo_pos TAB
       loo_alpha (%1.3e) TAB loo_clr (%1.2f) TAB d_pos TAB d_logalpha (%1.4f) TAB d_clr (%1.2f)
   (block_start = (b0 + j) * block_bp, block_end = block_start + block_bp - 1; the first and the last
   block also hold what lies beyond them), then
     [label TAB] chromosome TAB centre_pos TAB summary TAB n_pos TAB n_alpha TAB n_blocks (g) TAB pos TAB
       alpha TAB clr TAB se_pos (%1.1f) TAB se_logalpha (%1.4f) TAB se_clr (%1.2f) TAB bias_pos TAB
       bias_logalpha TAB top_shift_block TAB top_loss_block (their block_start) TAB n_edge_pos TAB n_edge_alpha
   with NA where a value does not exist. */
#define FSCL_AMD_BLOCKS_MAX_NB 1024
typedef struct {
  int32_t chr, centre_pos, halfwidth, step, n_la, point;
  int32_t start_pos, n_pos;  /* the run evaluated: start_pos + p * step, p < n_pos */
  int32_t block_bp, b0, nb, pad;
  uint64_t pos_off, cell_off;
  double la[FSCL_AMD_SURFACE_MAX_LA];
} fscl_amd_blocks_hdr_t;
typedef struct {
  int n;  /* peaks */
  fscl_amd_blocks_hdr_t *hdr;
  fsclg_point_t *pts;
  double *bs;
  uint32_t *cnt;
  size_t n_pos, n_cells;
  unsigned long long n_terms;
} fscl_amd_blocks_t;
typedef struct {
  int32_t block, has_terms, ipos, ila;
  uint32_t n_terms;
  int32_t pad;
  double v;
} fscl_amd_jack_block_t;
typedef struct {
  int32_t n_pos, n_la, nb, g, ipos, ila, top_shift, top_loss, n_edge_pos, n_edge_la;
  double v, se_pos, se_la, se_clr, bias_pos, bias_la, bias_clr;
} fscl_amd_jack_summary_t;
int fscl_amd_scan_blocks(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, const fscl_amd_surface_req_t *req, int n,
                         int block_bp, fscl_amd_blocks_t *out);
int fscl_amd_scan_point_jackknife(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, int top, int halfwidth, int step,
                                  double la_lo, double la_hi, int n_grid, int block_bp, fscl_amd_blocks_t *out);
void fscl_amd_blocks_free(fscl_amd_blocks_t *r);
size_t fscl_amd_blocks_cap(void);
int fscl_amd_blocks_bound(const scan_t *scan_obj, const fsclg_run_t *run, int eval_range, int block_bp, int *b0, int *nb);
int fscl_amd_jackknife_combine(const double *bs, const uint32_t *cnt, int n_pos, int nb, int n_la, const int32_t *pos,
                               const double *la, fscl_amd_jack_block_t *blocks /* [nb] */, fscl_amd_jack_summary_t *out);
int fscl_amd_jackknife_output(const char *fname, const scan_t *scan_obj, const fscl_amd_blocks_t *r, const char *prepend_label);
/* fsclg_blocks_submit / fsclg_blocks_wait on the first device, for any runs (the device entry's test
   handle): la holds n_runs lists of n_la values, blk one (block_bp, b0, nb) per run; pts sum(count)
   points, bs and cnt sum(count * nb) * n_la cells; rows and batch as fscl_amd_surface_runs.
   fscl_amd_blocks_last_ms: the block kernel's milliseconds of the last evaluation (the slowest
   device's). */
int fscl_amd_blocks_runs(scan_t *scan_obj, sm_ptable_t *sm_p, const fsclg_run_t *runs, int n_runs, const double *la,
                         int n_la, const fsclg_blocks_t *blk, int eval_range, const uint32_t *rows, int batch,
                         fsclg_point_t *pts, double *bs, uint32_t *cnt);
double fscl_amd_blocks_last_ms(void);

/* ---- per-site likelihood terms (--sites-file) --------------------------------------
   The data axis of a sweep position: which sites made this CLR.  A walk is one sm_likelihood
   (sm-search.c:105-150) at (chromosome index, position, log alpha); its header and terms are
   fsclg_site_hdr_t and the doubles of include/fsclg.h: terms[hdr.off + k] is snp_likelihood's value
   at the walk's k-th site in walk order (the nearest SNP, then leftwards, then rightwards), and
   folding them from hdr.pt.null_logl gives hdr.pt.sm_logl bit for bit.  A result owns its arrays
   (fscl_amd_sites_free; a zeroed one is empty); point[i] is the scan point of walk i, or NULL.

   fscl_amd_scan_sites: the walks of n requests, on the data as loaded (also after scan_permute),
   on the device context scan_chromosome uses; several local devices take contiguous shares
   balanced by window size (identical results); with several ranks, rank 0 alone evaluates (the
   others return FSCLG_OK and an empty result).  Returns a fsclg status code.
   fscl_amd_scan_point_sites: the walks of the scan points at their own sweep_pos and lalpha, after
   scan_chromosome or fscl_amd_scan_chromosome_grid: the top_k points of greatest CLR (ties keep
   scan order, a NaN CLR ranks last; top_k = 0: every point), listed in scan order.

   fscl_amd_sites_summary (host only), per walk into out[n]: n_sites = len; first_pos / last_pos
   the positions of the footprint's first and last site (-1 for an empty walk); n_pos / n_neg the
   terms above / below 0; top_term the greatest term and top_pos its site's position, the first in
   walk order on a tie, never a NaN (-1 and NaN when there is none); top_share = 2 * top_term / clr,
   NaN ("NA") when clr <= 0 or is NaN; n_half: with the positive terms in descending order (ties in
   walk order) and added one by one in double, the least count whose sum reaches half of the sum
   of all of them (0: no positive term).

   fscl_amd_sites_output (fname NULL: stdout), per walk in the result's order: one row per site in
   ascending site position
     [label TAB] chromosome TAB sweep_pos TAB site_pos TAB site_pos - sweep_pos TAB obs_freq TAB depth
       TAB folded TAB log(alpha d) (%1.4f) TAB term (%1.4f)
   then one summary row
     [label TAB] chromosome TAB sweep_pos TAB summary TAB n_sites TAB first_pos TAB last_pos TAB n_pos
       TAB n_neg TAB top_pos TAB top_term (%1.4f) TAB top_share (%1.4f) TAB n_half
   with NA for a position, term or share that does not exist. */
typedef fsclg_site_hdr_t fscl_amd_site_hdr_t;
typedef struct {
  int n;            /* walks */
  int *point;       /* [n] scan point index of each walk (fscl_amd_scan_point_sites), or NULL */
  fscl_amd_site_hdr_t *hdr;
  double *terms;
  size_t n_terms;
} fscl_amd_sites_t;
typedef struct {
  int32_t n_sites, first_pos, last_pos, n_pos, n_neg, top_pos, n_half, pad;
  double top_term, top_share;
} fscl_amd_sites_summary_t;
int fscl_amd_scan_sites(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, const fsclg_site_req_t *req, int n,
                        fscl_amd_sites_t *out);
int fscl_amd_scan_point_sites(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, int top_k, fscl_amd_sites_t *out);
void fscl_amd_sites_free(fscl_amd_sites_t *r);
void fscl_amd_sites_summary(const scan_t *scan_obj, const fscl_amd_sites_t *r, fscl_amd_sites_summary_t *out);
void fscl_amd_sites_output(const char *fname, const scan_t *scan_obj, const fscl_amd_sites_t *r,
                           const char *prepend_label);
/* the summed kernel milliseconds of the last evaluation (the slowest device's) */
double fscl_amd_sites_last_ms(void);

/* ---- sweep-model simulation and parametric bootstrap (--simulate-file, --bootstrap-file) ----
   Data under the model the scan fits, at the loaded data's own positions, depths, folded flags
   and chromosome limits (the reference's sm-sample.c draws uniform positions at one depth): per
   site one derived count from the model spectrum of its nearest sweep, by the site semantics of
   fsclg_sample_submit (include/fsclg.h) -- the scan's three-branch log distance, the tables as
   built (ascertainment correction included), a strict choice rule that never draws a count of
   probability 0, and a counter-based uniform that is a function of (seed, rep, site) alone.

   A sweep is (chromosome index, position, alpha > 0).  fscl_amd_parse_sweep reads "name:pos:alpha"
   (the name as in the input; the last two colons separate): 0, or -1 malformed, -2 unknown
   chromosome, -3 alpha not positive or not finite.  fscl_amd_nearest_sweep: the index of the sweep
   that governs a site at (chr, pos) -- least |pos - sweep pos|, a tie to the lower sweep position,
   then to the first given -- or -1 when the chromosome has none (the rule the kernel applies).

   fscl_amd_simulate: replicate `rep` of `seed` into freq_out[scan_obj->n_snps], the drawn derived
   counts 1 .. n-1; a degenerate site (model spectrum summing to 0 or not finite) keeps its observed
   count and is counted in *n_degenerate (may be NULL).  n_sweeps = 0 is a neutral replicate.  The
   sampler's tables (every unfolded row of every depth, interval-major) are built on first use and
   kept while the tables' hash stays; the sites go up as for a scan unless the device already holds
   these positions and chromosome limits.  Runs on the first device; with several ranks, rank 0
   alone evaluates (the others return FSCLG_OK and leave freq_out alone).  Neither scan_obj nor the
   permutation stream is touched.  FSCLG_E_ARG: alpha <= 0 or not finite, a chromosome out of
   range, n_sweeps < 0; otherwise a fsclg status code.
   fscl_amd_simulate_scan: a new scan_t with the same positions, depths, folded flags, chromosome
   limits and names, sharing nothing with the original, without scan points; obs_freq = freq[i], or
   min(freq[i], n - freq[i]) at a folded site; null_logl 0 (the caller runs compute_snp_null_model
   and scan_chromosome on it, as for loaded data).  fscl_amd_scan_free releases it.
   fscl_amd_simulate_output: the SNP input format, one line per site "chr pos derived_count
   sample_size folded", which load_snp_input reads back to the same sites; 0, or -1 if the file
   cannot be written.

   fscl_amd_bootstrap: for rep = 0 .. reps-1 -- simulate with every sweep planted, build the
   replicate scan, recompute its null model from fsp, scan_chromosome it (bisection), and per
   planted sweep record the replicate's scan point of greatest CLR with |sweep_pos - planted pos|
   <= window_bp on that chromosome (the first on a tie; est_pos -1 and NaN values when there is
   none) -- into out[sweep * reps + rep].  scan_obj, its scan points and its permutation counters
   stay as they are; the next call on scan_obj uploads it again, as a fresh scan does.  One process
   only (FSCLG_E_STATE with several ranks); FSCLG_E_ARG as fscl_amd_simulate, or reps < 0.
   fscl_amd_bootstrap_times: wall seconds of the last bootstrap -- total, simulation, null model and
   replicate building, upload of the replicates, scanning.
   fscl_amd_bootstrap_output (fname NULL: stdout; host only), per sweep one row per replicate
     [label TAB] chromosome TAB planted_pos TAB planted_alpha (%1.3e) TAB rep TAB est_pos TAB
       est_alpha (%1.3e) TAB CLR (%1.2f)          (NA NA NA when the replicate found no point)
   then one summary row
     [label TAB] chromosome TAB planted_pos TAB summary TAB reps TAB n_found TAB pos_q025 TAB pos_q50
       TAB pos_q975 TAB alpha_q025 TAB alpha_q50 TAB alpha_q975 TAB clr_q50
   where quantile q of the n_found found values is sorted[floor(q * (n_found - 1))], each column
   sorted on its own, and NA when n_found = 0. */
typedef struct {
  int chr;
  int pos;
  double alpha;
} fscl_amd_sweep_t;
typedef struct {
  int32_t sweep, rep, chr, planted_pos;
  double planted_alpha;
  int32_t est_pos, pad;       /* -1: no scan point within the window */
  double est_lalpha, clr;     /* NaN then */
} fscl_amd_boot_t;
int fscl_amd_parse_sweep(const scan_t *scan_obj, const char *text, fscl_amd_sweep_t *out);
int fscl_amd_nearest_sweep(const fscl_amd_sweep_t *sweeps, int n_sweeps, int chr, int pos);
int fscl_amd_simulate(scan_t *scan_obj, sm_ptable_t *sm_p, const fscl_amd_sweep_t *sweeps, int n_sweeps,
                      unsigned long long seed, int rep, int *freq_out, unsigned long long *n_degenerate);
scan_t *fscl_amd_simulate_scan(const scan_t *scan_obj, const int *freq);
void fscl_amd_scan_free(scan_t *scan_obj);
int fscl_amd_simulate_output(const char *fname, const scan_t *scan_obj);
double fscl_amd_simulate_last_ms(void);
int fscl_amd_bootstrap(scan_t *scan_obj, sm_ptable_t *sm_p, double **fsp, const fscl_amd_sweep_t *sweeps, int n_sweeps,
                       int reps, unsigned long long seed, int window_bp, int eval_range, int bp_resl, int large_grid_sp,
                       fscl_amd_boot_t *out);
void fscl_amd_bootstrap_times(double out[5]);
void fscl_amd_bootstrap_output(const char *fname, const scan_t *scan_obj, const fscl_amd_sweep_t *sweeps, int n_sweeps,
                               int reps, const fscl_amd_boot_t *out, const char *prepend_label);
/* the sampler's tables of n_depths depths, for fsclg_sample_tables: every unfolded row f = 1 .. n-1
   interval-major ([depth][interval][f][c0..c3]) and the neutral probabilities fsp[1 .. n-1]; both
   malloc'd, *n_iv the splines' interval count (host only) */
void fscl_amd_sample_tables_build(const sm_ptable_t *sm_p, int n_depths, double **coef_t, double **neutral,
                                  int32_t *depth_n, int *n_iv);

/* ---- expected CLR and term moments of a sweep under the model (--expect-file) ----------
   What the fitted model itself predicts at a sweep (chr, pos, alpha): for every site of the walk
   fscl_amd_scan_sites returns for it, the first two moments of the site's term over the model
   spectrum -- under the sweep (p_f = exp(spline_f(x))) and under neutrality (q_f = the tables'
   fsp[f]) -- with the class f = 1 .. n-1 observed as c = f, or min(f, n - f) on a folded site, and its
   term t_f = spline_c(x) - null_logl(depth, c), what snp_likelihood returns for the site observed in
   that class.  The definitions -- usable classes, renormalisation, lost mass, degenerate sites, the
   bins of x = logt(|d|) + log alpha over [-20, 4], the fixed order of every sum -- are fsclg_expect_submit's
   (include/fsclg.h).  null_logl comes from tables built with compute_snp_null_model's expressions from
   fsp, the background spectra the null model was computed from (fscl_amd_expect_tables_build, host
   only; all four malloc'd: the folded rows [depth][interval][c][c0..c3], the tables' neutral
   probabilities, the null values of the unfolded classes f = 1 .. n-1 and of the folded classes c = 1 ..
   n/2).
   fscl_amd_scan_expect: request i is evaluated at its own list -- la[0 .. n_la), ascending, with
   req[i].lalpha inserted in order unless it is one of them -- as the tasks first[i] .. first[i + 1),
   own[i] the index of its own alpha within them; hdr[task] is the walk's header (as fscl_amd_scan_sites';
   off counts the sites of the tasks before), tot[task * (n_bins + 1) + b] its totals of bin b, entry
   n_bins of all its sites.  The totals are sums of log-likelihood terms; the file doubles them (the
   CLR scale).  Runs on the first device on the data as loaded; with several ranks rank 0 alone
   evaluates (the others return FSCLG_OK with hdr NULL).  Refused with FSCLG_E_ARG before any device
   work, fscl_amd_expect_error() naming the option (fscl_amd_expect_check, host only: 0 or -1): n_bins
   outside 1 .. 64, n_la outside 1 .. 64 or a list not ascending within [-20, 4], an unknown chromosome, a
   log alpha outside [-20, 4], a result above $FSCL_AMD_EXPECT_CAP bytes (default 2^30).
   fscl_amd_scan_point_expect: the `top` scan points of greatest CLR at their fitted alpha, skipping
   a point within `spacing` bp of one already chosen (--surface-top's rule); point[i] is the scan point
   of request i.
   fscl_amd_expect_output (fname NULL: stdout; host only; 0, or -1 if the file cannot be written), per
   request, all likelihood columns on the CLR scale (2 x the sum, SD = 2 sqrt(sum var)):
     [label TAB] chromosome pos alpha bin x_lo x_hi n_sites obs E_sweep SD_sweep z_sweep E_null SD_null z_null
     [label TAB] chromosome pos alpha curve alpha_k n_sites E_sweep SD_sweep E_null SD_null dprime
     [label TAB] chromosome pos alpha summary n_sites n_degenerate obs E_sweep SD_sweep z_sweep E_null SD_null
       z_null max_lost_sweep max_lost_null
   tab separated; the bins of the request's own alpha that hold sites, then one curve row per alpha of
   its list, then the summary.  z = (obs - E) / SD, dprime = (E_sweep - E_null) / sqrt((SD_sweep^2 +
   SD_null^2) / 2), NA where the divisor is 0.  The SDs assume independent sites.
   fscl_amd_expect_runs: the test handle of fsclg_expect_submit / _count / _wait on the first device
   and slot 0, for any batch; *sites_out (may be NULL) is malloc'd. */
#define FSCL_AMD_EXPECT_MAX_LA 64
#define FSCL_AMD_EXPECT_MAX_BINS 64
typedef struct {
  int n, n_tasks, n_bins;
  fsclg_site_req_t *req;     /* [n] */
  int *first;                /* [n + 1] */
  int *own;                  /* [n] */
  double *la;                /* [n_tasks] */
  fsclg_site_hdr_t *hdr;     /* [n_tasks]; NULL: not evaluated on this rank */
  fsclg_expect_tot_t *tot;   /* [n_tasks][n_bins + 1] */
  int *point;                /* [n] scan point of each request (fscl_amd_scan_point_expect), else NULL */
  double kernel_ms;
} fscl_amd_expect_t;
int fscl_amd_scan_expect(scan_t *scan_obj, sm_ptable_t *sm_p, double **fsp, int eval_range, const fsclg_site_req_t *req, int n,
                         const double *la, int n_la, int n_bins, fscl_amd_expect_t *out);
int fscl_amd_scan_point_expect(scan_t *scan_obj, sm_ptable_t *sm_p, double **fsp, int eval_range, int top, int spacing,
                               const double *la, int n_la, int n_bins, fscl_amd_expect_t *out);
int fscl_amd_expect_runs(scan_t *scan_obj, sm_ptable_t *sm_p, double **fsp, const fsclg_site_req_t *req, int n_req,
                         const double *la, int n_la, int n_bins, int eval_range, int batch, fsclg_expect_tot_t *tot,
                         fsclg_site_hdr_t *hdr, fsclg_expect_site_t **sites_out, size_t *n_sites);
int fscl_amd_expect_check(const scan_t *scan_obj, const fsclg_site_req_t *req, int n, const double *la, int n_la, int n_bins);
const char *fscl_amd_expect_error(void);
size_t fscl_amd_expect_cap(void);
int fscl_amd_expect_bin(double x, int n_bins);
void fscl_amd_expect_tables_build(const sm_ptable_t *sm_p, double **fsp, int n_depths, double **fcoef, double **neutral,
                                  double **null_unf, double **null_fold, int32_t *depth_n, int *n_iv);
int fscl_amd_expect_output(const char *fname, const scan_t *scan_obj, const fscl_amd_expect_t *r, const char *prepend_label);
void fscl_amd_expect_free(fscl_amd_expect_t *r);
double fscl_amd_expect_last_ms(void);

/* ---- conditional sweep scan given fixed sweeps (--conditional-file) ------------------
   The composite likelihood of one more sweep at a candidate position, given sweeps held fixed, as
   a likelihood ratio against the model with the given sweeps alone -- the fit of what
   fscl_amd_simulate draws with several sweeps: every site belongs to its nearest sweep.

   Ownership.  The candidate's position s is the position's sweep_pos after init_scan_result's
   de-collision (the reference's rule, its comparison of a global index with the chromosome's count
   included).  A site at x belongs to the sweep of least |x - position|, a tie to the lower
   position, then to the first listed, the given sweeps listed before the candidate
   (fscl_amd_nearest_sweep's rule).  Against a given sweep q > s the candidate owns the sites with
   2x <= s + q, against q < s those with 2x > s + q (64-bit sums), with q = s nothing: its sites
   are one interval [lo, hi] of global site indices, cut by the nearest given sweep on either side
   and by the chromosome's ends; lo > hi when it is empty.  fscl_amd_cond_clip (host only) gives
   *sweep_pos, *lo and *hi from the chromosome's given sweeps (entries of another chromosome are
   skipped); -1 for a NULL argument or a bad chromosome.

   Values.  V(s, a): the position's window null sum N plus, in the reference's walk order, the terms
   of the walk at log alpha a whose sites lie in [lo, hi] (fsclg_cond_submit).  G_i: the term of
   site i in the walk of the given sweep that owns it among the given sweeps, at that sweep's
   log alpha -- the term fscl_amd_scan_sites returns for (chr, q, log alpha_q) -- and +0.0 where i is
   not in that walk (fscl_amd_cond_given_terms, host only, from the sites result of the chromosome's
   given sweeps in their order, into g[the chromosome's n_snps]).  A(s): the strictly sequential sum
   of G_i over [lo, hi] cut to [window_start, window_end], ascending from +0.0
   (fscl_amd_cond_base, host only; *n_terms: the sites of that interval).  The position's point is
   the first strict maximum of V in list order, and cond_clr = 2.0 * ((V - N) - A) at it.
   The given sweeps' positions and alphas are held fixed, ownership goes by distance alone, and the
   likelihood is composite: the ratio describes, it is not a calibrated test.

   fscl_amd_scan_conditional: per round (1 .. 8) and per chromosome that holds a given sweep, the
   positions chr start_pos + k * step over [start_pos, bp_length]; with halfwidth > 0 only those
   within halfwidth of a given sweep of the chromosome.  After a round each chromosome's position of
   greatest cond_clr (the first in position order on a tie; NaN never) joins the given sweeps with
   its alpha if it is strictly above min_clr, and the next round runs against the enlarged set; the
   rounds end early when no chromosome adds one.  alphas: an ascending list of n_la log alphas,
   1 .. 64 values in [-20, 4].  Runs on slot 0 as fscl_amd_scan_surface does (contiguous shares of
   the local devices, all submitted to before the first wait; rank 0 alone evaluates with several
   ranks).  Refused with FSCLG_E_ARG before any device work, fscl_amd_conditional_error() naming the
   option: an unknown chromosome, alpha not positive or log alpha outside [-20, 4], more than 64
   given sweeps on a chromosome (FSCL_AMD_COND_MAX_GIVEN), step < 1, rounds outside [1, 8], a bad
   alpha list, or a result above fscl_amd_conditional_cap() bytes ($FSCL_AMD_COND_CAP, default 2^30).
   A returned point whose sweep_pos is not the one its clip was computed from is fatal.

   fscl_amd_conditional_output (fname NULL: stdout; host only): per block one row per position
     [label TAB] chromosome TAB round TAB pos TAB alpha (%1.3e) TAB cond_CLR (%1.2f) TAB own_first_pos
       TAB own_last_pos TAB n_terms TAB base (%1.4f)
   then one summary row
     [label TAB] chromosome TAB round TAB summary TAB n_pos TAB n_given TAB given (pos:alpha,...) TAB
       max_pos TAB max_alpha TAB max_cond_clr TAB added
   own_*: the positions of the first and last owned site, NA for an empty interval; max_*: NA when
   no position has a cond_clr that is not NaN.  0, or -1 (a NULL argument, a block outside the
   arrays, a file that cannot be written). */
#define FSCL_AMD_COND_MAX_GIVEN 64
#define FSCL_AMD_COND_MAX_ROUNDS 8
typedef struct {
  int32_t pos;              /* the candidate's sweep_pos */
  int32_t lo, hi;           /* its sites, global indices; lo > hi: none */
  int32_t n_terms;          /* sites of [lo, hi] inside the position's window */
  double lalpha, cond_clr, base;
  double v, null_logl;      /* V at lalpha and N */
} fscl_amd_cond_row_t;
typedef struct {
  int32_t chr, round;       /* round 1 .. */
  int32_t n_pos, n_given;
  uint64_t row_off, given_off; /* the block's rows in rows[], its given sweeps in given[] */
  int32_t max_row, added;   /* the row of greatest cond_clr within the block (-1: none); whether it joined */
} fscl_amd_cond_block_t;
typedef struct {
  int n_blocks;
  fscl_amd_cond_block_t *blk;
  fscl_amd_cond_row_t *rows;
  fscl_amd_sweep_t *given;     /* every block's given sweeps, alpha > 0 */
  size_t n_rows, n_given;
  unsigned long long n_terms; /* the device's walk terms */
  double fold_s;              /* host seconds of the base folds */
} fscl_amd_conditional_t;
int fscl_amd_cond_clip(const scan_t *scan_obj, const fscl_amd_sweep_t *given, int n_given, int chr, int pos,
                       int *sweep_pos, int *lo, int *hi);
int fscl_amd_cond_given_terms(const scan_t *scan_obj, const fscl_amd_sweep_t *given, int n_given, int chr,
                              const fscl_amd_site_hdr_t *hdr, const double *terms, double *g);
double fscl_amd_cond_base(const double *g, int chr_start_index, int lo, int hi, int window_start, int window_end,
                          int *n_terms);
size_t fscl_amd_conditional_cap(void);
const char *fscl_amd_conditional_error(void);
/* every refusal of fscl_amd_scan_conditional, host only: 0, or -1 with fscl_amd_conditional_error() set */
int fscl_amd_conditional_check(const scan_t *scan_obj, const fscl_amd_sweep_t *given, int n_given, int halfwidth, int step,
                               const double *alphas, int n_la, int rounds, double min_clr);
int fscl_amd_scan_conditional(scan_t *scan_obj, sm_ptable_t *sm_p, int eval_range, const fscl_amd_sweep_t *given,
                              int n_given, int halfwidth, int step, const double *alphas, int n_la, int rounds,
                              double min_clr, fscl_amd_conditional_t *out);
int fscl_amd_conditional_output(const char *fname, const scan_t *scan_obj, const fscl_amd_conditional_t *r,
                                const char *prepend_label);
void fscl_amd_conditional_free(fscl_amd_conditional_t *r);
/* the kernel milliseconds of the last fscl_amd_scan_conditional / fscl_amd_cond_runs (the slowest device's, summed
   over the rounds) */
double fscl_amd_conditional_last_ms(void);
/* the test handle of fsclg_cond_submit / fsclg_cond_wait on the first device: fscl_amd_surface_runs with the
   positions' clips */
int fscl_amd_cond_runs(scan_t *scan_obj, sm_ptable_t *sm_p, const fsclg_run_t *runs, int n_runs, const double *la,
                       int n_la, const int32_t *clip, int eval_range, const uint32_t *rows, int batch,
                       fsclg_point_t *pts, double *sm);

/* ---- projected p-values from a noncentral chi-square fit (--tail-file) ----
   The permutation test's empirical p-value cannot go below 1 / permute_n.  Per scan point, the
   saved null CLRs x_1 .. x_m (m = min(permute_n, FSCL_AMD_TAIL_SAVE), the used prefix of
   permute_clr, in its own order; the record is not touched) are fitted by the model of
   fsclg_tail_submit (include/fsclg.h): the positive ones as noncentral chi-square with df degrees
   of freedom (even, >= 2) and a noncentrality lambda >= 0 found by maximum likelihood, the others
   as a point mass at "no sweep found".  The projected p-value at the observed CLR is
     p_tail = (m_pos / m) * Q(CLR; df, lambda),
   Q the fitted upper tail, carried as log10 so that it stays finite far below 1e-308; CLR <= 0
   gives Q = 1.  Points with fewer than min_n positive samples are not fitted (FSCLG_TAIL_NOFIT).
   The projection assumes one noncentral chi-square per point, a df fixed by the caller, and it
   treats twice a composite log-likelihood ratio as if it were a likelihood ratio; var_ratio --
   the positive samples' variance over the model's 2 (df + 2 lambda) -- and the calibration figure
   are the guards.

   fscl_amd_tail_fit: every scan point of scan_obj after scan_permute or
   fscl_amd_scan_permute_grid, into out->pt[n_scan_pts] (malloc'd; fscl_amd_tail_free), with the
   summary filled in.  Runs on the first device, in launches of at most $FSCL_AMD_TAIL_CAP floats
   (default 2^24).  One process only (FSCLG_E_STATE with several ranks); FSCLG_E_ARG for an odd df
   or one below 2; otherwise a fsclg status code.  Neither scan_obj nor the permutation stream is
   touched.
   fscl_amd_tail_runs: the same fit of raw records -- point p holds counts[p] floats at
   samples[offsets[p]], observed value x0[p] -- into out[n_points]; needs no scan.
   fscl_amd_tail_last_ms: the summed kernel milliseconds of the last of either.
   Host only: fscl_amd_tail_count (the used prefix of a point's record), fscl_amd_tail_chunk (how
   many points from `first` go into one launch of at most cap floats; at least one),
   fscl_amd_tail_pack (those points' samples into buf, their offsets into offsets[n]; returns the
   floats written), fscl_amd_tail_log10p (log10 p_tail of a row, NaN when not fitted),
   fscl_amd_tail_summary (n_fit, n_central, n_nofit and the calibration: over the fitted points
   with permute_p >= 5 the median of log10 p_tail - log10 p_empirical, p_empirical the -o column's
   ratio; NaN without such a point) and fscl_amd_tail_output (fname NULL: stdout; 0, or -1 if the
   file cannot be written), one row per scan point in -o order:
     [label TAB] chromosome TAB position TAB CLR (%1.2f) TAB permute_p TAB permute_n TAB m_pos TAB
       lambda (%1.4f) TAB var_ratio (%1.3f) TAB -log10 p_empirical (%1.3f) TAB -log10 p_tail (%1.3f)
       TAB flag (fit, central, nofit)
   with NA for lambda, var_ratio and -log10 p_tail of a nofit point, and for a var_ratio that is
   not finite. */
#define FSCL_AMD_TAIL_SAVE 10000 /* CLR_NULL_DIST_SAVE: the null CLRs a point keeps */
typedef struct {
  int n;              /* scan points */
  int df, min_n;
  fsclg_tail_t *pt;   /* [n] */
  int n_fit, n_central, n_nofit;
  int n_calibration;  /* points behind the calibration figure */
  double calibration;
  double kernel_ms, wall_s;
} fscl_amd_tail_t;
int fscl_amd_tail_fit(scan_t *scan_obj, int df, int min_n, fscl_amd_tail_t *out);
int fscl_amd_tail_runs(const float *samples, size_t n_samples, const unsigned long long *offsets, const int32_t *counts,
                       const double *x0, int n_points, int df, int min_n, fsclg_tail_t *out);
double fscl_amd_tail_last_ms(void);
void fscl_amd_tail_free(fscl_amd_tail_t *t);
int fscl_amd_tail_count(const scan_pt_t *scan_pt);
int fscl_amd_tail_chunk(const int32_t *counts, int n_points, int first, size_t cap);
size_t fscl_amd_tail_pack(const float *const *src, const int32_t *counts, int first, int n, float *buf,
                          unsigned long long *offsets);
double fscl_amd_tail_log10p(const fsclg_tail_t *row);
void fscl_amd_tail_summary(const scan_t *scan_obj, fscl_amd_tail_t *t);
int fscl_amd_tail_output(const char *fname, const scan_t *scan_obj, const fscl_amd_tail_t *t, const char *prepend_label);

/* ---- family-wise adjusted p-values from unpruned permutation maxima (--familywise-file) ----
   Westfall-Young maxT over the scan points.  Trial t = 0 .. trials-1 applies the block permutation
   the throughput mode gives its trial t under `seed`, evaluates EVERY scan point on
   its trial cell (the G-aligned, unclipped cell, Q5) -- no pruning, no prune draw -- and T[t][i] is
   point i's CLR there.  The trials are pipelined over the row slots and the local devices (one
   trial per device at a time); T is reduced on the first device in chunks of B trials by
   fsclg_maxt_submit (include/fsclg.h), B the most trials whose B * n doubles fit in
   $FSCL_AMD_FWER_CAP bytes (default 2^28), and the chunks' counts are added.  No result depends on
   B, on the number of devices or on the depth of the pipeline.  With obs_i the point's CLR, the
   points ranked by obs descending (ties by index ascending), M = trials:
     p_single_i = (1 + c_single_i) / (M + 1),   c_single_i = #{t : max_k T[t][k] >= obs_i};
     p_chr_i    = (1 + c_chr_i) / (M + 1),      the same over the points of i's chromosome;
     p_step     the step-down value: in rank order p_step_(1) = (1 + c_step_(1)) / (M + 1) and
                p_step_(j) = max(p_step_(j-1), (1 + c_step_(j)) / (M + 1)), c_step_(j) the trials
                whose maximum over the ranks >= j reaches obs_(j).
   At level a, k = floor(a (M + 1)) and the threshold is the k-th largest of the M maxima (none when
   k = 0); a point is significant exactly when its CLR is strictly above it, which is p_single <= a.
   maxT controls the family-wise error rate only as far as the block permutation is a valid null
   (the per-point test's own assumption); the reference has no such test; the cost is M full scans.

   fscl_amd_familywise: the pass, after a bisection scan (scan_chromosome), in one process
   (FSCLG_E_STATE with several ranks); FSCLG_E_ARG for trials < 1, a cap below one trial or more
   chromosomes than FSCLG_MAXT_MAX_GROUPS (fscl_amd_familywise_error names the reason).  The
   arrays of *out are malloc'd (fscl_amd_familywise_free); matrix is T itself when keep_matrix, else
   NULL.  The scan points, the permutation test's records and the rand() stream are not touched; the
   original rows are back on the devices at the end.
   fscl_amd_familywise_runs: fsclg_maxt_submit / wait of a caller's matrix clr[n_trials][m] on the
   first device, in the same chunks, counts added; needs no scan.
   fscl_amd_familywise_last_ms: the summed maxt_kernel milliseconds of the last of either.
   Host only (familywise.c): fscl_amd_familywise_order (the rank order of obs[n]; a NaN ranks last),
   fscl_amd_familywise_chunk (B for n points under cap bytes, at most trials; 0 when one trial does
   not fit), fscl_amd_familywise_combine (rank[n] from 1, and the three p-values, from the counts),
   fscl_amd_familywise_threshold (k, and *thr the k-th largest of maxima[M], NaN when k = 0),
   fscl_amd_familywise_output (fname NULL: stdout; 0, or -1 if the file cannot be written) -- one
   row per scan point in -o order, then one summary row per chromosome and one for the genome:
     [label TAB] chromosome TAB position TAB CLR (%1.2f) TAB alpha (%1.3e) TAB rank TAB p_chr (%1.3e)
       TAB p_single (%1.3e) TAB p_step (%1.3e) TAB -log10 p_step (%1.3f)
     [label TAB] chromosome | "genome" TAB "summary" TAB M TAB n_points TAB max_q50 (%1.2f) TAB thr_10
       TAB thr_05 TAB thr_01 (%1.2f) TAB n_sig_05 TAB n_sig_01
   max_q50 the median of the row's M maxima, thr_* its thresholds at levels 0.10, 0.05 and 0.01,
   n_sig_* counted by p_step on the genome row and by p_chr on a chromosome row; NA for a threshold
   with k = 0 and for a figure that is not finite --
   and fscl_amd_familywise_null_output, one row per trial:
     [label TAB] trial TAB genome_max (%1.4f) TAB argmax_chromosome TAB argmax_position
       then every chromosome's maximum (%1.4f); NA where there is none. */
typedef struct {
  int n, n_groups, trials;      /* scan points, chromosomes, M */
  unsigned long long seed;
  int32_t *order;               /* [n] the points by observed CLR descending */
  int32_t *c_single, *c_chr, *c_step; /* [n] */
  double *gmax;                 /* [trials] */
  int32_t *garg;
  double *chr_max;              /* [trials][n_groups] */
  int32_t *chr_arg;
  double *matrix;               /* [trials][n], or NULL */
  double kernel_ms, wall_s;
} fscl_amd_familywise_t;
int fscl_amd_familywise(scan_t *scan_obj, sm_ptable_t *sm_p, int trials, unsigned long long seed, double permute_nbp,
                        int eval_range, int bp_resl, int large_grid_sp, double scan_width_mb, int keep_matrix,
                        fscl_amd_familywise_t *out);
int fscl_amd_familywise_runs(const double *clr, int n_trials, int m, const double *obs, const int32_t *order,
                             const int32_t *group, int n_groups, double *gmax, int32_t *garg, double *grp_max,
                             int32_t *grp_arg, int32_t *c_single, int32_t *c_chr, int32_t *c_step);
double fscl_amd_familywise_last_ms(void);
const char *fscl_amd_familywise_error(void);
size_t fscl_amd_familywise_cap(void); /* $FSCL_AMD_FWER_CAP, or 2^28 */
/* the pass's host-only refusals before any device work: trials, the chromosomes, and one trial of
   the scan's cells (one point each at this spacing) under the cap; 0, or -1 with the reason */
int fscl_amd_familywise_check(const scan_t *scan_obj, int large_grid_sp, int trials);
void fscl_amd_familywise_free(fscl_amd_familywise_t *f);
void fscl_amd_familywise_order(const double *obs, int n, int32_t *order);
int fscl_amd_familywise_chunk(int n, int trials, size_t cap_bytes);
void fscl_amd_familywise_combine(const int32_t *c_single, const int32_t *c_chr, const int32_t *c_step, const int32_t *order,
                                 int n, int trials, int32_t *rank, double *p_single, double *p_chr, double *p_step);
int fscl_amd_familywise_threshold(const double *maxima, int trials, double level, double *thr);
int fscl_amd_familywise_output(const char *fname, const scan_t *scan_obj, const fscl_amd_familywise_t *f,
                               const char *prepend_label);
int fscl_amd_familywise_null_output(const char *fname, const scan_t *scan_obj, const fscl_amd_familywise_t *f,
                                    const char *prepend_label);

/* release the device context (tables / snps) */
void fscl_amd_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif
