/* scan_internal.h -- what crosses the seams between scan.c (the scan core), trials.c (everything
   that permutes rows) and analyses.c (the analysis drivers); included by those three alone.  Every
   name here is hidden: libfscl_amd.so is linked under the reference's own fscl.c,
   where a global `D` or `fh_prepare` would interpose. */
#ifndef SCAN_INTERNAL_H
#define SCAN_INTERNAL_H

#include <stdio.h>

#include "fscl_host.h"

#define FH_HIDDEN __attribute__((visibility("hidden")))

#define CLR_NULL_DIST_SAVE 10000 /* scan-chromosome.c:227 */

/* ---------------------------------------------------------- device state
   One host process drives n_dev local GPUs (fscl_amd_set_devices; the fscl CLI's
   --n-gpus), and optionally takes part in a job of `world` such processes (one per GPU,
   fscl_amd_set_ranks / fscl_amd_set_ranks_shm).  The host logic -- cells, rand stream,
   block permutation, null sums, pruning -- runs once per process; every batch of cells is
   split into world * n_dev contiguous shares of equal estimated cost, share
   rank * n_dev + l evaluated by local device l; the local shares land in one host array,
   and with several processes one exchange per batch completes it on every rank. */
#define FH_MAX_DEV 16

typedef struct {
  fsclg_ctx *ctx[FH_MAX_DEV];
  int dev[FH_MAX_DEV];
  int n_dev;                       /* open contexts (0: not yet opened) */
  int want_n;                      /* requested local devices: 0 default (one), -1 all visible */
  int want_dev[FH_MAX_DEV];
  const sm_ptable_t *tab_key;
  const snp_t *snp_key;
  int n_snps_key;
  uint64_t key;
  fh_rowmap_t rm;
  uint32_t *row;  /* row of every site (unpermuted) */
  void *rowp;     /* the same at the staging width */
  int rb;         /* staging width: 1, 2 or 4 bytes per row (the narrowest that holds the device rows) */
  int *chr_list;  /* permutation trials: the chromosomes whose null sum is read (window = whole chromosome,
                     n <= 2 eval_range + 1, init_scan_result); NULL: every chromosome */
  int n_chr_list;
  int32_t *pos;
  double *nullrow;
  int32_t *chr_start, *chr_n;
  int n_chr;
  void *stage[FSCLG_N_SLOTS];  /* one trial's rows (rb bytes each), read by every local device (fsclg_host_alloc) */
  int stage_cap, stage_rb;
  /* ranks */
  int rank, world;
  fscl_amd_exchange_fn xfn;
  void *xctx;
  fh_shm_t *shm;
  FILE *sim;                       /* FSCL_AMD_SIM record / replay file (development: scaling rehearsal) */
  int sim_replay;
  fscl_amd_stats_t st;
} dev_t_;
extern FH_HIDDEN dev_t_ D;

FH_HIDDEN int fh_dbg(void);
#define DBG(...) do { if (fh_dbg()) { fprintf(stderr, "[fscl_amd] " __VA_ARGS__); fflush(stderr); } } while (0)

/* the cost of a cell: its window size (snp_likelihood terms scale with it) */
static inline double fh_window_cost(int chr, int eval_range) {
  return (double)(D.chr_n[chr] < 2 * eval_range + 1 ? D.chr_n[chr] : 2 * eval_range + 1);
}

/* the arrays of one batch of an analysis scan, and its submit and wait (fh_run_on_devices, scan.c) */
typedef struct {
  const fsclg_run_t *runs;
  const double *la;            /* [run][n_la] */
  int n_la, eval_range;
  const size_t *poff, *coff;   /* the positions / cells of the runs before run i (blocks alone have coff) */
  const int32_t *clip;         /* conditional: 2 per position */
  const fsclg_blocks_t *blk;   /* blocks: per run */
  fscl_amd_curve_t *curves;    /* the results: per position; val and cnt per cell */
  fsclg_point_t *pts;
  double *val;
  uint32_t *cnt;
} dev_job_t;
typedef int (*dev_submit_fn)(int l, int lo, int hi, const dev_job_t *j);
typedef int (*dev_wait_fn)(int k, int lo, const dev_job_t *j);

/* scan.c */
FH_HIDDEN fh_rand_t *fh_perm_rng(void);
FH_HIDDEN int fh_env_int(const char *name, int dflt, int lo, int hi);
FH_HIDDEN void fh_dump_target(const char **fname, const char **label); /* what a SIGINT dump writes */
FH_HIDDEN void fh_dev_check(int r, const char *what);
FH_HIDDEN void fh_dev_open(void);
FH_HIDDEN uint64_t fh_hash_words(const void *p, size_t n, uint64_t h);
FH_HIDDEN uint64_t fh_tables_hash(const sm_ptable_t *sm, int n_depths);
FH_HIDDEN void fh_prepare(scan_t *s, sm_ptable_t *sm);
FH_HIDDEN void fh_chr_null_sums(const void *row, double *out); /* rows_impl.h at D.rb, for D.chr_list's chromosomes */
FH_HIDDEN void fh_dev_shares(const double *cost, int n, int *lo, int *hi);
FH_HIDDEN void fh_local_shares(const double *cost, int n, int *lo, int *hi);
FH_HIDDEN int fh_run_on_devices(const char *what, const int *lo, const int *hi, dev_submit_fn submit, dev_wait_fn wait,
                      double (*last_ms)(fsclg_ctx *, int), const dev_job_t *j, double *dev_ms,
                      unsigned long long *n_terms);
FH_HIDDEN double fh_dev_ms_max(const double *dev_ms);
FH_HIDDEN size_t *fh_run_offsets(const fsclg_run_t *runs, int n);
FH_HIDDEN void fh_exchange_points_flags(fsclg_point_t *out, int n, int lo, int hi, unsigned *flags);
FH_HIDDEN void fh_exchange_points(fsclg_point_t *out, int n, int lo, int hi);
FH_HIDDEN void fh_ranks_agree(const char *what, uint64_t word);
FH_HIDDEN void fh_eval_cells(const fsclg_cell_t *cells, int n, int eval_range, int bp_resl, fsclg_point_t *out);
FH_HIDDEN void fh_to_scan_pt(scan_pt_t *p, const fsclg_point_t *o);
FH_HIDDEN void fh_set_original_rows(void);
FH_HIDDEN int fh_runs_handle_begin(scan_t *s, sm_ptable_t *sm, const fsclg_run_t *runs, int n_runs, const uint32_t *rows,
                         int *slot);
FH_HIDDEN fsclg_cell_t *fh_scan_cells(const scan_t *s, int large_grid_sp, int *n_out);
FH_HIDDEN void fh_eval_cell_maxima(int slot, const fsclg_cell_t *cells, int n, int g, int eval_range, fsclg_point_t *out);
FH_HIDDEN int fh_grid_points_are(const scan_t *s, int small_grid_sp, int large_grid_sp); /* fscl_amd_scan_chromosome_grid's last */
FH_HIDDEN void fh_output_clr_null_distribution(const char *fname, scan_t *s);
/* trials.c */
FH_HIDDEN int fh_null_threads(void);
FH_HIDDEN void fh_pool_drop(void);
FH_HIDDEN void fh_spec_stop(void);
/* analyses.c */
FH_HIDDEN void fh_sampler_forget(void); /* the devices were closed: the sampler's tables went with them */

#endif
