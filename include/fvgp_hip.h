/*
 * fvgp_hip.h -- flat C ABI of the MI355X-native exact-GP engine (libfvgp_hip.so).
 *
 * The library replaces the numpy/scipy calls on fvGP's dense hot path.  Each entry point
 * names the reference interface it stands in for (paths relative to the lbl-camera/fvGP
 * root).  The reference is pure Python, so the binding a maintainer adds is a ctypes stub
 * (INTEGRATION.md); fvgp_amd/_lib.py is that stub.
 *
 * Conventions
 *   - every matrix is fp64, ROW-MAJOR (numpy / torch default) with an explicit leading
 *     dimension in elements; device pointers unless the parameter says "host";
 *   - square factor / covariance buffers are PADDED: rows and leading dimension are
 *     fvgp_hip_padded_dim(n) (a multiple of 128); the library owns the contents of the
 *     padding (identity on the diagonal, zero elsewhere) so every kernel runs on whole
 *     128x128 tiles;
 *   - only the LOWER triangle (i >= j) of a symmetric input / Cholesky output is defined,
 *     exactly like scipy.linalg.cho_factor(lower=True) (fvgp/gp_lin_alg.py:245);
 *   - the caller (torch tensors on the Python side) owns every buffer; the handle owns
 *     only its scratch (diagonal-block inverses, reduction slots);
 *   - return value: 0 ok; -k = argument k (1-based) is invalid (LAPACK style);
 *     >= 1000 = HIP runtime failure (text in fvgp_hip_last_error_string);
 *     "info" out-parameters follow dpotrf: 0, or the order of the first leading minor
 *     that is not positive definite.
 *   - a handle is bound to one device and one stream and is not thread-safe; distinct
 *     handles are independent.  Calls that return host scalars synchronise the stream;
 *     all others are asynchronous on it.
 */
#ifndef FVGP_HIP_H
#define FVGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fvgp_handle fvgp_handle;

/* stationary kernels of fvgp/kernels.py; theta = [signal variance, l_1..l_d] (ARD)
 * or [signal variance, l] (isotropic) */
enum fvgp_kernel_id {
    FVGP_KERNEL_RBF_ARD = 0,      /* hps[0]*squared_exponential_kernel(get_anisotropic_distance_matrix(..,hps[1:]),1)  kernels.py:16-33,461-481 */
    FVGP_KERNEL_MATERN32_ARD = 1, /* GPprior._default_kernel                                                            gp_prior.py:376-400 */
    FVGP_KERNEL_MATERN52_ARD = 2, /* gp_bo._surrogate_kernel                                                            gp_bo.py:115-126 */
    FVGP_KERNEL_RBF_ISO = 3,      /* hps[0]*squared_exponential_kernel(get_distance_matrix(x1,x2),hps[1])               kernels.py:440-458 */
    FVGP_KERNEL_MATERN32_ISO = 4, /* hps[0]*matern_kernel_diff1(get_distance_matrix, hps[1])                            kernels.py:98-118 */
    FVGP_KERNEL_MATERN52_ISO = 5  /* hps[0]*matern_kernel_diff2(get_distance_matrix, hps[1])                            kernels.py:166-188 */
};

enum fvgp_uplo { FVGP_FULL = 0, FVGP_LOWER = 1 };

#define FVGP_TILE 128
#define FVGP_MAX_DIM 16     /* input dimension limit of the assembly kernels */
#define FVGP_MATVEC_CHUNK 4096   /* rows of x2 per chunk sum of fvgp_hip_kmatvec (part of its bit contract) */
#define FVGP_PCG_MAX_RHS 16      /* right-hand sides per call of fvgp_hip_pcg */
#define FVGP_PCG_MAX_RANK 1024   /* largest rank of the pivoted-Cholesky preconditioner */
#define FVGP_LANCZOS_MAX_STEPS 256   /* most CG coefficients per column fvgp_hip_pcg_lanczos records */
#define FVGP_MAX_RHS_VEC 8  /* potrs switches from the GEMV path to the GEMM path above this */
#define FVGP_CHAIN_MAX_BLOCKS 32   /* widest panel (in 128-column blocks) the resident panel kernel takes; wider ones use the launch-per-step chain */
#define FVGP_BATCH_MAX_DIM 4096    /* largest per-problem square the batched evaluation takes (32 block columns) */

int fvgp_hip_version(void);
const char *fvgp_hip_last_error_string(void);
int64_t fvgp_hip_padded_dim(int64_t n);
/* rows AND columns of the square scratch fvgp_hip_loglik_rows wants for n points and ncol columns of y: padded_dim(n) while that
 * leaves ncol padding rows for the appended (y-m)^T, else 128 more (n a multiple of 128: gp_kv.py:589-593's forward solve then
 * rides in the factorisation for every n).  A scratch of only padded_dim(n) rows is accepted: the forward solve is then a sweep of
 * its own. */
int64_t fvgp_hip_loglik_dim(int64_t n, int ncol);
/* device bytes a handle allocates by itself for problems of n points (npred prediction points, 0 = none);
 * every N x N buffer is the caller's (gp_kv.py keeps Chol_factor / KVinvY as attributes the same way) */
int64_t fvgp_hip_workspace_bytes(int64_t n, int64_t npred);

/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL; it must outlive the handle
 * (fvgp_hip_destroy synchronises it) */
int fvgp_hip_create(fvgp_handle **out, int device, void *stream);
int fvgp_hip_destroy(fvgp_handle *h);
int fvgp_hip_sync(fvgp_handle *h);
/* a stream restricted to the compute units whose bits are set in cu_mask (mask_words x 32 bits), or an
 * ordinary non-blocking stream (high_priority 0/1) when cu_mask is NULL.  The row-sharded driver gives
 * the panel chain a few CUs of its own so its small kernels never queue behind the trailing update. */
int fvgp_hip_stream_create(void **out_stream, int device, int high_priority, const uint32_t *cu_mask, int mask_words);
int fvgp_hip_stream_destroy(void *stream);
/* Options.  Three keys are the library's interface; none changes a result except where noted "order": another, equally valid order of
 * the same sums (LAPACK accuracy either way: dpotrf behind gp_lin_alg.py:245 has no fixed order either).
 *   "schedule" ("order"): how a matrix is factored.
 *       0 = wide (default): panels of 4096 columns, each ONE resident kernel (csrc/chain.hip, a workgroup per 128 x 128 block) ALONE on
 *           the chip, followed by ONE trailing update with K = the panel's width; a panel over at least 16384 rows goes in sub-panels of
 *           2048 columns with the update kernel bringing the rest of the panel up to date in between;
 *       1 = lookahead: panels of 2048 / 1024 / 512 columns, the next panel factored on a high-priority side stream under the trailing
 *           update (the default until round 5; the row-sharded driver still runs its stacked panels this way);
 *       2 = narrow: the same panels, three launches per 128 columns instead of the resident kernel (panels wider than 4096 columns
 *           always take this form).
 *   "profile" (0/1): time the trailing-update launches with HIP events -> fvgp_hip_get_profile.
 *   "chain_verify" (0/1): checksummed hand-offs of the resident panel kernel, see fvgp_hip_chain_verify_counts.
 * Everything below is a MEASUREMENT knob underneath one of the schedules -- kept because each has a test
 * (tests/test_gpu_primitives.py) and a measured A/B behind its default; not an interface, no promise that a key
 * survives a round:
 *   wide: "chain_wide" (1), "wide_block" = 4096 ("wide_block_big" while more than "wide_threshold" rows remain), "wide_inner" = 2048 and
 *       "wide_inner_rows" = 16384 (the sub-panels);
 *   lookahead / narrow: "lookahead_min" (2^40 = off; padded size from which look-ahead runs, 4608 under schedule 1), "lookahead" (1),
 *       "outer_block" (1024; "outer_block_big" = 2048 while more than "big_threshold" = 24576 rows remain, "outer_block_small" = 512
 *       for the last "small_threshold" = 12288; any multiple of 128),
 *   panel chain: "panel_chain" (1: one resident kernel per panel -- in the look-ahead schedule for panels with at least
 *       "panel_chain_min" = 4096 rows below their first column -- and for the row-sharded driver's stacked panel; 0: three launches
 *       per 128 columns ("inner_block" / "panel_recursive": how those split a panel); 2: in the row-sharded driver a workgroup per
 *       block ROW below the square instead of per block) ("order"), "chain_sleep_rows" (96: in panels of at most this many block rows
 *       a block's early products yield their compute unit to a leaf or to the block the next leaf waits for), "chain_single_rows"
 *       (80: panels of at most this many block rows run one workgroup per compute unit), "chain_ahead" (0 = plain column order: alone on
 *       the chip the diagonal block and the two blocks under it of the next block columns are started this many columns ahead of the
 *       other blocks; the leaves of a tall panel end earlier, the launch does not: profiles/r06_chain_ahead_ab.txt),
 *       "cols_split" (look-ahead schedule; 1: while at most "cols_split_rows" = 8192 rows remain only the next panel's square is
 *       brought up to date before its resident kernel starts; the rows below follow on the main stream and the kernel's block rows
 *       wait for a flag in memory),
 *       "leaf_tiles" / "leaf_tiles_rows" / "k128_kernels" / "small_tile_max" / "small_tile_max_update" (kernels of the three-launch
 *       chain) ("order"), "leaf_yield" / "chain_yield" (1: the trailing update's waves sleep while a workgroup of the chain shares
 *       their compute unit; chain_yield 2: also for the resident kernel's rows below the square); "tile_tables" (1: XCD-balanced
 *       block -> tile tables instead of the formula map);
 *   solves / posterior / gradient: "bwd_sweep" / "fwd_sweep" (1: the backward / forward vector sweep with one right-hand side in
 *       one launch), "block_inverses" (1: the posterior substitutes with inverted diagonal blocks) ("order"), "posterior_block"
 *       (2048 / 1024: width of those blocks up to 1024 prediction points; 1024 beyond) ("order"), "posterior_halves" (1: 512-1024
 *       points as two halves on two streams) ("order"), "potri_kminor" (1: POTRI on (M,K) x (N,K) products only) ("order");
 *   batch selection: "select_block" (65536: candidates per pair of launches of fvgp_hip_select_batch, a multiple of 64, at most 65536;
 *       the results have the same bits for every value);
 *   matrix-free product: "matvec_split" (0: fvgp_hip_kmatvec deals chunk ranges of x2 over gridDim.y only while the 64-row blocks of
 *       x1 cannot fill the chip; 1: never; k: over k workgroups per 64 rows; the results have the same bits for every value);
 *   diagnostics: "chain_stamps" / "leaf_stamps" (device pointers, 0 = off: in-kernel timestamps of the panel kernel's hand-offs /
 *       the leaf's phases).
 * The library reads no environment variable.  The Python binding (fvgp_amd/_lib.py, Handle) applies FVGP_<KEY>=<integer> for the keys
 * it lists -- every key above but "profile" and the two diagnostics pointers -- once, when it creates a handle. */
int fvgp_hip_set_option(fvgp_handle *h, const char *key, int64_t value);
/* Option "chain_verify" (0/1, default 0): every in-launch hand-off of the resident panel kernel (csrc/chain.hip: a solved block row,
 * a factored diagonal block with its tile inverses) carries a checksum of its payload, taken by the producer from what it stores and
 * compared by every consumer with what ARRIVED (LDS images of its LDS-DMA loads, registers of its buffer loads).  out2_host[0] =
 * mismatches, [1] = comparisons since the last call; synchronises.  A verifying run is slower (LDS reductions on the chain's critical
 * path) and returns the same bits.  The dpotrf it guards: gp_lin_alg.py:245. */
int fvgp_hip_chain_verify_counts(fvgp_handle *h, int64_t *out2_host);
/* out[0] = number of trailing-update launches of the last potrf, out[1] = their summed
 * duration in ms, out[2] = their summed algorithmic flops, out[3] = whole-potrf ms; of the last fused
 * evaluation (fvgp_hip_loglik): out[4] = covariance-assembly ms, out[5] = its algorithmic bytes (lower
 * 128-tiles written once), out[6] = ms of everything after the factorisation (backward solve, reductions);
 * out[7] = host milliseconds the last row-sharded evaluation (fvgp_hip_loglik_dist) took to ENQUEUE (no synchronisation inside).
 * out needs 8 doubles. */
int fvgp_hip_get_profile(fvgp_handle *h, double *out8_host);
/* the same eight, then out[8] = summed ALGORITHMIC bytes of those trailing-update launches (every C tile read and written once, the
 * panel's rows read once: what bench.py's roofline.traffic is compared with); out[9..15] reserved (0).  out needs 16 doubles. */
int fvgp_hip_get_profile_ex(fvgp_handle *h, double *out16_host);
/* The handle keeps the inverted 128 x 128 diagonal blocks of the LAST factor it produced or solved with, keyed
 * on (pointer, n, ld).  A caller that fills a factor buffer by any other means than fvgp_hip_potrf / _loglik
 * (upload of a pickled factor, bordering update, device-to-device copy: gp_kv.py:462-476,718-765) must call
 * this before the next potrs / trsm / potri / posterior on that buffer -- an allocator may hand back the
 * address of a freed factor of the same size. */
int fvgp_hip_invalidate_factor(fvgp_handle *h);

/* ---- covariance assembly -------------------------------------------------------------
 * replaces GPprior.compute_covariances -> kernel(x1,x2,hps) (gp_prior.py:217-224) and,
 * with vdiag, GPkv.addKV (gp_kv.py:639-669) fused into the same pass.
 * x1 (n1,d), x2 (n2,d) row-major device; theta host; K (rows, ldk).
 * uplo = FVGP_LOWER writes only tiles on/below the diagonal (requires x1 == x2 semantics).
 * pad != 0: K has padded_dim(n1) rows and ldk >= padded_dim(n2); padding is written
 *           (1 on the diagonal, else 0).  pad == 0: exactly n1 x n2 entries are written. */
int fvgp_hip_kmat(fvgp_handle *h, int kernel_id, const double *x1, int64_t n1, const double *x2, int64_t n2,
                  int d, const double *theta_host, int ntheta, const double *vdiag_or_null,
                  double *K, int64_t ldk, int uplo, int pad);

/* ---- dense Cholesky ------------------------------------------------------------------
 * potrf  : calculate_Chol_factor   gp_lin_alg.py:237-269   (scipy cho_factor -> dpotrf)
 * potrs  : calculate_Chol_solve    gp_lin_alg.py:289-328   (cho_solve -> dpotrs)
 * logdet : calculate_Chol_logdet   gp_lin_alg.py:331-360   (2*sum(log|diag|))
 * potri  : calculate_inv_from_chol gp_lin_alg.py:1558-1566 (KV^-1 from L), lower triangle
 * A / L: padded_dim(n) rows, lda >= padded_dim(n).  B: (padded_dim(n), ldb) row-major,
 * nrhs columns used; rows >= n of B are overwritten with zeros. */
int fvgp_hip_potrf(fvgp_handle *h, double *A, int64_t n, int64_t lda, int *info_host);
/* potrf without the host round trip (the row-sharded driver factors one diagonal block per panel and must
 * not drain the stream): info goes to `info_dev` (device int), 2*sum(log|diag|) of the first n_logdet
 * rows to `logdet_dev` (device double, may be null).  Enqueue only. */
int fvgp_hip_potrf_dev(fvgp_handle *h, double *A, int64_t n, int64_t lda, int64_t n_logdet, int *info_dev, double *logdet_dev);
int fvgp_hip_potrs(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb);
int fvgp_hip_logdet(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *out_host);
int fvgp_hip_potri(fvgp_handle *h, double *L, int64_t n, int64_t ldl, double *work, int64_t ldw);
/* forward half only: B <- L^-1 B (the new rows of an append, gp_lin_alg.py:1310-1477; the posterior covariance of kernel callables,
 * gp_posterior.py:120-136).  One column: the one-launch forward sweep; 128 .. 1024 columns against >= 2048 rows: the right-hand
 * sides are transposed into handle scratch (nrhs x padded_dim(n) doubles) and swept with the inverted 1024 x 1024 diagonal blocks. */
int fvgp_hip_trsm_lower(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb);

/* backward half only: B <- L^-T B, nrhs a multiple of 128 (GEMM path) */
int fvgp_hip_trsm_lower_t(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb);

/* ---- row-sharded (multi-GPU) building blocks: the gp2Scale partitioning pattern -----------
 * (fvgp/gp2Scale_covariance.py:381-396, gp_prior.py:319-322) applied to a DENSE factorisation:
 * 128-row blocks of K+V are dealt block-cyclically to the ranks, x is replicated.
 * panel_trsm   : P (rows, nd) <- P * L_D^-T with D the factored nd x nd diagonal block (nd % 128 == 0)
 * syrk_rowshard: C[ti][tj] -= A[ti] B[tj]^T for the 128x128 tiles with tj <= ti*scale + off, i.e. the
 *                lower-triangular part of the trailing update restricted to this rank's block rows
 *                (scale = number of ranks, off = global offset of the first local block row, may be < 0);
 *                A (M,K), B (N,K), C (M,N) row-major.  B may be used as an all-gather leaves it:
 *                b_ranks chunks of b_blocks 128-row blocks each, chunk q holding the cyclic blocks
 *                q, q + b_ranks, ...; tile column tj reads cyclic block tj + b_off
 *                (b_ranks = 1, b_off = 0: plain row order). */
int fvgp_hip_panel_trsm(fvgp_handle *h, const double *D, int64_t nd, int64_t ldd, double *P, int64_t rows, int64_t ldp);

/* ---- row-sharded (multi-GPU) evaluation: one process per GPU, RCCL over xGMI ---------------------------------
 * Stands in for the reference's distribution switch and scheduler: GP(..., gp2Scale=True, dask_client=...) (gp.py:419-439),
 * GPprior._gp2Scale_covariance / distributed_covariance (gp_prior.py:324-347, gp2Scale_covariance.py:313-431) and the
 * broadcast of x (gp_prior.py:319-322) -- with a dense factorisation behind it.
 *
 * Collectives are function pointers on device buffers, enqueued on `stream`: fvgp_hip_comm_init binds RCCL
 * (ncclAllGather / ncclAllReduce on a communicator built from the 128-byte ncclUniqueId of fvgp_hip_comm_unique_id, which
 * rank 0 hands to the others by any means -- torch.distributed's store on the Python side); fvgp_hip_comm_init_callbacks
 * binds the caller's own (the CPU tests bind gloo).  bytes = what this rank receives (bookkeeping for the timings). */
typedef struct fvgp_collectives {
    void *ctx;
    int (*all_gather)(void *ctx, const double *send, double *recv, int64_t count_per_rank, void *stream);    /* recv: nranks x count */
    int (*all_reduce_sum)(void *ctx, double *buf, int64_t count, void *stream);                             /* in place */
} fvgp_collectives;
int fvgp_hip_comm_unique_id(void *out128_host);
int fvgp_hip_comm_init(fvgp_handle *h, const void *unique_id128_host, int rank, int nranks);
int fvgp_hip_comm_init_callbacks(fvgp_handle *h, const fvgp_collectives *cb, int rank, int nranks);
int fvgp_hip_comm_destroy(fvgp_handle *h);
/* Direct collectives over peer mappings instead of a collective library (csrc/ipc.hip): the reference's workers hand covariance
 * blocks to each other directly (gp_prior.py:301-322, gp2Scale_covariance.py:419-420).  The payload moves by hipMemcpyAsync
 * between IPC mappings (copy engines, every peer at once); the only kernels are one-wave flag writers / pollers.
 *   ipc_window   : allocates this rank's window (window_bytes, two halves: a call moves at most window_bytes / 2 per piece) and
 *                  returns its 64-byte IPC handle (host); every rank hands its handle to every other by any means;
 *   comm_init_ipc: all_handles64_host = nranks x 64 bytes in rank order; shm_name = a POSIX shared-memory name ("/fvgp_...") that is
 *                  NEW for this communicator and the same on every rank (the flag words live there; unlink it once every rank has
 *                  returned).  Binds the handle's collectives like fvgp_hip_comm_init.  nranks <= 16. */
int fvgp_hip_ipc_window(fvgp_handle *h, int64_t window_bytes, void *out_handle64_host);
int fvgp_hip_comm_init_ipc(fvgp_handle *h, const void *all_handles64_host, const char *shm_name, int rank, int nranks);
/* the handle's collectives on its stream (the parts of the sharded path that are sequenced by the caller: backward solve,
 * posterior, gradient -- gp_kv.py:574-593, gp_posterior.py:139-288 on the distributed factor) */
int fvgp_hip_all_reduce(fvgp_handle *h, double *buf, int64_t count);
int fvgp_hip_all_gather(fvgp_handle *h, const double *send, double *recv, int64_t count_per_rank);
/* out[0..1] = calls, out[2..3] = bytes received, out[4..5] = milliseconds on the chain stream of the all_gather /
 * all_reduce calls since the last call of this function (option "profile" on); out needs 6 doubles */
int fvgp_hip_comm_profile(fvgp_handle *h, double *out6_host);
/* what the handle's communicator is, as the communicator itself reports it (the reference's analogue: the Dask client's own view of its
 * workers, gp_prior.py:319-322): out[0] = 0 none / 1 RCCL / 2 direct IPC / 3 caller's callbacks, out[1] = nranks and out[2] = rank as
 * bound; RCCL only: out[3] = ncclCommCount, out[4] = ncclCommUserRank, out[5] = ncclCommCuDevice, out[6] = ncclGetVersion; -1 where
 * not applicable.  out needs 8 int64. */
int fvgp_hip_comm_info(fvgp_handle *h, int64_t *out8_host);
/* 0, or 2200 once a poll of the direct (IPC) collectives has given up waiting for a peer: everything the collectives delivered since is
 * stale.  Ask after synchronising; fvgp_hip_sync and every entry that returns host values do (they fail with 2200 instead of
 * returning results computed from stale windows).  The condition is sticky: destroy the communicator and build a new one. */
int fvgp_hip_comm_check(fvgp_handle *h);

/* One GP sharded over the ranks.  Every buffer is the caller's (sizes in doubles from fvgp_hip_dist_workspace):
 *   x_all (n, d) and vdiag (n) replicated; zt (128, np): (y-m)^T in the first ncol rows, zeros below;
 *   A ((nb_max + 1) * 128, np): this rank's block rows (local block l = global block l * nranks + rank) and the block of
 *   right-hand-side rows; T[2], recv[2], Dfac, gather: panel buffers (nranks > 1 or force_general); info_dev (npan ints)
 *   and logdet_dev (npan doubles): per-panel results, on the device.
 * np = padded_dim(n), nb_max = ceil(np / 128 / nranks), npan = ceil(np / panel). */
typedef struct fvgp_dist_desc {
    int64_t n; int d; int ncol; int64_t panel; int rank, nranks; int kernel_id;
    const double *x_all; const double *vdiag; const double *zt;
    double *A; double *T[2]; double *recv[2]; double *Dfac; double *gather;
    int *info_dev; double *logdet_dev;
    int keep_factor;      /* 0: likelihood only -- the factored panels are not copied back into A (no solve can follow) */
    int force_general;    /* 1: a single rank still takes the panel-buffer / collective path (exercises RCCL on one GPU) */
    int preassembled;     /* 1: the caller has filled A's block rows with its rows of K (host kernel callables, matrix-valued noise
                           *    already added; zero padding rows): the driver adds vdiag / the identity padding and (y-m)^T only */
} fvgp_dist_desc;
/* out[0] A, [1] each T, [2] each recv, [3] Dfac, [4] gather (doubles); [5] = npan */
int fvgp_hip_dist_workspace(const fvgp_dist_desc *d, int64_t *out6);
/* GPMarginalLikelihood.log_likelihood(theta) (gp_marginal_likelihood.py:137-179) on the sharded matrix: assembly of the
 * rank's rows, blocked right-looking Cholesky with one panel of look-ahead (per panel: all-gather of the diagonal block from
 * its owners, factorisation of the tall panel, all-gather of the panel factor, trailing update of the rank's block rows),
 * the forward solve riding along.  out_host = {log-likelihood, log|KV|, (y-m)^T KV^-1 (y-m) / ncol}, replicated;
 * *info_host = dpotrf's info (global index of the first non-positive pivot) or 0.  One host synchronisation. */
int fvgp_hip_loglik_dist(fvgp_handle *h, const fvgp_dist_desc *d, const double *theta_host, int ntheta, double *out_host, int *info_host);
/* After fvgp_hip_loglik_dist with keep_factor = 1 -- the rank's block rows of L in A, the factored diagonal blocks replicated in
 * Dfac -- the rest of what the reference's distributed mode answers through the same object (gp_kv.py:574-593,
 * gp_posterior.py:139-288, tests/test_fvgp.py:3112-3149), each ONE call per rank (collectives issued from the library):
 *   solve_dist     : KVinvY = L^-T z, replicated: alpha_out (np x 128 row-major device; columns >= ncol are zero);
 *   posterior_dist : k^T KVinvY -> mean_out (pp x 128) and kk - k^T KV^-1 k -> S_out (pp x pp, may be null), replicated,
 *                    pp = padded_dim(npred).  Kernel callables: k_pre = the rank's rows of k(x_data, x_pred)
 *                    (nb_max*128 x pp, block l = global block l*nranks + rank, zero padded) and kk_pre = k(x_pred, x_pred)
 *                    (pp x pp, read on rank 0 only) assembled by the caller; else null and xpred (npred x d) is given;
 *   grad_dist      : 1/2 (tr(KV^-1 dK_i) - b^T dK_i b), b = alpha[:, component] (gp_marginal_likelihood.py:262-300) for the
 *                    kernel-owned hyperparameters -> grad_host (ntheta), replicated; diag_out (np device doubles or null)
 *                    receives diag(KV^-1).  The rank's rows of inv(L) (N^2 / nranks doubles) live in the scratch; the Gram
 *                    matrix is walked in column slabs of `slab` columns (a multiple of 128).
 * ws: caller-owned device scratch of fvgp_hip_dist_scratch(d, what, npred, slab) doubles, what = 0 solve, 1 posterior, 2 gradient. */
int64_t fvgp_hip_dist_scratch(const fvgp_dist_desc *d, int what, int64_t npred, int64_t slab);
int fvgp_hip_solve_dist(fvgp_handle *h, const fvgp_dist_desc *d, double *alpha_out, double *ws);
int fvgp_hip_posterior_dist(fvgp_handle *h, const fvgp_dist_desc *d, const double *theta_host, int ntheta, const double *xpred, int64_t npred,
                            const double *k_pre, const double *kk_pre, const double *alpha, double *mean_out, double *S_out, double *ws);
int fvgp_hip_grad_dist(fvgp_handle *h, const fvgp_dist_desc *d, const double *theta_host, int ntheta, const double *alpha, int component,
                       int64_t slab, double *grad_host, double *diag_out, double *ws);
/* one tall panel T (rows x w, row-major, ldt): the w x w diagonal block on top (lower triangle; the first
 * n_valid rows are data, the rest identity padding), this rank's rows of the panel below it.  Factors the top
 * block and solves the rows below against it, 128 columns at a time (leaf, TRSM by the inverted diagonal tile,
 * in-panel update), exactly as the single-GPU driver treats a panel.  Enqueue only: info -> info_dev,
 * 2*sum(log diag) of the first n_valid rows -> logdet_dev (may be null). */
int fvgp_hip_panel_potrf_dev(fvgp_handle *h, double *T, int64_t w, int64_t rows, int64_t ldt, int64_t n_valid,
                             int *info_dev, double *logdet_dev);
int fvgp_hip_syrk_rowshard(fvgp_handle *h, int64_t M, int64_t N, int64_t K, const double *A, int64_t lda,
                            const double *B, int64_t ldb, double *C, int64_t ldc, int scale, int off,
                            int b_ranks, int b_blocks, int b_off);

/* ---- fused evaluations ----------------------------------------------------------------
 * loglik: GPMarginalLikelihood.log_likelihood(theta)  gp_marginal_likelihood.py:137-179
 *         = kernel -> addKV -> potrf -> potrs -> logdet -> scalar, nothing leaves HBM.
 *   ymean  (n, ncol) row-major = y - m   (default mean: gp_prior.py:449-458, done by caller)
 *   KV     scratch of padded_dim(n) rows at leading dimension ld >= padded_dim(n); holds the factor L of the n x n matrix (identity
 *          on the padding) on return.  NOTHING below row padded_dim(n) is read or written, whatever ld is (a pitched buffer, a row
 *          slice of a larger arena): where n leaves fewer than ncol padding rows the forward solve is a sweep of its own.
 *          fvgp_hip_loglik_rows takes the number of rows the caller really owns: with kv_rows and ld >= fvgp_hip_loglik_dim(n, ncol)
 *          the appended (y-m)^T rows go into the extra block row and the forward solve is fused for every n (rows
 *          padded_dim(n) .. kv_rows - 1 are identity padding again on return)
 *   alpha  (padded_dim(n), ncol) receives KVinvY
 *   out_host[0] = log marginal likelihood, [1] = log|KV|, [2] = sum((y-m)*KVinvY)/ncol
 *   vdiag is REQUIRED here (n positive noise variances, gp_likelihood.py:89-110): returns -8 when NULL;
 *   every entry must be positive (the facade takes the unfused kmat/potrf/potrs route otherwise). */
int fvgp_hip_loglik(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                    const double *theta_host, int ntheta, const double *vdiag,
                    const double *ymean, int ncol, double *KV, int64_t ld,
                    double *alpha, double *out_host, int *info_host);
int fvgp_hip_loglik_rows(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                         const double *theta_host, int ntheta, const double *vdiag,
                         const double *ymean, int ncol, double *KV, int64_t kv_rows, int64_t ld,
                         double *alpha, double *out_host, int *info_host);

/* loglik_batch: GPMarginalLikelihood.log_likelihood (gp_marginal_likelihood.py:137-179) at B hyperparameter vectors on the same
 * resident x, in one call -- the objective of a population-based optimiser (differential_evolution scores a whole population per
 * generation: fvgp/gp_training.py:66-76) or of a grid scan.  B independent factorisations side by side fill the chip where one at
 * training sizes cannot (csrc/batch.hip: per 128 columns a leaf and a panel-TRSM launch, trailing updates between halves of a
 * recursive halving over the block columns, every launch over all B problems).
 *   thetas_host   B x ntheta, row-major, host
 *   vdiag         n noise variances per problem (all > 0); problem b reads vdiag + b * vdiag_stride (0 = shared by all)
 *   ymean         (n, ncol) per problem = y - m(theta_b); problem b reads ymean + b * ymean_stride (0 = shared)
 *   KV            caller-owned scratch: problem b's square at KV + b * kv_stride, fvgp_hip_loglik_batch_dim(n, ncol) rows at leading
 *                 dimension ld (ld even, kv_stride even and >= dim * ld when B > 1, KV 16-byte aligned); contents on return unspecified;
 *                 nothing outside the B dim x dim squares is touched; the strict upper triangle of each square is never read
 *   out_host      B x 3: {log-likelihood, log|KV|, (y-m)^T KV^-1 (y-m) / ncol}, NaN for a problem whose factorisation failed
 *   info_host     B dpotrf info words (0, or the order of the first non-positive leading minor); may be NULL
 * Errors (argument numbers): -4 n past FVGP_BATCH_MAX_DIM (or fvgp_hip_loglik_batch_dim(n, ncol) == 0), -13 ncol outside 1..8
 * (FVGP_MAX_RHS_VEC), -8 B < 1.  Returns 0 even when some problems are not positive definite (their info says so).  One host
 * synchronisation per call.  Problem b's results are bitwise the same whatever B is, whatever position b holds and whatever else is in
 * the batch (kernel variants depend on the per-problem shape only, per-problem fixed-order reductions, no split K); they agree with
 * fvgp_hip_loglik to rounding (another schedule of the same factorisation). */
int fvgp_hip_loglik_batch(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                          const double *thetas_host, int ntheta, int64_t B,
                          const double *vdiag, int64_t vdiag_stride, const double *ymean, int64_t ymean_stride, int ncol,
                          double *KV, int64_t ld, int64_t kv_stride, double *out_host, int *info_host);
/* rows = columns of ONE problem's square in the batched scratch: fvgp_hip_loglik_dim(n, ncol); 0 when that exceeds FVGP_BATCH_MAX_DIM */
int64_t fvgp_hip_loglik_batch_dim(int64_t n, int ncol);
/* device bytes the HANDLE allocates for a batch of B problems (the block inverse of the current step, reciprocal pivots, the theta
 * table, reductions and info word per problem); -1 for invalid arguments */
int64_t fvgp_hip_loglik_batch_workspace_bytes(int64_t n, int ncol, int64_t B);

/* loglik_grad_batch: fvgp_hip_loglik followed by fvgp_hip_loglik_grad at each of B hyperparameter vectors on the same resident x, in
 * one call -- the step of a multi-start gradient optimiser (csrc/grad_batch.hip: the batched factorisation of fvgp_hip_loglik_batch
 * with every leaf inverse kept, W = L^-1 by recursive halving, b = W^T z, KV^-1 = W^T W, the fused trace and a per-problem reduction,
 * every launch over all B problems).  Arguments 1-13 as fvgp_hip_loglik_batch, then:
 *   component     which column of y - m gives b (0 <= component < ncol), as in fvgp_hip_loglik_grad
 *   KV, ld, kv_stride    as fvgp_hip_loglik_batch (contents on return: KV^-1 in the lower tiles of the padded_dim(n) square)
 *   work, ldw, work_stride   a second caller-owned square per problem, padded_dim(n) rows at leading dimension ldw (even, >= padded_dim(n);
 *                 work_stride even and >= padded_dim(n) * ldw when B > 1; 16-byte aligned); contents on return unspecified
 *   out_host      B x 3, each value bitwise equal to what fvgp_hip_loglik_batch returns for that theta
 *   grad_host     B x ntheta: g_i = 1/2 sum_jk (KV^-1_jk - b_j b_k) dK_jk/dtheta_i for the kernel-owned hyperparameters, 0 for the rest
 *   info_host     B dpotrf info words (may be NULL); a problem with info > 0 gets NaN in its out_host and grad_host rows
 *   b_out         optional device B x n: b = KV^-1 (y - m)[:, component]
 *   diag_out      optional device B x n: diag(KV^-1)
 * Errors (argument numbers): -4 n past FVGP_BATCH_MAX_DIM, -8 B < 1, -13 ncol outside 1..8, -14 component, -15..-17 KV, -18..-20 work,
 * -21 / -22 missing out_host / grad_host.  One host synchronisation per call.  Problem b's results are bitwise the same whatever B is,
 * whatever position b holds and whatever else is in the batch. */
int fvgp_hip_loglik_grad_batch(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                               const double *thetas_host, int ntheta, int64_t B,
                               const double *vdiag, int64_t vdiag_stride, const double *ymean, int64_t ymean_stride,
                               int ncol, int component,
                               double *KV, int64_t ld, int64_t kv_stride,
                               double *work, int64_t ldw, int64_t work_stride,
                               double *out_host, double *grad_host, int *info_host,
                               double *b_out, double *diag_out);
/* device bytes the HANDLE allocates for fvgp_hip_loglik_grad_batch (per problem: every leaf inverse, reciprocal pivots, the theta table
 * row, z and b, the trace's partial sums for 1 + FVGP_MAX_DIM hyperparameters, two reductions, the gradient row, the info word);
 * -1 for invalid arguments or where fvgp_hip_loglik_batch_dim(n, ncol) is 0 */
int64_t fvgp_hip_loglik_grad_batch_workspace_bytes(int64_t n, int ncol, int64_t B);

/* posterior_batch: GPposterior.posterior_mean / posterior_covariance (gp_posterior.py:139-182, 229-288, 120-136) at B hyperparameter
 * vectors on the same resident x and the same P prediction points, in one call -- a prediction averaged over the theta samples of an
 * MCMC run, the end points of a multi-start optimiser side by side, a theta grid.  With V = L^-1 k(x, x*) and z = L^-1 (y - m):
 * mean = V^T z, var = k(x*, x*) - colsumsq(V), S = k(x*, x*) - V^T V, no backward solve (csrc/posterior_batch.hip: the prediction rows
 * k(x*, x; theta_b) ride under each problem's square through the batched factorisation of fvgp_hip_loglik_batch, which leaves them as
 * V^T; a streaming epilogue per chunk of points; every launch over all B problems).  Arguments 1-13 as fvgp_hip_loglik_batch, then:
 *   xpred         (P, d) device, shared by all problems
 *   KV            caller-owned tall scratch: problem b's at KV + b * kv_stride, kv_rows = fvgp_hip_loglik_batch_dim(n, ncol) + P_chunk rows
 *                 at leading dimension ld (even, >= dim; kv_stride even and >= kv_rows * ld when B > 1; 16-byte aligned), P_chunk a
 *                 multiple of 128 (>= 128) of the caller's choice.  The top dim rows are fvgp_hip_loglik_batch's square, the P_chunk rows
 *                 below take the prediction rows: P > P_chunk points go through them chunk by chunk (the first rides in the
 *                 factorisation, the others take a solve-only pass of the same recursion by the kept leaf inverses), with the same
 *                 bits whatever P_chunk is.  Contents on return unspecified
 *   mean_out      (B, P, ncol) device = V^T z (prior mean added by the caller, as fvgp_hip_posterior)
 *   var_out       (B, P) device or NULL = k(x*, x*) - colsumsq(V), unclipped
 *   S_out         NULL, or B squares of padded_dim(P) rows at leading dimension lds (even, >= padded_dim(P)), problem b's at
 *                 S_out + b * s_stride (even, >= padded_dim(P) * lds when B > 1; 16-byte aligned): kk - k^T KV^-1 k, full and bitwise
 *                 symmetric (the lower tiles are computed, with K ending at padded_dim(n) over prediction rows whose columns from n on
 *                 the epilogue has zeroed, and mirrored).  Needs all points in one chunk: P <= P_chunk
 *   out_host      NULL, or B x 3: bitwise what fvgp_hip_loglik_batch returns for the same arguments (the top squares see the same
 *                 launches on the same data)
 *   info_host     B dpotrf info words (may be NULL); a problem with info > 0 gets NaN in its mean_out / var_out / S_out (and out_host)
 *                 rows and does not disturb its neighbours
 * Errors (argument numbers): -4 n past FVGP_BATCH_MAX_DIM (or fvgp_hip_loglik_batch_dim(n, ncol) == 0), -8 B < 1, -13 ncol outside
 * 1..8, -14 xpred, -15 P < 1, -16 KV, -17 kv_rows (dim + a multiple of 128 >= 128), -18 ld, -19 kv_stride, -20 mean_out, -22 S_out
 * (P > P_chunk or alignment), -23 lds, -24 s_stride; nothing is launched then.  One host synchronisation per call.  Problem b's outputs
 * are bitwise the same whatever B is, whatever position b holds and whatever else is in the batch (a failing theta included): every sum
 * of a prediction row sees that row and its problem's factor only, in a fixed order; they agree with fvgp_hip_loglik + fvgp_hip_posterior
 * to rounding (another schedule of the same sums). */
int fvgp_hip_posterior_batch(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                             const double *thetas_host, int ntheta, int64_t B,
                             const double *vdiag, int64_t vdiag_stride, const double *ymean, int64_t ymean_stride, int ncol,
                             const double *xpred, int64_t P,
                             double *KV, int64_t kv_rows, int64_t ld, int64_t kv_stride,
                             double *mean_out, double *var_out, double *S_out, int64_t lds, int64_t s_stride,
                             double *out_host, int *info_host);
/* device bytes the HANDLE allocates for fvgp_hip_posterior_batch (per problem: every leaf inverse -- dim / 128 blocks of 128 x 128 --,
 * dim reciprocal pivots, the theta table row of 1 + FVGP_MAX_DIM, two reductions, the info word; the prediction rows live in the
 * caller's scratch, so P_chunk only has to be valid); -1 for invalid arguments or where fvgp_hip_loglik_batch_dim(n, ncol) is 0 */
int64_t fvgp_hip_posterior_batch_workspace_bytes(int64_t n, int ncol, int64_t B, int64_t P_chunk);

/* loglik_grad: GPMarginalLikelihood.neg_log_likelihood_gradient  gp_marginal_likelihood.py:224-309
 *   g_i = 1/2 sum_jk (KVinv_jk - b_j b_k) dK_jk/dtheta_i,  b = KVinvY[:,component];
 *   dK/dtheta re-evaluated on the fly (gp_prior.py:421-436, gp_bo.py:167-201).
 *   KV on entry: the factor L from fvgp_hip_loglik / potrf (destroyed: holds KV^-1 lower on return)
 *   work: second padded_dim(n) x ld scratch.  grad_host: ntheta doubles. */
int fvgp_hip_loglik_grad(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                         const double *theta_host, int ntheta, const double *alpha, int ncol, int component,
                         double *KV, int64_t ld, double *work, int64_t ldw, double *grad_host);

/* loglik_hess: the exact Hessian of the negative log marginal likelihood in the hyperparameters the named kernel owns, with the
 * gradient of fvgp_hip_loglik_grad from the same call (no counterpart in the reference, whose gp_marginal_likelihood.py:312-336
 * differences the gradient).  With W = KV^-1, b = KVinvY[:, component], K_i = dK/dtheta_i, G_i = W K_i W, w_i = W K_i b:
 *   H_ij = 1/2 sum_ab (W - b b^T)_ab (d2K/dtheta_i dtheta_j)_ab - [ 1/2 tr(G_i K_j) - b^T K_j w_i ]
 *   KV on entry: the factor L from fvgp_hip_loglik / potrf (its strict upper triangle is never read) -- any lower factor, with any
 *   alpha: W is the inverse of L L^T.  KV, work and work2 -- three padded_dim(n)-row scratches, each 16-byte aligned with an even
 *   leading dimension >= padded_dim(n) -- are destroyed: KV holds KV^-1, both triangles, on return (nothing writes it after the
 *   mirror), work and work2 the last hyperparameter's products.
 *   ws: device scratch of fvgp_hip_loglik_hess_workspace_bytes(n, d) bytes, 8-byte aligned.
 *   grad_host: ntheta doubles (kernel-owned entries, the rest 0).
 *   hess_host: nk x nk doubles, row-major, nk = the kernel's parameter count (d + 1, or 2 for an isotropic kernel): the RAW block --
 *   row i comes from G_i, so H_ij and H_ji are two independent computations; a caller wanting a symmetric matrix averages them.
 * A bad argument returns minus its position before anything is launched or written.  One synchronisation. */
int64_t fvgp_hip_loglik_hess_workspace_bytes(int64_t n, int d);          /* -1 for n < 1 or d outside 1..FVGP_MAX_DIM */
int fvgp_hip_loglik_hess(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                         const double *theta_host, int ntheta, const double *alpha, int ncol, int component,
                         double *KV, int64_t ld, double *work, int64_t ldw, double *work2, int64_t ldw2,
                         double *ws, int64_t ws_bytes, double *grad_host, double *hess_host);

/* the trace part of the gradient on its own: grad_host[i] = 1/2 sum_jk (W_jk - b_j b_k) dK_jk/dtheta_i over the
 * n x n symmetric W (lower triangle read; b with stride ldb, or NULL for the pure trace 1/2 tr(W dK_i)).  The row-sharded
 * gradient calls it on each rank's partial Gram matrix inv(L)_p^T inv(L)_p (gp_marginal_likelihood.py:262-300).
 * W: 16-byte aligned, ldw even and >= padded_dim(n) (-9 otherwise, before anything is launched): the pass loads whole
 * 128-column tile rows, so every row of W owns the columns up to the end of its last tile (their values are never used).
 * partial: device scratch of T(T+1)/2 * ntheta doubles, T = ceil(n/128).  Synchronises. */
int fvgp_hip_grad_trace(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                        const double *theta_host, int ntheta, const double *W, int64_t ldw,
                        const double *b_or_null, int64_t ldb, double *partial, double *grad_host);
/* the same pass over a SLAB of columns [col0, col0 + ncols) of the symmetric matrix (col0 % 128 == 0): W (n, ldw) holds those
 * columns only, entries with row >= column are read.  The row-sharded gradient walks its partial Gram matrix of inv(L) slab by
 * slab, so that no rank ever holds an N x N buffer; the slabs' results add up to fvgp_hip_grad_trace's.
 * W: 16-byte aligned, ldw even and >= 128 * ceil(ncols/128) (-9 otherwise, before anything is launched), for the same reason.
 * partial: ceil(n/128) * ceil(ncols/128) * ntheta doubles (device scratch). */
int fvgp_hip_grad_trace_cols(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                             const double *theta_host, int ntheta, const double *W, int64_t ldw, int64_t col0, int64_t ncols,
                             const double *b, int64_t ldb, double *partial, double *grad_host);

/* posterior: GPposterior.posterior_mean / posterior_covariance  gp_posterior.py:139-182,229-288
 *   L: factor (padded), alpha: KVinvY (padded_dim(n), ncol)
 *   kx: scratch of padded_dim(n) x ldk doubles with ldk >= padded_dim(P).  On return (P >= 2, var_out or S_out given) its first
 *       padded_dim(P) x padded_dim(n) doubles hold V^T = (L^-1 k)^T, row-major with leading dimension padded_dim(n): a caller that
 *       walks many prediction points in chunks builds the off-diagonal blocks S_ij = k(x_i, x_j) - V_i^T V_j from the chunks'
 *       scratches (fvgp_amd/gp.py _posterior_chunked; gp_posterior.py:120-136).  One point: unspecified.  The first call after a new factor
 *       also inverts its diagonal blocks into the handle (2048 x 2048 up to 1024 points, option "posterior_block"; 1024 x 1024
 *       beyond; fvgp_hip_workspace_bytes counts them).  The block width depends on P and the option only: the same call returns
 *       the same bits whether it is the first on a factor or a later one
 *   mean_out (P, ncol) device  = k^T alpha          (prior mean added by the caller)
 *   S_out (padded_dim(P), lds) device or NULL  = kk - k^T KV^-1 k  (full, symmetric)
 *   var_out (P) device  = diag of the above (unclipped; clipping is gp_posterior.py:248-259, caller side) */
/* Enqueue what the first fvgp_hip_posterior on a new factor would otherwise do in front of its sweep (the inverted diagonal blocks,
 * 2.6 ms at N = 20k) -- GPkv._refresh computes what the posterior queries need when the state changes, not at the first query
 * (gp_kv.py:404-428).  Asynchronous; a no-op where the sweep does not use inverted blocks. */
int fvgp_hip_posterior_prepare(fvgp_handle *h, const double *L, int64_t n, int64_t ldl);
int fvgp_hip_posterior(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                       const double *theta_host, int ntheta, const double *L, int64_t ldl,
                       const double *alpha, int ncol, const double *xpred, int64_t P,
                       double *kx, int64_t ldk, double *mean_out, double *var_out, double *S_out, int64_t lds);

/* posterior_grad: the posterior mean and variance at P points TOGETHER WITH their exact gradients in the prediction points, for the
 * optimiser of an acquisition function.  The reference takes these derivatives by a forward difference of the kernel with step 1e-8
 * (gp_posterior.py:184-226, 290-331; gp_prior.py:402-409); for the stationary kernels here dk(x*, x_i)/dx*_k = -cf(r^2) (x*_k - x_ik) / l_k^2
 * in closed form, so with alpha = KVinvY[:, component] and W = KV^-1 k(x, x*) one pass over W gives (csrc/posterior_grad.hip)
 *     A_out[p] = sum_i k_ip alpha_i                          (prior mean added by the caller, as fvgp_hip_posterior)
 *     q_out[p] = sum_i k_ip W_ip                             (the caller forms k(x*, x*) - q)
 *     dm_out[p][k] = sum_i dk_ip/dx*_k alpha_i               (P, n_dirs)
 *     dv_out[p][k] = -2 sum_i dk_ip/dx*_k W_ip               (P, n_dirs): the derivative of the unclipped latent variance
 *   alpha     (padded_dim(n), ncol) device, column `component` is read
 *   W         (padded_dim(n), ldw) device with ldw >= padded_dim(P): the first n rows of KV^-1 k(x, x*), prediction points contiguous
 *             (what fvgp_hip_kmat with zero padding followed by fvgp_hip_potrs / fvgp_hip_potrs_cols leaves), or NULL: A_out and
 *             dm_out only (q_out, dv_out may be NULL then)
 *   n_dirs    1 .. d: the LEADING input columns to differentiate (a multi-task index set differentiates its spatial columns, not the
 *             task column)
 *   work      caller-owned device scratch of at least fvgp_hip_posterior_grad_workspace_bytes(n, P, n_dirs) bytes (the partial sums of
 *             the slices of 256 data rows); work_bytes its size
 * The data rows are split over workgroups by n alone and the partial sums added in a fixed order without atomics: a point's four
 * results have the same bits whatever P is, whichever other points are in the call and wherever a caller cuts a list of points into
 * calls.  Asynchronous on the handle's stream.  Errors (argument numbers): -3 x, -4 n, -6 theta, -8 xpred, -9 P, -10 alpha, -11 ncol,
 * -12 component, -14 ldw, -15 n_dirs, -16 work, -17 work_bytes, -18 .. -21 an output that is needed is NULL; kernel id, d and ntheta
 * as fvgp_hip_kmat. */
int fvgp_hip_posterior_grad(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                            const double *theta_host, int ntheta, const double *xpred, int64_t P,
                            const double *alpha, int ncol, int component, const double *W, int64_t ldw, int n_dirs,
                            double *work, int64_t work_bytes, double *A_out, double *q_out, double *dm_out, double *dv_out);
/* bytes of the caller-owned scratch of fvgp_hip_posterior_grad; -1 for invalid arguments */
int64_t fvgp_hip_posterior_grad_workspace_bytes(int64_t n, int64_t P, int n_dirs);
/* fvgp_hip_potrs for nrhs % 128 == 0 columns with every product on the 128-tile kernel, whatever nrhs is: fvgp_hip_potrs sends products
 * of few tiles to the 64-tile kernel, which contracts k in another order, so that a column's bits there depend on how many columns
 * travel with it.  Here a column of the solution has the same bits in every call (the results fvgp_hip_posterior_grad builds on). */
int fvgp_hip_potrs_cols(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb);

/* loo: leave-one-out cross-validation in closed form, with the exact gradient of the LOO log predictive probability in the kernel's
 * hyperparameters (csrc/loo.hip; Rasmussen & Williams 5.4.2).  With Q = KV^-1, q_i = Q_ii and alpha = Q (y - m)[:, component]:
 *     resid_out[i] = y_i - mu_i = alpha_i / q_i        var_out[i] = sigma^2_i = 1 / q_i   (of the NOISY observation)
 *     L_LOO = sum_i (log q_i - alpha_i^2 / q_i) / 2 - n / 2 log 2 pi                      (sum_i log p(y_i | y_-i))
 * and with w = alpha / q, c_i = (1 + alpha_i^2 / q_i) / (2 q_i), u = Q w, M = Q diag(c) Q:
 *     grad_host[j] = dL_LOO/dtheta_j = sum_kl ((u_k alpha_l + alpha_k u_l) / 2 - M_kl) dK_kl/dtheta_j
 * -- one symmetric N^3 product for all hyperparameters and one pass of the fused trace kernel; the derivative of the quantity to be
 * MAXIMISED, 0 for hyperparameters the kernel does not own.  A caller adds the terms of a diagonal noise derivative dV,
 * sum_k dV_k (u_k alpha_k - M_kk), and of a mean derivative, u^T dm, from u_out and mdiag_out.
 *   KV        the factor L as fvgp_hip_loglik / fvgp_hip_potrf leave it (padded); destroyed
 *   work      a second padded square; destroyed
 *   alpha     (padded_dim(n), ncol) device, column `component` is read
 *   ws        caller-owned device scratch of at least fvgp_hip_loo_workspace_bytes(n) bytes (vectors only), ws_bytes its size
 *   out_host  4 doubles: L_LOO, sum resid^2, sum log q_i, the number of q_i that are not positive and finite (non-zero: the first
 *             three, and the gradient, are NaN)
 *   resid_out, var_out   device n-vectors
 *   grad_host NULL: values only -- the call is POTRI and one pass over the diagonal, KV holds exactly what fvgp_hip_potri leaves, and
 *             kernel_id, x, d, theta are not read (the path of kernel callables).  Else ntheta doubles, and
 *   u_out, mdiag_out     device n-vectors u and diag(M), required with grad_host
 * One host synchronisation per call; no atomics: the same inputs give the same bits on every run.  Flops: 2/3 n^3 (POTRI) + n^3.
 * Errors (argument numbers, nothing is launched): -3 x, -4 n, -6 theta, -8 alpha, -9 ncol, -10 component, -11 / -12 KV / ld,
 * -13 / -14 work / ldw, -15 ws, -16 ws_bytes, -17 .. -19 out_host, resid_out, var_out, -21 u_out, -22 mdiag_out; kernel id, d and
 * ntheta as fvgp_hip_kmat. */
int fvgp_hip_loo(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                 const double *theta_host, int ntheta, const double *alpha, int ncol, int component,
                 double *KV, int64_t ld, double *work, int64_t ldw, double *ws, int64_t ws_bytes,
                 double *out_host, double *resid_out, double *var_out,
                 double *grad_host, double *u_out, double *mdiag_out);
/* bytes of the caller-owned scratch of fvgp_hip_loo: (3 padded_dim(n) + 4 padded_dim(n) / 128) doubles; -1 for n < 1 */
int64_t fvgp_hip_loo_workspace_bytes(int64_t n);

/* ---- sampling ------------------------------------------------------------------------------
 * Joint draws f ~ N(mean, L L^T) for Thompson sampling and Monte-Carlo acquisition functions (csrc/sample.hip).  The reference has no
 * counterpart: its users take numpy.linalg.cholesky of the posterior_covariance result (gp_posterior.py:229-288) on the host.
 *
 * The generator is a pure function z(seed, stream, i, j) with no state: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key
 * increments 0x9E3779B9 / 0xBB67AE85) on the counter (i, j, lo32(stream), hi32(stream)) with the key (lo32(seed), hi32(seed)); with its
 * output words w0..w3: u1 = (((w0 | w1 << 32) >> 11) + 0.5) 2^-53, u2 the same from w2, w3, z = sqrt(-2 ln u1) cos(2 pi u2).  i is the
 * point (row) index and j the sample index, both below 2^32.  One counter per element: z(seed, stream, i, j) never depends on its
 * neighbours, on the launch shape or on how a caller cuts a request into calls (tests/samples_ref.py is the numpy twin).
 *
 * normal_fill: Z[r][c] = z(seed, stream, row0 + r, col0 + c); rows x cols doubles at leading dimension ldz; nothing outside that block
 * is written; asynchronous.  Errors (argument numbers, nothing is launched): -6 Z NULL, -7 rows < 1, -8 cols < 1, -9 ldz < cols,
 * -4 / -5 row0 + rows / col0 + cols past 2^32 (or a negative offset). */
int fvgp_hip_normal_fill(fvgp_handle *h, uint64_t seed, uint64_t stream, int64_t row0, int64_t col0,
                         double *Z, int64_t rows, int64_t cols, int64_t ldz);
/* Y[s][p] = mean[p] + sum_{q <= p} L[p][q] * z(seed, stream, q, samp0 + s),  s < nsamp, p < n.
 * L: factor as fvgp_hip_potrf leaves it (padded); its strict upper triangle is never read, and what its padding holds does not reach Y.
 * Y (nsamp, ldy >= n) row-major device; mean (n) device or NULL; Z_out NULL or (n, ldz >= nsamp): the normals used.
 * work: caller-owned scratch of fvgp_hip_mvn_sample_workspace_bytes(n, nsamp) bytes, 16-byte aligned.  Asynchronous.
 * The product runs on the 128-tile GEMM kernel in its explicit-K-range form (whatever the shape, never the 64-tile kernel, never a
 * split K): the diagonal 128-tiles of L, copied into `work` with their upper halves zeroed, times their block rows of Z, then the
 * tiles below the diagonal with the K range of a tile row ending at its diagonal tile.  An entry of Y is a sum over its row of L and
 * its column of Z in an order the row alone fixes, so A SAMPLE'S BITS DO NOT DEPEND ON nsamp, ON samp0 OR ON WHAT ELSE IS IN THE
 * CALL: sample samp0 + s is the same whether it is drawn alone, as part of a longer call or in a call that starts elsewhere.
 * Errors (argument numbers, nothing is launched): -2 .. -4 L, n, ldl as fvgp_hip_potrf (ldl below 2^21), -8 samp0 (samp0 + nsamp
 * past 2^32), -9 nsamp (< 1, or padded_dim(nsamp) not below 2^21: draw more in several calls), -10 / -11 Y / ldy, -13 ldz,
 * -14 / -15 work / work_bytes. */
int fvgp_hip_mvn_sample(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, const double *mean,
                        uint64_t seed, uint64_t stream, int64_t samp0, int64_t nsamp,
                        double *Y, int64_t ldy, double *Z_out, int64_t ldz, double *work, int64_t work_bytes);
/* Greedy batch selection (csrc/select.hip): which q of P candidate positions to measure next -- the pivoted Cholesky of the
 * candidates' posterior covariance, column by column from the factor L of K + V, without the P x P matrix.  d = var (P) holds the
 * conditional latent variances (in: the posterior variances, e.g. var_out of fvgp_hip_posterior; entries below 0 are taken as 0),
 * s = noise (P) the candidates' noise variances (NULL = 0).  Step t = 0 .. q-1:
 *     score_i = d_i (criterion 0) or d_i / s_i (criterion 1: monotone in the information gain 1/2 log(1 + d_i / s_i); the CALLER
 *         guarantees every s_i > 0 -- the values live on the device and are not checked: with an s_i <= 0 the picks are undefined);
 *         candidates already picked do not score unless allow_repeats != 0; j = the largest score, ties to the lowest index;
 *     if d_j <= tol * max_i d_i(in), or nothing scores: idx_out[t..q-1] = -1, pick_var_out[t..q-1] = 0, and the call ends there
 *         (decided on the device: the remaining steps' kernels return at once; var keeps what step t-1 left);
 *     idx_out[t] = j, pick_var_out[t] = d_j, p = d_j + s_j;
 *     r_i = k(x_i, x_j) - sum_n k(x_i, X_n) w_n with w = (K + V)^-1 k(X, x_j)      (column j of the posterior covariance)
 *     c_i = (r_i - sum_{s<t} G[s][i] G[s][j]) / sqrt(p);   G[t][i] = c_i;   d_i <- max(d_i - c_i^2, 0)
 * so that on return var is the latent variance every candidate would have after the picked points are measured with their noise, and
 * G (rows up to the last pick) is the pivoted factor: sum_t G[t][i] G[t][k] is the covariance the measurements remove.  Nothing depends
 * on y.  Every sum has a fixed order and the split of the data rows is a function of n alone: r_i, row t of G at candidate i and d_i have
 * the same bits whatever P is, whichever candidates share the call, and for every "select_block".
 *   x (n, d), xcand (P, d), noise (P) or NULL, var (P): device, row-major;  theta_host: the kernel's hyperparameters (host);
 *   L: the factor (padded_dim(n) rows, ldl) as fvgp_hip_potrf leaves it;  idx_out (q) int64, pick_var_out (q): device;
 *   G_out: NULL, or device (q, ldg) with ldg >= P (rows from the first exhausted step on are not written);
 *   work: device, 16-byte aligned, at least fvgp_hip_select_workspace_bytes(n, P, q) bytes.
 * Asynchronous on the handle's stream: the q steps are enqueued by this one call and nothing is read back; the host waits only if the
 * handle has to allocate its own vector scratch or the block inverses of a factor it has not solved with before (the first call).
 * Returns, before anything is enqueued and with no buffer touched, -1 .. -23 by argument number: -1 h, -2 unknown kernel_id, -3 x,
 * -4 n < 1 (or more than 65535 slices of 256 rows), -5 d outside 1 .. FVGP_MAX_DIM, -6 theta_host, -7 too few hyperparameters,
 * -8 L NULL or not 16-byte aligned, -9 ldl odd or below padded_dim(n), -10 xcand, -11 P < 1, -12 criterion 1 without noise, -13 var,
 * -14 q < 1, -15 criterion not 0 / 1, -17 tol negative or no number, -18 work NULL or misaligned, -19 work_bytes too small,
 * -20 idx_out, -21 pick_var_out, -23 ldg < P with a G_out. */
int fvgp_hip_select_batch(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                          const double *theta_host, int ntheta, const double *L, int64_t ldl,
                          const double *xcand, int64_t P, const double *noise, double *var,
                          int q, int criterion, int allow_repeats, double tol,
                          double *work, int64_t work_bytes, int64_t *idx_out, double *pick_var_out, double *G_out, int64_t ldg);
/* bytes of the caller-owned workspace of fvgp_hip_select_batch: the padded column (padded_dim(n) doubles), the slot and the state words,
 * three doubles per 64 candidates, one byte per candidate, the factor G (q P doubles) and the slices' partial sums, ceil(n / 256) min(P, 65536) doubles whatever
 * P is -- O(P q), never P x P; -1 for n, P or q < 1 */
int64_t fvgp_hip_select_workspace_bytes(int64_t n, int64_t P, int q);
/* bytes of the caller-owned scratch of fvgp_hip_mvn_sample: (2 padded_dim(n) padded_dim(nsamp) + 128 padded_dim(n)) doubles -- the
 * normals, the product and the masked diagonal tiles; -1 for n < 1 or nsamp < 1 */
int64_t fvgp_hip_mvn_sample_workspace_bytes(int64_t n, int64_t nsamp);

/* ---- matrix-free solves (csrc/matrix_free.hip) --------------------------------------
 * (K(theta) + V) X = B without ever storing K: memory O(n (rank + s)).  What gp2Scale reaches with sparse kernels
 * (fvgp/gp2Scale_covariance.py) is reached here for the dense stationary kernels by preconditioned conjugate gradients.
 *
 * fvgp_hip_kmatvec: Y = K(x1, x2; theta) B + diag(vdiag) B.  x1 (n1, d), x2 (n2, d), B (n2, ldb >= s), Y (n1, ldy >= s), vdiag (n1) or
 * NULL (only with n1 == n2): device, row-major, fp64.  Y is written inside its n1 x s view only.  The columns go in groups of 16, 8, 4
 * or 1 (the narrowest that holds what is left); each kernel entry is evaluated once per group.  Asynchronous.
 * BIT CONTRACT: Y[i][c] is a function of (x1_i, x2, B[:, c], theta, vdiag_i) alone -- the same bits whatever n1 is, whichever rows and
 * columns share the call, whatever the grouping and for every "matvec_split".  The order: x2 in chunks of FVGP_MATVEC_CHUNK rows, a
 * chunk in slices of 256; wave w of four sums rows [64 w, 64 w + 64) of every slice of the chunk, even and odd rows apart; the chunk's sum
 * is (((e0 + o0) + (e1 + o1)) + (e2 + o2)) + (e3 + o3); chunk sums are added to 0 in ascending order; vdiag_i B[i][c] enters as the last fused
 * multiply-add.
 * work: device scratch of fvgp_hip_kmatvec_workspace_bytes(n1, n2, s) bytes for the split form (per-chunk sums); NULL or less is fine
 * unless "matvec_split" > 1 forces a split (option 0 then simply does not split).
 * Errors (argument numbers, nothing is launched): -1 h, -2 unknown kernel_id, -3 x1, -4 n1 < 1, -5 x2, -6 n2 < 1, -7 d outside
 * 1 .. FVGP_MAX_DIM, -8 theta_host, -9 too few hyperparameters, -10 vdiag with n1 != n2, -11 B, -12 ldb < s, -13 s < 1, -14 Y,
 * -15 ldy < s, -16 work not 8-byte aligned, -17 work_bytes negative, or too small for a forced split. */
int fvgp_hip_kmatvec(fvgp_handle *h, int kernel_id, const double *x1, int64_t n1, const double *x2, int64_t n2, int d,
                     const double *theta_host, int ntheta, const double *vdiag_or_null, const double *B, int64_t ldb, int s,
                     double *Y, int64_t ldy, double *work, int64_t work_bytes);
/* bytes of the split form's per-chunk sums: ceil(n2 / FVGP_MATVEC_CHUNK) n1 min(group width of s, 16) doubles; -1 for n1, n2 or s < 1 */
int64_t fvgp_hip_kmatvec_workspace_bytes(int64_t n1, int64_t n2, int s);
/* Greedy pivoted Cholesky of K(x, x; theta) (no noise), rank <= q, K never formed.  d = sigma^2 at every point; step t = 0 .. q-1:
 *     j = argmax d over the points not picked yet, ties to the lowest index (step 0 picks point 0);
 *     if d_j <= tol sigma^2 (or nothing is left): piv_out[t .. q-1] = -1 and the call ends there (decided on the device; the remaining
 *         rows of G stay ZERO rows, so G^T G and every shape downstream are unaffected);
 *     c_i = (k(x_i, x_j) - sum_{s<t} G[s][i] G[s][j]) / sqrt(d_j);   G[t][i] = c_i;   d_i <- max(d_i - c_i^2, 0).
 * A point's column of G has the same bits whatever else is in the call as long as the pivots are the same.
 *   x (n, d) device; G (q, ldg >= n) device, written inside its (q, n) view only; piv_out (q) int64 device; resid_diag_out (n) device or
 *   NULL: d after the last step; work: device, 16-byte aligned, fvgp_hip_pchol_workspace_bytes(n, q) bytes; rank_host: the achieved rank.
 * All q steps are enqueued by this one call; the stream is drained once, at the end, for the rank.
 * Errors: -1 h, -2 unknown kernel_id, -3 x, -4 n < 1, -5 d, -6 theta_host, -7 too few hyperparameters, -8 q < 1, -9 tol negative or no
 * number, -10 G, -11 ldg < n, -12 piv_out, -14 work NULL or misaligned, -15 work_bytes too small, -16 rank_host. */
int fvgp_hip_pchol(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta_host, int ntheta,
                   int q, double tol, double *G, int64_t ldg, int64_t *piv_out, double *resid_diag_out,
                   double *work, int64_t work_bytes, int *rank_host);
/* the slot, the state words, two doubles per 64 points, one byte per point and the residual diagonal: O(n); -1 for n or q < 1 */
int64_t fvgp_hip_pchol_workspace_bytes(int64_t n, int q);
/* The preconditioner M = G^T G + D, D = diag(vdiag), through Woodbury: M^-1 = D^-1 - D^-1 G^T C^-1 G D^-1 with C = I + G D^-1 G^T.
 * Forms C (q x q; G is NOT modified) by plain streaming kernels -- partial sums over chunks of 8192 points, every entry's points in
 * ascending order, chunks in ascending order -- into C (padded_dim(q) rows, ldc even and >= padded_dim(q), 16-byte aligned) and factors
 * it in place like fvgp_hip_potrf; *info_host as there (0, or the failing pivot).  work: fvgp_hip_precond_workspace_bytes(n, q) bytes.
 * Errors: -1 h, -2 G, -3 ldg < n, -4 q outside 1 .. FVGP_PCG_MAX_RANK, -5 n < 1, -6 vdiag, -7 C NULL or misaligned, -8 ldc, -9 work,
 * -10 work_bytes too small, -11 info_host. */
int fvgp_hip_precond_factor(fvgp_handle *h, const double *G, int64_t ldg, int q, int64_t n, const double *vdiag,
                            double *C, int64_t ldc, double *work, int64_t work_bytes, int *info_host);
int64_t fvgp_hip_precond_workspace_bytes(int64_t n, int q);      /* ceil(n / 8192) q^2 doubles; -1 for n or q < 1 */
/* Preconditioned conjugate gradients for (K(x, x; theta) + D) X = B, s <= FVGP_PCG_MAX_RHS columns: s independent recurrences that share
 * every product (fvgp_hip_kmatvec).  rho, alpha, beta, |r| and |b| live per column on the device; every dot product is reduced in an
 * order n alone fixes.  A column FREEZES (no vector kernel writes it again) once its recurrence residual is <= tol |b|, after max_iter
 * iterations of its own, or on breakdown (p^T A p or r^T z not positive or not finite).  The host reads the status words every
 * check_every iterations.  When every column is frozen one more product gives the TRUE residual b - A x: a column above tol that met
 * its recurrence test restarts from the true residual, at most max_restarts times.
 *   G (q, ldg) and C (factor of fvgp_hip_precond_factor): the preconditioner; q == 0 or G == NULL: Jacobi, D^-1.  M^-1 is applied as
 *   two streaming products with G and one potrs per column on C.
 *   warm != 0: X holds the initial guess (one more product); else the start is x = 0.  A zero column of B returns x = 0, 0 iterations.
 *   iters_host, relres_host (true relative residual), status_host (0 converged, 1 not converged: iteration or restart limit,
 *   2 breakdown): s entries each.  Returns 0 whenever the call ran: non-convergence is data.  Synchronous.
 * BIT CONTRACT: column c of X, its iters and its relres have the same bits whatever other columns share the call, and the same call
 * returns the same bits every run.
 *   work: device, 16-byte aligned, fvgp_hip_pcg_workspace_bytes(n, q) bytes.
 * Errors: -1 h, -2 unknown kernel_id, -3 x, -4 n < 1, -5 d, -6 theta_host, -7 too few hyperparameters, -8 vdiag, -10 ldg < n,
 * -11 q outside 0 .. FVGP_PCG_MAX_RANK, -12 C NULL or misaligned with q > 0, -13 ldc, -14 B, -15 ldb < s, -16 s outside
 * 1 .. FVGP_PCG_MAX_RHS, -17 X, -18 ldx < s, -20 tol not positive, -21 max_iter < 1, -22 check_every < 1, -23 max_restarts < 0,
 * -24 work NULL or misaligned, -25 work_bytes too small, -26 iters_host, -27 relres_host, -28 status_host. */
int fvgp_hip_pcg(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta_host, int ntheta,
                 const double *vdiag, const double *G_or_null, int64_t ldg, int q, const double *C, int64_t ldc,
                 const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
                 double tol, int max_iter, int check_every, int max_restarts,
                 double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host);
/* four (n, 16) vectors, the rank's partial sums (ceil(n / 4096) q 16 doubles), the dot products' partials and, while the product would
 * split by itself, its per-chunk sums; -1 for n < 1 or q < 0 */
int64_t fvgp_hip_pcg_workspace_bytes(int64_t n, int q);

/* ---- the stochastic log-likelihood on the matrix-free path (csrc/matrix_free.hip) --------------------------
 * log det(K + D) by preconditioned stochastic Lanczos quadrature and tr((K + D)^-1 dK/dtheta_j) by Hutchinson probes drawn from the
 * preconditioner M = G^T G + D: probes (precond_probes), M^-1 outside the solver (precond_apply), the solver with its coefficients
 * recorded (pcg_lanczos), and the bilinear form u^T (dK/dtheta_j) w without dK (kgrad_form).
 *
 * fvgp_hip_kgrad_form: out_host[j] = sum_{c < s} U[:, c]^T (dK(x1, x2; theta) / dtheta_j) W[:, c], j < the kernel's own hyperparameter count
 * (sigma^2 first, then one length scale or d of them).  x1 (n1, d), U (n1, ldu >= s), x2 (n2, d), W (n2, ldw >= s), 1 <= s <=
 * FVGP_PCG_MAX_RHS: device, row-major, fp64.  Noise never enters.  One pass over the n1 x n2 kernel entries per column group: per entry
 * one exp (and one rsq for the Matern kinds), t = sum_c U[i][c] W[k][c], and one fused multiply-add per hyperparameter.  Synchronous.
 * BIT CONTRACT: the result is a function of the arguments' VALUES alone -- the same bits on every run, for every "matvec_split" and
 * whatever `work` held before.  The order: the columns go in groups of 16, 8, 4 or 1 as in fvgp_hip_kmatvec, t is a chain of fused
 * multiply-adds over the group's columns in ascending order starting from 0 (so a zero column changes nothing); per row i of x1 the rows of
 * x2 are summed exactly as fvgp_hip_kmatvec sums them (chunks of FVGP_MATVEC_CHUNK, slices of 256, four waves, even and odd rows apart,
 * chunk sums added to 0 in ascending order); the length-scale sums are multiplied by 1 / l once per row; the 64 rows of a block are added
 * by a halving tree (lane i += lane i + 32, 16, .. 1), the blocks to 0 in ascending order, and the groups in ascending order.  The split
 * into column groups is part of the value: s columns in one call and the same columns in several calls added on the host differ in the
 * last bits.
 * work: device, 8-byte aligned, fvgp_hip_kgrad_form_workspace_bytes(n1, n2) bytes at least.
 * Errors (argument numbers, nothing is launched): -1 h, -2 unknown kernel_id, -3 x1, -4 n1 < 1, -5 x2, -6 n2 < 1, -7 d outside
 * 1 .. FVGP_MAX_DIM, -8 theta_host, -9 too few hyperparameters, -10 U, -11 ldu < s, -12 W, -13 ldw < s, -14 s outside
 * 1 .. FVGP_PCG_MAX_RHS, -15 work NULL or misaligned, -16 work_bytes too small, -17 out_host. */
int fvgp_hip_kgrad_form(fvgp_handle *h, int kernel_id, const double *x1, int64_t n1, const double *x2, int64_t n2, int d,
                        const double *theta_host, int ntheta, const double *U, int64_t ldu, const double *W, int64_t ldw, int s,
                        double *work, int64_t work_bytes, double *out_host);
/* (1 + ceil(n1 / 64)) (1 + FVGP_MAX_DIM) doubles for the result and the blocks' sums, and, while the product would deal chunk ranges
 * over workgroups by itself (fewer than 512 blocks of 64 rows and at least two chunks), ceil(n2 / FVGP_MATVEC_CHUNK) n1 (1 + FVGP_MAX_DIM)
 * more for the parked chunk sums; with less than that second part the chunks are walked by one workgroup per 64 rows (the same bits);
 * -1 for n1 or n2 < 1 */
int64_t fvgp_hip_kgrad_form_workspace_bytes(int64_t n1, int64_t n2);
/* Probes with covariance M = G^T G + D: Z[i][c] = sqrt(v_i) z(seed, 2 stream, i, col0 + c) + sum_t G[t][i] z(seed, 2 stream + 1, t, col0 + c),
 * z the function of fvgp_hip_normal_fill; the first product first, then fused multiply-adds over t in ascending order.  G (q, ldg >= n)
 * or NULL / q == 0 (then Z = D^1/2 z), vdiag (n), Z (n, ldz >= s), 1 <= s <= FVGP_PCG_MAX_RHS: device.  Z is written inside its n x s
 * view only.  Column c is a function of (seed, stream, col0 + c, G, v) alone: a longer call extends a shorter one bit for bit, and col0
 * shifts columns.  Asynchronous.
 * Errors: -1 h, -3 stream (2 stream + 1 must fit 64 bits), -4 col0 negative or col0 + s past 2^32, -6 ldg < n with q > 0, -7 q outside
 * 0 .. FVGP_PCG_MAX_RANK, -8 n < 1 or past 2^32, -9 vdiag, -10 Z, -11 ldz < s, -12 s outside 1 .. FVGP_PCG_MAX_RHS. */
int fvgp_hip_precond_probes(fvgp_handle *h, uint64_t seed, uint64_t stream, int64_t col0, const double *G_or_null, int64_t ldg, int q,
                            int64_t n, const double *vdiag, double *Z, int64_t ldz, int s);
/* W = M^-1 R for an (n, s <= FVGP_PCG_MAX_RHS) block, M = G^T G + D with the factor C of fvgp_hip_precond_factor (q == 0 or G NULL:
 * W = D^-1 R): the launches fvgp_hip_pcg applies its preconditioner with, so a column of W has the bits the solver's first z has for the
 * same right-hand side, whatever else is in the call.  R (n, ldr >= s), W (n, ldw >= s): device; W is written inside its n x s view only
 * and may be R.  work: device, 16-byte aligned, fvgp_hip_precond_apply_workspace_bytes(n, q) bytes.  Asynchronous (the host waits only
 * where fvgp_hip_potrs would).
 * Errors: -1 h, -3 ldg < n with q > 0, -4 q outside 0 .. FVGP_PCG_MAX_RANK, -5 C NULL or misaligned with q > 0, -6 ldc, -7 n < 1,
 * -8 vdiag, -9 R, -10 ldr < s, -11 s outside 1 .. FVGP_PCG_MAX_RHS, -12 W, -13 ldw < s, -14 work NULL or misaligned, -15 work_bytes too
 * small. */
int fvgp_hip_precond_apply(fvgp_handle *h, const double *G_or_null, int64_t ldg, int q, const double *C, int64_t ldc, int64_t n,
                           const double *vdiag, const double *R, int64_t ldr, int s, double *W, int64_t ldw,
                           double *work, int64_t work_bytes);
/* two (n, 16) vectors, the rank's partial sums and the padded (q, 16) block; -1 for n < 1 or q < 0 */
int64_t fvgp_hip_precond_apply_workspace_bytes(int64_t n, int q);
/* fvgp_hip_pcg that also records the coefficients of every column's FIRST recurrence (before any restart), the Lanczos tridiagonal of
 * M^-1/2 (K + D) M^-1/2 started from M^-1/2 b:  T[k][k] = 1 / alpha_k + beta_{k-1} / alpha_{k-1} (the second term absent at k = 0),
 * T[k][k+1] = sqrt(beta_k) / alpha_k.  One driver serves both entries: X, iters_host, relres_host and status_host have the bits of
 * fvgp_hip_pcg for every lanczos_steps, and the solve goes on to its tolerance whatever is recorded.
 *   lanczos_steps = L in 0 .. FVGP_LANCZOS_MAX_STEPS;  alpha_host, beta_host (s, L) row-major, steps_host (s), rho0_host (s): host.
 *   rho0_host[c] = r_0^T M^-1 r_0 (b^T M^-1 b for a cold start; 0 for a column that never started);  alpha_host[c][k], k < steps_host[c] =
 *   min(L, iterations of the first recurrence);  beta_host[c][k] for every k < L the recurrence went on after (at least steps_host[c] - 1 of
 *   them); entries not recorded are 0.  With L == 0 nothing is recorded and the four pointers may be NULL.
 * A column's records do not depend on what else is in the call.  work: fvgp_hip_pcg_lanczos_workspace_bytes(n, q, L) bytes.
 * Errors: those of fvgp_hip_pcg (-25 against this entry's workspace size), -29 lanczos_steps outside 0 .. FVGP_LANCZOS_MAX_STEPS, and
 * with L > 0: -30 alpha_host, -31 beta_host, -32 steps_host, -33 rho0_host. */
int fvgp_hip_pcg_lanczos(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta_host, int ntheta,
                         const double *vdiag, const double *G_or_null, int64_t ldg, int q, const double *C, int64_t ldc,
                         const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
                         double tol, int max_iter, int check_every, int max_restarts,
                         double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host,
                         int lanczos_steps, double *alpha_host, double *beta_host, int *steps_host, double *rho0_host);
/* the solver's workspace and, behind it, 16 (2 L + 3) doubles of records; -1 for n < 1, q < 0 or L outside 0 .. FVGP_LANCZOS_MAX_STEPS */
int64_t fvgp_hip_pcg_lanczos_workspace_bytes(int64_t n, int q, int lanczos_steps);

/* ---- rank-k update of a resident factor, removal of data points (csrc/chol_update.hip) ---------------
 * The other half of the bordering append (gp_lin_alg.py:1310-1477 only ever grows a factor): with S the kept and R the removed indices
 * of a factor L of K+V,  KV[S,S] = L[S,S] L[S,S]^T + L[S,R] L[S,R]^T,  so the factor of the kept points is a POSITIVE rank-|R| update
 * of the compacted triangle -- orthogonal transforms only, no kernel evaluation, nothing that can lose positive definiteness.
 *
 * fvgp_hip_chol_update: L <- chol(L L^T + W W^T) in place.  L: the factor (padded_dim(n) rows, ldl) as fvgp_hip_potrf leaves it;
 *   W: device (n, ldw >= k) row-major, DESTROYED.  Rows < row0 of W are promised to be zero (0 <= row0 <= n): block columns left of
 *   row0 are not touched.  The strict upper triangle of L is never read or written, the padding rows are left as they were.  k above
 *   FVGP_CHOL_UPDATE_MAX_RANK runs as successive passes of at most that many columns of W, each an exact update.  Per pass and
 *   128-column block: one workgroup rotates the diagonal block and writes the block's Givens coefficients, then one launch applies them
 *   to every row below, each element of L read once and written once.  Plain stream-ordered launches, no atomics.
 *   BIT INVARIANT: the same call returns the same bits, and row i of the result depends only on rows <= i of L and W -- the leading m
 *   rows of an update of n rows equal, bit for bit, the update of the leading m x m problem alone (whatever ldl is).
 *   ws: device, 16-byte aligned; the update itself uses its first FVGP_CHOL_UPDATE_TABLE_BYTES only.  Asynchronous on the handle's stream.
 *   Returns, before anything is launched, minus the position of a bad argument: -1 h, -2 L NULL or misaligned, -3 n < 1, -4 ldl odd or
 *   below padded_dim(n), -5 W, -6 k < 1, -7 ldw < k, -8 row0 outside 0 .. n, -9 ws NULL or misaligned, -10 ws_bytes too small.
 * fvgp_hip_chol_delete: the factor of the n - k points that remain when the points idx_host[0 .. k) (HOST, strictly increasing, every
 *   index in [0, n), 1 <= k < n) leave: W = L[S,R] is gathered, L[S,S] moved up-left inside the same buffer (through a strip of at most
 *   1024 rows in ws, strip after strip in stream order: there is no second n x n buffer), rows n - k .. padded_dim(n) - 1 become
 *   identity padding again, and the update runs -- one enqueue.  On return the buffer holds the factor of the kept points, in their
 *   original order, exactly as fvgp_hip_potrf leaves a factor of n - k points.  Removing only trailing points costs no update at all.
 *   THE CALLER MUST INVALIDATE THE HANDLE'S CACHED DIAGONAL-BLOCK INVERSES (fvgp_hip_invalidate_factor) after either call and before
 *   the next potrs / trsm / potri / posterior on that buffer: the factor changed under the same (pointer, n, ld) key or a stale one.
 *   Returns -1 h, -2 .. -4 as above, -5 idx_host NULL, not strictly increasing or out of range, -6 k outside 1 .. n - 1, -7 ws NULL or
 *   misaligned, -8 ws_bytes below fvgp_hip_chol_update_workspace_bytes(n, k); nothing is written then.
 * fvgp_hip_chol_update_workspace_bytes(n, k): what both calls accept -- the coefficient table, the index lists (n + k words), W
 *   (n k doubles) and the strip (min(1024, n, 2^25 / n) rows of n doubles): O(n (k + 1024)), never n x n;  -1 for n < 1 or k < 1. */
#define FVGP_CHOL_UPDATE_MAX_RANK 16
#define FVGP_CHOL_UPDATE_TABLE_BYTES (128 * FVGP_CHOL_UPDATE_MAX_RANK * 2 * 8)
int fvgp_hip_chol_update(fvgp_handle *h, double *L, int64_t n, int64_t ldl, double *W, int64_t k, int64_t ldw, int64_t row0,
                         double *ws, int64_t ws_bytes);
int fvgp_hip_chol_delete(fvgp_handle *h, double *L, int64_t n, int64_t ldl, const int64_t *idx_host, int64_t k, double *ws, int64_t ws_bytes);
int64_t fvgp_hip_chol_update_workspace_bytes(int64_t n, int64_t k);

/* ---- building blocks exported for the parity tests --------------------------------------
 * C (M,N) = alpha * opA * opB + beta * C on fp64 MFMA.  M, N multiples of 128, K of 16.
 *   a_kmajor == 0: A stored (M,K) row-major;  != 0: A stored (K,M) row-major (A^T product)
 *   b_nmajor == 0: B stored (N,K) row-major (C = A B^T); != 0: B stored (K,N) row-major
 *   lower != 0: only 128x128 tiles with row-tile >= col-tile are computed (SYRK-style); every non-zero value means the same, and the
 *     tiles above the diagonal keep their bits
 *   K == 0 is valid (A and B are not read): every computed tile becomes beta * C, and with beta == 0 it becomes zero without C being read
 * Returns -5 for M, N not multiples of 128 or K not a multiple of 16, -9 for A or B not 16-byte aligned or a leading dimension of
 * theirs that is odd or not below 2^21, -9 / -11 / -14 for a NULL A / B / C; nothing is launched and C is untouched then.
 * With fewer than 256 output tiles and K >= 1024 the K range is split over workgroups and the partial tiles added in a fixed
 * order (handle scratch, at most 64 MB): same result on every run, another rounding than the unsplit product.  The split needs
 * C 16-byte aligned with an even ldc; a C that is not takes the unsplit product (state it if rounding must not depend on where a
 * buffer lies: pass aligned buffers). */
int fvgp_hip_gemm(fvgp_handle *h, int a_kmajor, int b_nmajor, int lower, int64_t M, int64_t N, int64_t K,
                  double alpha, const double *A, int64_t lda, const double *B, int64_t ldb,
                  double beta, double *C, int64_t ldc);
/* one 64-lane wave: D = A(16x4) * B(4x16) with the lane maps the kernels assume */
int fvgp_hip_mfma_selftest(fvgp_handle *h, const double *A16x4, const double *B4x16, double *D16x16);
/* host-only replay of the GEMM kernel's blockIdx -> (tile row, tile col) map, XCD remap included
 * (no GPU needed); returns the grid size, fills min(grid, cap) entries; out-of-range tiles are
 * the ones the kernel exits on. */
int64_t fvgp_hip_debug_tile_map(int tiles_m, int tiles_n, int lower, int scale, int off, int *out_ti, int *out_tj, int64_t cap);
/* host-only: the XCD-balanced block -> tile table the plain launches of the 128-tile kernels use instead of the formula map (block b runs
 * on XCD b % 8; each XCD gets a contiguous, equally long run of the REAL tiles in super-tile order).  Entries are
 * (tile row << 16) | tile col, or -1; returns the grid size, fills min(grid, cap) entries. */
int64_t fvgp_hip_debug_tile_table(int tiles_m, int tiles_n, int lower, int scale, int off, int *out, int64_t cap);
/* host-only: the task a start-order ticket gets in the resident panel kernel (csrc/chain.hip) for a panel of n block columns whose first
 * n2 >= n block rows have a workgroup per 128 x 128 block: out3 = {kind, block row, block column}, kind 0 = diagonal block (updates it,
 * then its leaf), 1 = block below the diagonal (products, then the solve behind the leaf), 2 = a whole block row (column = -1).
 * Per block column the diagonal block and the two blocks under it are CRITICAL (the chain of leaves runs through them), the rest BULK;
 * the critical tasks of column k + ahead are dealt right before the bulk tasks of column k ("chain_ahead").  tests/test_host_logic.py
 * replays the order: a bulk task only ever waits for LOWER tickets (ahead = 0: every task does), and the order makes progress with as
 * few as 16 slots. */
int fvgp_hip_debug_chain_ticket(int n, int n2, int ahead, int ticket, int *out3);
/* diagnostic: blocks x 256 threads each issue iters x 16 register-only fp64 MFMAs (2048 flop each per wave);
 * out needs blocks*256 doubles.  Gives the sustained fp64 MFMA ceiling of the device. */
int fvgp_hip_mfma_peak(fvgp_handle *h, double *out, int blocks, int iters);
/* A[i][j] += alpha * B[i][j] for j <= i < n: GPkv.addKV with a matrix-valued (2-d) noise model, KV = K + V
 * (gp_kv.py:654-657); only the lower triangle, like every other symmetric buffer of this ABI */
int fvgp_hip_add_lower(fvgp_handle *h, double *A, int64_t n, int64_t lda, const double *B, int64_t ldb, double alpha);
/* out = sum_{i,j<n} (W[i][j] - b_i b_j) D[i][j]  =  tr(W D) - b^T D b for symmetric W: the kernel term of the gradient,
 * dL/dtheta_i = -1/2 (b^T dK_i b - tr(KV^-1 dK_i)) (gp_marginal_likelihood.py:301-306), for a derivative matrix that exists as
 * numbers -- kernel callables (user gradient or the central differences of gp_prior.py:438-447) and matrix-valued noise
 * derivatives (gp_marginal_likelihood.py:262-267).  W, D full n x n device arrays (W symmetric: both triangles valid), b a
 * device vector with stride ldb or NULL.  Fixed-order reduction. */
int fvgp_hip_trace_dot(fvgp_handle *h, const double *W, int64_t ldw, const double *D, int64_t ldd, const double *b, int64_t ldb,
                       int64_t n, double *out_host);
/* out_host = sum_{i<n, k<c} a[i][k] b[i][k]: the data-fit term sum((y-m) o KVinvY) (gp_marginal_likelihood.py:175) */
int fvgp_hip_dot(fvgp_handle *h, const double *a, int64_t lda, const double *b, int64_t ldb, int64_t n, int c, double *out_host);
/* out[p] = sum_i A[i][p] B[i][p], p < cols (device): einsum('ij,jk,ki->i', k^T, KVinv, k) of the CholInv variance path
 * (gp_posterior.py:238-244) after KVinv k came from fvgp_hip_gemm */
int fvgp_hip_coldot(fvgp_handle *h, const double *A, int64_t lda, const double *B, int64_t ldb, int64_t rows, int64_t cols, double *out);
/* out[p] = sum_i V[i][p]^2, p < ncols: the column sums of squares of a rank's rows of inv(L) are its share of diag(KV^-1)
 * (gradients of noise-function hyperparameters, gp_marginal_likelihood.py:262-267, in the row-sharded mode) */
int fvgp_hip_colsumsq(fvgp_handle *h, const double *V, int64_t rows, int64_t ldv, int64_t ncols, double *out);
/* A[i][j] += alpha * B[i][j], rows x cols: a rank's rows of a matrix-valued noise model added to its rows of K (gp_kv.py:654-657) */
int fvgp_hip_add_matrix(fvgp_handle *h, double *A, int64_t lda, const double *B, int64_t ldb, int64_t rows, int64_t cols, double alpha);
/* mirror the lower triangle into the upper (for exporting K / KV^-1 to numpy) */
int fvgp_hip_symmetrize(fvgp_handle *h, double *A, int64_t n, int64_t lda);

#ifdef __cplusplus
}
#endif
#endif
