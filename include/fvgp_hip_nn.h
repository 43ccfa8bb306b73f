/*
 * fvgp_hip_nn.h -- the nearest-neighbour (Vecchia / NNGP "response") entries of libfvgp_hip.so (csrc/nn.hip, csrc/nn_search.hip).
 *
 * The likelihood of n points as a product of n small conditionals, p(y) ~ prod_i p(y_i | y_c(i)), c(i) the m nearest of the points
 * that come earlier in the ordering; prediction at x* conditions on the m nearest data points.  O(n m^3) time, O(n m) memory, no
 * iteration count and no standard error; with m >= n - 1 it is the exact likelihood.
 *
 * The conventions of fvgp_hip.h hold: fp64, row-major, device pointers unless the parameter says "host", 0 / -k / >= 1000 as return
 * value.  Every call here synchronises the stream except fvgp_hip_nn_search, fvgp_hip_nn_maxmin_order and fvgp_hip_nn_grid_search
 * (fvgp_hip_nn_grid_build synchronises once, in its middle).  No call allocates device memory.
 */
#ifndef FVGP_HIP_NN_H
#define FVGP_HIP_NN_H

#include "fvgp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FVGP_NN_MAX_NEIGHBORS 64   /* most neighbours per row (one lane of a wavefront each) */

/* which call fvgp_hip_nn_workspace_bytes sizes */
#define FVGP_NN_SEARCH 0
#define FVGP_NN_CONDITIONALS 1
#define FVGP_NN_LOGLIK 2

/* Exact brute-force m-nearest neighbours.  xq (nq, d) query rows, xr (nr, d) reference rows, scales_host NULL or d positive numbers:
 * the distance of query i and reference j is  sum_k ((xq[i][k] - xr[j][k]) * (1 / scales[k]))^2  (no scales: 1), the products added by
 * fused multiply-adds in ascending k.  c0 < 0: every reference row is a candidate of every query; c0 >= 0 (causal): the candidates of
 * query i are the reference rows j < min(nr, c0 + i) -- c0 = 0 with xq == xr is the likelihood's structure, c0 = n_old with the appended
 * rows as queries the append, c0 < 0 prediction.
 * idx_out (nq, ld >= m) int32: row i receives its min(m, candidates) nearest candidates sorted by (distance, index) ascending -- ties
 * go to the lower index -- then -1 up to column m; columns m .. ld are not written.
 * BIT CONTRACT: a row is a function of its query, the reference rows, the scales, m and its candidate count alone.
 * Cost O(nq nr d): one wavefront per 64 queries walks every candidate; more than 65536 queries go in several launches.  Asynchronous.
 * Errors: -1 h, -2 xq, -3 nq < 1, -4 xr, -5 nr < 1 or past 2^31 - 1, -6 d outside 1 .. FVGP_MAX_DIM, -7 a scale that is not positive and
 * finite, -8 m outside 1 .. FVGP_NN_MAX_NEIGHBORS, -10 idx_out, -11 ld < m. */
int fvgp_hip_nn_search(fvgp_handle *h, const double *xq, int64_t nq, const double *xr, int64_t nr, int d, const double *scales_host,
                       int m, int64_t c0, int *idx_out, int64_t ld);

/* The conditionals.  For query row i with the neighbour list c = idx[i][0 .. m) (entries outside 0 .. nr - 1, the -1 of the search among
 * them, are skipped wherever in the list they stand, between neighbours too; a list of such entries alone is an empty list, bit for bit;
 * columns m .. ld of idx are never read) and each of the B rows theta_b of thetas_host (B, ntheta):
 *     A = K(x_c, x_c) + diag(v_c),  k = K(x_c, x_i),  A = L L^T,  w = L^-1 k,  z = L^-1 r_c,
 *     mu[b][i] = w^T z,     var[b][i] = (k(x_i, x_i) + s_i) - w^T w
 * r (nr): the caller's centred data on the reference rows, v (nr): their noise, s_or_null (nq): a per-query addend (the row's own noise
 * in the likelihood, nothing or the prediction noise in prediction).  mu, var (B, nq).  A row without neighbours gives mu = 0,
 * var = k(x, x) + s.  Kernel entries are computed by the operations of the covariance assembly.
 * One wavefront per (row, b): the block padded with identity to 16, 32 or 64 rows by m alone, a lane per row, column by column, both
 * substitutions inside the factorisation, w^T z and w^T w by a halving tree over the lanes.
 * BIT CONTRACT: mu[b][i], var[b][i] are functions of (x_i, s_i, the listed rows in their listed order, theta_b, m) alone: not of nq, B,
 * or the position in either.
 * A pivot that is not positive gives mu = var = NaN for that (b, i); nothing traps.  info_host: 0, or 1 + b nq + i of the first
 * (b, i) in that order whose var is not positive (NaN included).
 * work: device, 8-byte aligned, fvgp_hip_nn_workspace_bytes(FVGP_NN_CONDITIONALS, nq, B) bytes.
 * Errors: -1 h, -2 unknown kernel_id, -3 xq, -4 nq < 1, -5 xr, -6 nr < 1 or past 2^31 - 1, -7 d outside 1 .. FVGP_MAX_DIM, -8 thetas_host,
 * -9 too few hyperparameters, -10 B outside 1 .. 65535, -11 idx, -12 ld < m, -13 m outside 1 .. FVGP_NN_MAX_NEIGHBORS, -14 r, -15 v,
 * -17 mu, -18 var, -19 work NULL or misaligned, -20 work_bytes too small, -21 info_host. */
int fvgp_hip_nn_conditionals(fvgp_handle *h, int kernel_id, const double *xq, int64_t nq, const double *xr, int64_t nr, int d,
                             const double *thetas_host, int ntheta, int B, const int *idx, int64_t ld, int m,
                             const double *r, const double *v, const double *s_or_null, double *mu, double *var,
                             double *work, int64_t work_bytes, int64_t *info_host);

/* The likelihood: the conditionals of x (n, d) on itself (idx from fvgp_hip_nn_search with c0 = 0, s = v), then per b
 *     out_host[b] = { log p, fit, logdet },  fit = sum_i (r_i - mu_i)^2 / var_i,  logdet = sum_i log var_i,
 *     log p = -1/2 (fit + logdet + n log 2 pi).
 * mu, var (B, n) keep the per-row conditionals (the approximation's residual diagnostics).
 * The sums run in a fixed order: slices of 256 rows added by a halving tree, the slices to 0 in ascending order.  The same call
 * gives the same bits, and row b's values do not depend on B.  Rows with info (see above) make the sums NaN.
 * work: fvgp_hip_nn_workspace_bytes(FVGP_NN_LOGLIK, n, B) bytes.
 * Errors: -1 h, -2 unknown kernel_id, -3 x, -4 n < 1 or past 2^31 - 1, -5 d outside 1 .. FVGP_MAX_DIM, -6 thetas_host, -7 too few
 * hyperparameters, -8 B outside 1 .. 65535, -9 idx, -10 ld < m, -11 m outside 1 .. FVGP_NN_MAX_NEIGHBORS, -12 r, -13 v, -14 mu, -15 var,
 * -16 work NULL or misaligned, -17 work_bytes too small, -18 out_host, -19 info_host. */
int fvgp_hip_nn_loglik(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *thetas_host, int ntheta, int B,
                       const int *idx, int64_t ld, int m, const double *r, const double *v, double *mu, double *var,
                       double *work, int64_t work_bytes, double *out_host, int64_t *info_host);

/* bytes of the caller-owned `work` of the call `what` (FVGP_NN_SEARCH: 0, it takes none) for nq query rows and B hyperparameter
 * vectors: the theta table (B (1 + FVGP_MAX_DIM) doubles) and the info word; for the likelihood also two sums per (b, slice of 256
 * rows) and the three results per b.  -1 for an unknown `what`, nq < 1 or B < 1. */
int64_t fvgp_hip_nn_workspace_bytes(int what, int64_t nq, int B);

/* The likelihood and its exact gradient in the hyperparameters: fvgp_hip_nn_loglik, and per (b, row i) the score
 *     score[b][i][h] = d/d theta_h log p(y_i | y_c(i)),      grad_host[b][h] = sum_i score[b][i][h] = d log p / d theta_h.
 * No second factorisation: with the row's L still in place, a = L^-T w = A^-1 k and beta = L^-T z = A^-1 r_c (one backward pass for
 * both, step j = M - 1 .. 0 taking a_j from lane j and the lanes l < j subtracting L[j][l] a_j), e = r_i - mu, d = var, the
 * (m + 1)-vectors b = (-a, 1), g = (beta, 0),
 *     q = (e / d) g + 1/2 (e^2 / d^2 - 1 / d) b,        score_h = b^T (dSigma / d theta_h) q,
 * Sigma the kernel part of the joint covariance of (c, i) (the noise is no hyperparameter); as dSigma is symmetric the form is
 * sum_{p > q'} (b_p q_q' + b_q' q_p) dSigma[p][q'] + sum_p b_p q_p dSigma[p][p], one more sweep over the (m + 1)(m + 2) / 2 entries, each
 * evaluated with its derivative: dK / d sigma^2 = phi, dK / d l_k = cf e2[k] invl[k]; a kernel with one length scale for every dimension
 * adds the d terms into it.  A row without neighbours has the sigma^2 term of d = k(x, x) + v alone.  score (B, n, ntheta) device:
 * columns past the kernel's own hyperparameters receive +0.0 (so does grad_host there), and nothing else depends on ntheta.
 * BIT CONTRACT: out_host, mu and var are bit for bit those of fvgp_hip_nn_loglik on the same inputs.  score[b][i][:] is a function of
 * (x_i, v_i, the listed rows in their listed order, theta_b, m) alone: not of n, B, or the position in either.  The rows' scores are added
 * as the likelihood's terms are (slices of 256 rows by a halving tree, the slices to 0 in ascending order, one thread per (b, h)): the
 * same call gives the same bits, and row b of grad_host does not depend on B.
 * A failed pivot gives NaN scores next to the NaN mu and var, and the same info; grad_host is then NaN.
 * work: device, 8-byte aligned, fvgp_hip_nn_grad_workspace_bytes(n, B, ntheta) bytes.
 * Errors: -1 h, -2 unknown kernel_id, -3 x, -4 n < 1 or past 2^31 - 1, -5 d outside 1 .. FVGP_MAX_DIM, -6 thetas_host, -7 too few
 * hyperparameters, -8 B outside 1 .. 65535, -9 idx, -10 ld < m, -11 m outside 1 .. FVGP_NN_MAX_NEIGHBORS, -12 r, -13 v, -14 mu, -15 var,
 * -16 score, -17 work NULL or misaligned, -18 work_bytes too small, -19 out_host, -20 grad_host, -21 info_host. */
int fvgp_hip_nn_loglik_grad(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *thetas_host, int ntheta, int B,
                            const int *idx, int64_t ld, int m, const double *r, const double *v, double *mu, double *var, double *score,
                            double *work, int64_t work_bytes, double *out_host, double *grad_host, int64_t *info_host);

/* bytes of the caller-owned `work` of fvgp_hip_nn_loglik_grad: the likelihood's, then the gradient per b and one sum per (b, slice of 256
 * rows, hyperparameter).  -1 for n < 1, B < 1 or ntheta < 1. */
int64_t fvgp_hip_nn_grad_workspace_bytes(int64_t n, int B, int ntheta);

/* The likelihood, its gradient and the Fisher information of the product of conditionals: everything
 * fvgp_hip_nn_loglik_grad does, and per (b, row i) the row's expected negative Hessian under the exact GP,
 *     F_i = F(Sigma_ci + noise) - F(A),   F(S)[h][k] = 1/2 tr(S^-1 d_h S S^-1 d_k S),     fisher_host[b] = sum_i F_i.
 * The Cholesky factor of the joint block extends L by the row (w^T, sqrt(d)), and the difference collapses to that row: with b = (-a, 1),
 *     t_h = (d_h Sigma b) on the neighbours,   delta_h = b^T d_h Sigma b = d_h var,   u_h = L^-1 t_h,
 *     F_i[h][k] = u_h^T u_k / var + 1/2 delta_h delta_k / var^2        (= E[d_h mu d_k mu] / var + 1/2 d_h var d_k var / var^2),
 * each F_i positive semidefinite.  No second factorisation: one more sweep over the block's entries with their derivatives (both
 * triangles, as t is a matrix-vector product), one forward pass with every right-hand side, the np (np + 1) / 2 products by the halving
 * tree.  A row without neighbours has 1/2 delta delta^T / var^2 alone, delta = (1, 0, ..).  With every earlier point a neighbour the sum
 * is the dense 1/2 tr((K + V)^-1 d_h K (K + V)^-1 d_k K).
 * fisher_rows (B, n, P) device, P = ntheta (ntheta + 1) / 2: the packed lower triangle of F_i, (h, k <= h) at h (h + 1) / 2 + k; entries
 * that involve a column past the kernel's own hyperparameters receive +0.0.  fisher_host (B, ntheta, ntheta) host: the sums, full symmetric.
 * BIT CONTRACT: out_host, mu, var, score and grad_host are bit for bit those of fvgp_hip_nn_loglik_grad on the same inputs.
 * fisher_rows[b][i][:] is a function of (x_i, v_i, the listed rows in their listed order, theta_b, m) alone: not of n, B, or the position in
 * either, and -- unlike the score -- not of r.  The rows' terms are added as the scores are (slices of 256 rows by a halving tree, the
 * slices to 0 in ascending order, one thread per (b, entry), no atomics): the same call gives the same bits, and row b of fisher_host
 * does not depend on B.
 * A failed pivot gives a NaN row of fisher_rows next to the NaN mu, var and scores, and the same info; fisher_host[b] is then NaN.
 * work: device, 8-byte aligned, fvgp_hip_nn_fisher_workspace_bytes(n, B, ntheta) bytes.
 * Errors: -1 h, -2 unknown kernel_id, -3 x, -4 n < 1 or past 2^31 - 1, -5 d outside 1 .. FVGP_MAX_DIM, -6 thetas_host, -7 too few
 * hyperparameters, -8 B outside 1 .. 65535, -9 idx, -10 ld < m, -11 m outside 1 .. FVGP_NN_MAX_NEIGHBORS, -12 r, -13 v, -14 mu, -15 var,
 * -16 score, -17 fisher_rows, -18 work NULL or misaligned, -19 work_bytes too small, -20 out_host, -21 grad_host, -22 fisher_host,
 * -23 info_host. */
int fvgp_hip_nn_loglik_fisher(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *thetas_host, int ntheta, int B,
                              const int *idx, int64_t ld, int m, const double *r, const double *v, double *mu, double *var, double *score,
                              double *fisher_rows, double *work, int64_t work_bytes, double *out_host, double *grad_host,
                              double *fisher_host, int64_t *info_host);

/* bytes of the caller-owned `work` of fvgp_hip_nn_loglik_fisher: the gradient call's, then the packed sums per b and one sum per (b, slice
 * of 256 rows, packed entry).  -1 for n < 1, B < 1 or ntheta < 1. */
int64_t fvgp_hip_nn_fisher_workspace_bytes(int64_t n, int B, int ntheta);

/* ---- the exact cell-grid search (csrc/nn_grid.hip): the lists of fvgp_hip_nn_search in near-linear time, d <= 3 ---- */
#define FVGP_NN_GRID_MAX_DIM 3     /* most dimensions of the cell grid */
#define FVGP_NN_GRID_INFO 20       /* doubles of the host record fvgp_hip_nn_grid_build leaves for fvgp_hip_nn_grid_search */

/* bytes of the caller-owned device buffer that holds the grid of nr reference rows in d dimensions: the rows' coordinates bucketed by
 * cell (nr d doubles), the cells' first positions (at most min(nr, 2^24) + 1 ints) and the bucketed row indices (nr ints).  A function
 * of (nr, d) alone, not of the data.  -1 for nr < 1 or past 2^31 - 1, d outside 1 .. FVGP_NN_GRID_MAX_DIM. */
int64_t fvgp_hip_nn_grid_bytes(int64_t nr, int d);

/* bytes of the caller-owned `work` of fvgp_hip_nn_grid_build: the box partials, every row's cell and rank, the block sums of the scan.
 * -1 as above. */
int64_t fvgp_hip_nn_grid_workspace_bytes(int64_t nr, int d);

/* Build the grid over the reference rows xr (nr, d), d <= 3, in the search's scaled coordinates (scales_host_or_null as in
 * fvgp_hip_nn_search): cubic cells of one scaled edge h over the rows' bounding box, about two rows per cell on average and at most
 * min(nr, 2^24) cells; a dimension of zero extent, or thinner than a cell, has one cell.  Row x lies in cell
 * min(floor(((x[k] - lo[k]) * (1 / scales[k])) * (1 / h)), cells[k] - 1) of dimension k.  grid_dev receives the rows bucketed by cell;
 * info_host (FVGP_NN_GRID_INFO doubles, host) what was chosen: { a magic word, nr, d, scales[3], 1 / scales[3], lo[3], h, 1 / h,
 * cells[3], their product, the causal candidate count below which the search takes the brute entry, 0 }.
 * Steps: the box by a reduction, read back (the call SYNCHRONISES the stream once, there); every row's cell and its rank inside the cell
 * by an integer atomic on the cell's counter; an exclusive scan of the counts; the scatter.  Cost O(nr d + cells), independent of how
 * many rows share a cell.  Returns with the last launches still in the stream: a search on the same handle may follow at once.
 * BIT CONTRACT: info_host is a function of (xr, scales) alone.  The order of the rows inside a cell's bucket is not (it follows the
 * atomics), and no result of fvgp_hip_nn_grid_search depends on it.
 * grid_dev: device, 8-byte aligned, fvgp_hip_nn_grid_bytes(nr, d) bytes; work: device, 8-byte aligned,
 * fvgp_hip_nn_grid_workspace_bytes(nr, d) bytes, free again when the stream has passed the call.
 * Errors: -1 h, -2 xr, -3 nr < 1 or past 2^31 - 1, -4 d outside 1 .. FVGP_NN_GRID_MAX_DIM (fvgp_hip_nn_search remains the route there),
 * -5 a scale that is not positive and finite, -6 grid_dev NULL or misaligned, -7 grid_bytes too small, -8 work NULL or misaligned,
 * -9 work_bytes too small, -10 info_host, -11 a coordinate of xr, or the scaled extent of the box, is not finite (nothing was built). */
int fvgp_hip_nn_grid_build(fvgp_handle *h, const double *xr, int64_t nr, int d, const double *scales_host_or_null, void *grid_dev,
                           int64_t grid_bytes, void *work, int64_t work_bytes, double *info_host);

/* fvgp_hip_nn_search through the grid: idx_out (nq, ld >= m) int32 receives, ELEMENT FOR ELEMENT, what fvgp_hip_nn_search writes for the
 * same (xq, xr, m, c0) under the scales the grid was built with -- min(m, candidates) entries sorted by (distance, index) ascending, ties
 * to the lower index, then -1 up to column m; columns m .. ld are not written; c0 as there.  xr, nr, d: the rows the grid was built over,
 * unchanged since; info_host and grid_dev: what that build left.
 * A lane per query.  Every candidate's distance is computed by the brute kernel's operations; cells are visited in growing shells around
 * the query's cell (queries outside the box start from the nearest border cell) and the running list is ordered by the pair
 * (distance, index) explicitly.  The walk of a query ends when every cell has been visited, or when the list is full and its worst
 * distance is strictly below (1 - 2^-20) times the square of a lower bound, itself lowered by 2^-40 (|cell coordinate| + cells + 2)
 * cells, on the computed distance to any row in a cell not visited yet.  In a causal call the queries with fewer than 1024 (nr < 65536) or 4096
 * candidates are searched by fvgp_hip_nn_search itself.  Every loop is bounded by the cells per dimension or a cell's occupancy.
 * BIT CONTRACT: that of fvgp_hip_nn_search -- a row is a function of its query, the reference rows, the scales, m and its candidate count
 * alone: not of the other queries, the launch geometry, the cell sizes or the order of the rows inside a bucket.
 * Query coordinates that are not finite are the caller's error: such a row receives legal candidates, not necessarily the brute entry's.
 * Cost: for rows spread evenly, O(m) distances per query once the candidates outnumber m by far; a causal query i visits about N m / i
 * rows' worth of cells; clustered rows cost what their fullest visited cells hold.  Asynchronous.
 * Errors: -1 h, -2 xq, -3 nq < 1, -4 xr, -5 nr < 1 or past 2^31 - 1, -6 d outside 1 .. FVGP_NN_GRID_MAX_DIM, -8 m outside
 * 1 .. FVGP_NN_MAX_NEIGHBORS, -9 info_host NULL or not the record of a grid over (nr, d), -10 idx_out, -11 ld < m, -12 grid_dev NULL or
 * misaligned. */
int fvgp_hip_nn_grid_search(fvgp_handle *h, const double *xq, int64_t nq, const double *xr, int64_t nr, int d, int m, int64_t c0,
                            const double *info_host, const void *grid_dev, int *idx_out, int64_t ld);

/* ---- the nearest-neighbour factor as a preconditioner of the matrix-free solves (csrc/nn.hip, csrc/matrix_free.hip) ----
 * With every row's conditional, the sparse lower-triangular W whose row i is (-a, 1) / sqrt(d_i) -- a = A^-1 k on the row's neighbours,
 * d_i its conditional variance -- satisfies (K + V)^-1 ~ W^T W, exactly with m >= n - 1: the Vecchia / KL-optimal sparse inverse
 * Cholesky factor.  W^T W is symmetric positive definite whenever every d_i is positive, costs O(n m) to hold and to apply, and stays
 * local where the rank-q pivoted Cholesky of fvgp_hip.h is global. */

/* bytes of the caller-owned `work` of fvgp_hip_nn_factor for n rows: the info word, the theta table and the n conditional variances
 * d_i.  -1 for n < 1. */
int64_t fvgp_hip_nn_factor_workspace_bytes(int64_t n);

/* The factor's rows.  x (n, d) in the ordering, idx (n, ld >= m) the lists of the likelihood (the conventions of the conditionals entry:
 * entries outside 0 .. n - 1 are skipped wherever they stand, an empty list is legal, columns m .. ld are never read), ONE theta, v (n)
 * the noise.  With A = K(x_c, x_c) + diag(v_c) = L L^T, k = K(x_c, x_i), w = L^-1 k, a = L^-T w (the backward pass of the gradient
 * entry), d_i = (k(x_i, x_i) + v_i) - w^T w:
 *     dinv[i] = 1 / sqrt(d_i),      coef[i][l] = -(a_l dinv[i]),  +0.0 where entry l of the list is skipped.
 * coef (n, ldc >= m), columns m .. ldc are not written; dinv (n).  The assembly, the factorisation and d_i are the conditionals entry's
 * own code (one more level of the same kernel); the data values r are never read.
 * BIT CONTRACT: row i of coef and dinv[i] are functions of (x_i, v_i, the listed rows in their listed order, theta, m) alone: not of n
 * or the position in it.  d_i has the bits of var[i] of the conditionals entry on the same inputs with s = v, and dinv[i] is the
 * correctly rounded 1 / (correctly rounded sqrt(d_i)).
 * A pivot that is not positive gives NaN in dinv[i] and in columns 0 .. m - 1 of coef's row; nothing traps.  info_host: 0, or 1 + i of
 * the first row whose d_i is not positive (NaN included).  Synchronises the stream.
 * work: device, 8-byte aligned, fvgp_hip_nn_factor_workspace_bytes(n) bytes.
 * Errors: -1 h, -2 unknown kernel_id, -3 x, -4 n < 1 or past 2^31 - 1, -5 d outside 1 .. FVGP_MAX_DIM, -6 theta_host, -7 too few
 * hyperparameters, -8 idx, -9 ld < m, -10 m outside 1 .. FVGP_NN_MAX_NEIGHBORS, -11 v, -12 coef, -13 ldc < m, -14 dinv, -15 work NULL or
 * misaligned, -16 work_bytes too small, -17 info_host. */
int fvgp_hip_nn_factor(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta_host, int ntheta,
                       const int *idx, int64_t ld, int m, const double *v, double *coef, int64_t ldc, double *dinv,
                       double *work, int64_t work_bytes, int64_t *info_host);

/* bytes of the caller-owned `work` of fvgp_hip_nn_precond_apply for n rows: R, the intermediate T and Z in the solver's layout of
 * FVGP_PCG_MAX_RHS columns, and one partial per 256 rows and column.  -1 for n < 1. */
int64_t fvgp_hip_nn_precond_apply_workspace_bytes(int64_t n);

/* Z[:, :s] = W^T (W R[:, :s]), s <= FVGP_PCG_MAX_RHS.  The factor is (idx, coef, dinv) with ONE leading dimension ld >= m for idx and
 * coef, and the transposed lists: tr_start (n + 1) int64, tr_pos (nnz) int64 -- bucket j = tr_pos[tr_start[j] .. tr_start[j + 1]) holds
 * the flat positions i ld + l of the entries with idx[i][l] == j in ascending i (the binding builds them on the host by a stable sort,
 * once per neighbour structure).  Two launches in stream order over the solver's layout (a row is 16 doubles, 16 lanes take a row, one
 * column each, so that a wave instruction reads four whole 128-byte rows):
 *     gather     T[i][c] = dinv[i] R[i][c] + sum_{l = 0 .. m - 1} coef[i][l] R[idx[i][l]][c]     fused multiply-adds in ascending l,
 *     transpose  Z[j][c] = dinv[j] T[j][c] + sum_{e in bucket j, ascending} coef_flat[pos_e] T[pos_e / ld][c].
 * An entry of idx outside 0 .. n - 1 and a position outside 0 .. n ld - 1 are skipped, not read; bucket bounds are clipped to
 * 0 .. nnz, and nothing of tr_pos at or past tr_start[n] is read.  A bucket's loop is bounded by its length alone (with coincident
 * points one bucket can hold most rows); no atomics, no grid barrier, no dependence between workgroups.
 * BIT CONTRACT: Z[.][c] is a function of (the factor, R[.][c]) alone: the same bits whatever s, the other columns or the launch geometry.
 * Asynchronous.  work: device, 16-byte aligned, fvgp_hip_nn_precond_apply_workspace_bytes(n) bytes.
 * Errors: -1 h, -2 n < 1 or past 2^31 - 1, -3 idx, -4 ld < m, -5 m outside 1 .. FVGP_NN_MAX_NEIGHBORS, -6 coef, -7 dinv, -8 tr_start,
 * -9 tr_pos, -10 nnz < 0 or past n ld, -11 R, -12 ldr < s, -13 s outside 1 .. FVGP_PCG_MAX_RHS, -14 Z, -15 ldz < s, -16 work NULL or
 * misaligned, -17 work_bytes too small. */
int fvgp_hip_nn_precond_apply(fvgp_handle *h, int64_t n, const int *idx, int64_t ld, int m, const double *coef, const double *dinv,
                              const int64_t *tr_start, const int64_t *tr_pos, int64_t nnz, const double *R, int64_t ldr, int s,
                              double *Z, int64_t ldz, double *work, int64_t work_bytes);

/* bytes of the caller-owned `work` of fvgp_hip_pcg_nn: the solver's with no low-rank part, and the (n, FVGP_PCG_MAX_RHS) intermediate
 * T.  -1 for n < 1. */
int64_t fvgp_hip_pcg_nn_workspace_bytes(int64_t n);

/* The preconditioned conjugate gradients of fvgp_hip.h (the entry fvgp_hip_pcg: same recurrences, same kernels, same stopping rules, same
 * outputs) with z = W^T W r in the place of the low-rank preconditioner: the arguments of that entry, the sparse factor (as
 * fvgp_hip_nn_precond_apply takes it) where it has (G, ldg, q, C, ldc).  x, vdiag, B and X are in the factor's ordering.  The apply
 * leaves the r.z partials per 256 rows where the low-rank apply leaves them, and the scalar steps are the same kernel.
 * BIT CONTRACT: that of the entry fvgp_hip_pcg -- a column's iterates do not depend on s or on the other columns.
 * Errors: -1 h, -2 unknown kernel_id, -3 x, -4 n < 1, -5 d, -6 theta, -7 too few hyperparameters, -8 vdiag, -9 idx, -10 ld < m, -11 m
 * outside 1 .. FVGP_NN_MAX_NEIGHBORS, -12 coef, -13 dinv, -14 tr_start, -15 tr_pos, -16 nnz < 0 or past n ld, -17 B, -18 ldb < s, -19 s
 * outside 1 .. FVGP_PCG_MAX_RHS, -20 X, -21 ldx < s, -23 tol not positive, -24 max_iter < 1, -25 check_every < 1, -26 max_restarts < 0,
 * -27 work NULL or misaligned (16 bytes), -28 work_bytes too small, -29 iters_host, -30 relres_host, -31 status_host. */
int fvgp_hip_pcg_nn(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
                    const double *vdiag, const int *idx, int64_t ld, int m, const double *coef, const double *dinv,
                    const int64_t *tr_start, const int64_t *tr_pos, int64_t nnz,
                    const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
                    double tol, int max_iter, int check_every, int max_restarts,
                    double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host);

/* bytes of the caller-owned `work` of the maxmin ordering below: the n distances to the nearest pick and two rows of per-workgroup
 * partials.  -1 for n < 1. */
int64_t fvgp_hip_nn_maxmin_workspace_bytes(int64_t n);

/* The exact maxmin (farthest-point, coarse-to-fine) ordering of the rows of x (n, d) (csrc/nn_order.hip).  With the search's
 * distance  dist(i, j) = sum_k ((x[i][k] - x[j][k]) * (1 / scales[k]))^2  (scales_host NULL: 1; fused multiply-adds in ascending k):
 *     perm_out[0] = first,      perm_out[t] = the i not picked yet with the largest  mindist_t(i) = min_{s < t} dist(i, perm_out[s]),
 * ties to the lowest index, for t < q.  dist_out (q) or NULL: dist_out[t] = mindist_t(perm_out[t]), the SQUARED scaled distance at which
 * the point entered; dist_out[0] = +inf, dist_out[1 ..] never increases.  Duplicated points have mindist 0 and come last, in index order:
 * with q = n every point is ordered.  perm_out (q) int64, device.
 * One launch per step, q launches in stream order: every workgroup reduces the previous step's per-workgroup partials to the same pick,
 * lowers the mindist of its own strip of points against it and leaves its best point as its partial.  No atomics, no host
 * synchronisation: asynchronous.  O(q n d) flops.
 * BIT CONTRACT: perm_out and dist_out are functions of (x, scales, first, q) alone -- the same bits on every call, whatever the grid --
 * and the first q' entries of a call with q are those of the call with q' < q.  mindist_t(i) depends on x[i] and the t earlier picks
 * alone: rows appended to x change nothing before the first step at which one of them is picked.
 * Coordinates that are not finite are the caller's error: a distance that comes out as no number counts as 0 (such a point is ordered
 * with the duplicates), an infinite one as the largest.  Every entry of perm_out is one of 0 .. n - 1 and none repeats, whatever x holds.
 * work: device, 8-byte aligned, the bytes the sizing entry above gives for n.
 * Errors: -1 h, -2 x, -3 n < 1 or past 2^31 - 1, -4 d outside 1 .. FVGP_MAX_DIM, -5 a scale that is not positive and finite, -6 first
 * outside 0 .. n - 1, -7 q outside 1 .. n, -8 perm_out, -10 work NULL or misaligned, -11 work_bytes too small. */
int fvgp_hip_nn_maxmin_order(fvgp_handle *h, const double *x, int64_t n, int d, const double *scales_host_or_null,
                             int64_t first, int64_t q, int64_t *perm_out, double *dist_out_or_null,
                             double *work, int64_t work_bytes);

#ifdef __cplusplus
}
#endif
#endif
