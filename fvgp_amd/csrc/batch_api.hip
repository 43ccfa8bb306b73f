// Host side of the C ABI: the three batched evaluations (batch.hip, grad_batch.hip, posterior_batch.hip) with their workspace sizes.
#include "common.h"
#include "kernel_family.h"
#include <math.h>
#include <functional>

extern "C" {

int64_t fvgp_hip_loglik_batch_dim(int64_t n, int ncol) {
    const int64_t dim = fvgp_hip_loglik_dim(n, ncol);
    if (dim < 0) return -1;
    return dim <= FVGP_BATCH_MAX_DIM ? dim : 0;
}
// The handle's buffer for B problems of one batched evaluation.  Per problem: the block inverses (BATCH_VALUE: one slot, the current step's;
// else every leaf's, dim / 128 of them), the reciprocal pivots of every step, the theta table row; BATCH_GRAD: z and b (2 padded_dim(n)) and
// the trace's partial sums (T (T + 1) / 2 tiles x (1 + FVGP_MAX_DIM), T = padded_dim(n) / 128); then, packed, the block the host reads back
// in ONE copy of back_bytes from `red` on: two reductions, BATCH_GRAD: the gradient row, the info word
enum { BATCH_VALUE = 0, BATCH_GRAD = 1, BATCH_POSTERIOR = 2 };
struct BatchWs { double *linv, *logdet, *tab, *zb, *partial, *red, *grad; int *info; int64_t lstride, zstride, pstride, ntiles; size_t back_bytes; };
static BatchWs batch_layout(Carve &c, int which, int64_t n, int64_t dim, int64_t B) {
    constexpr int64_t TW = 1 + FVGP_MAX_DIM, D = sizeof(double);
    const int64_t np = pad128(n), T = np / TILE;
    BatchWs l{};
    l.lstride = which == BATCH_VALUE ? LEAF_DOUBLES : (dim / TILE) * LEAF_DOUBLES;
    l.linv = c.take<double>(B * l.lstride, D); l.logdet = c.take<double>(B * dim, D); l.tab = c.take<double>(B * TW, D);
    if (which == BATCH_GRAD) {
        l.zstride = 2 * np; l.ntiles = T * (T + 1) / 2; l.pstride = l.ntiles * TW;
        l.zb = c.take<double>(B * l.zstride, D); l.partial = c.take<double>(B * l.pstride, D);
    }
    const int64_t back = c.bytes();
    l.red = c.take<double>(2 * B, D);
    if (which == BATCH_GRAD) l.grad = c.take<double>(B * TW, D);
    l.info = c.take<int>(B, sizeof(int));
    l.back_bytes = (size_t)(c.bytes() - back);
    return l;
}

int64_t fvgp_hip_loglik_batch_workspace_bytes(int64_t n, int ncol, int64_t B) {
    const int64_t dim = fvgp_hip_loglik_batch_dim(n, ncol);
    if (dim <= 0 || B < 1) return -1;
    return carve_bytes(batch_layout, BATCH_VALUE, n, dim, B);
}

int64_t fvgp_hip_loglik_grad_batch_workspace_bytes(int64_t n, int ncol, int64_t B) {
    const int64_t dim = fvgp_hip_loglik_batch_dim(n, ncol);
    if (dim <= 0 || B < 1) return -1;
    return carve_bytes(batch_layout, BATCH_GRAD, n, dim, B);
}

// (the prediction rows live in the caller's scratch, so P_chunk adds nothing here)
int64_t fvgp_hip_posterior_batch_workspace_bytes(int64_t n, int ncol, int64_t B, int64_t P_chunk) {
    const int64_t dim = fvgp_hip_loglik_batch_dim(n, ncol);
    if (dim <= 0 || B < 1 || P_chunk < TILE || P_chunk % TILE) return -1;
    return carve_bytes(batch_layout, BATCH_POSTERIOR, n, dim, B);
}

// kmat_desc_from_theta numbers a bad d or ntheta as fvgp_hip_kmat's arguments (7, 9); in the batched entries they are arguments 5 and 7
static inline int batch_theta_rc(int rc) { return rc == -7 ? -5 : rc == -9 ? -7 : rc; }

// sigma^2 and 1 / l of every problem, exactly as the single evaluation computes them (kmat_desc_from_theta), into the device table `tab`
// (B rows of 1 + FVGP_MAX_DIM); argument errors numbered as in fvgp_hip_loglik_batch
static int batch_theta_table(fvgp_handle *h, int kernel_id, int d, const double *thetas, int ntheta, int64_t B, double *tab) {
    constexpr int TW = 1 + FVGP_MAX_DIM;
    h->bat_tab_host.assign((size_t)(B * TW), 0.0);
    for (int64_t b = 0; b < B; ++b) {
        KmatDesc kd{};
        const int rc = kmat_desc_from_theta(kernel_id, d, thetas + b * ntheta, ntheta, &kd); if (rc) return batch_theta_rc(rc);
        h->bat_tab_host[(size_t)(b * TW)] = kd.sig;
        for (int q = 0; q < d; ++q) h->bat_tab_host[(size_t)(b * TW + 1 + q)] = kd.invl[q];
    }
    HIPCHK(hipMemcpyAsync(tab, h->bat_tab_host.data(), (size_t)(B * TW) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return 0;
}

// the handle's buffer grown to what the evaluation `which` needs, and carved
static int batch_workspace(fvgp_handle *h, int which, int64_t n, int64_t dim, int64_t B, BatchWs *l) {
    const size_t ws = (size_t)carve_bytes(batch_layout, which, n, dim, B);
    if (ws > h->bat_cap) {
        if (h->bat_ws) HIPCHK(hipFree(h->bat_ws));
        h->bat_ws = nullptr; h->bat_cap = 0;
        HIPCHK(hipMalloc((void **)&h->bat_ws, ws));
        h->bat_cap = ws;
    }
    Carve c(h->bat_ws); *l = batch_layout(c, which, n, dim, B);
    return 0;
}

// the factorisation of Bs problems whose squares start at K0 (stride apart; stride 0 for one) by recursive halving over the block
// columns, with `rows` >= dim rows per problem: the rows dim .. rows - 1 under a square (fvgp_hip_posterior_batch's prediction rows) ride
// along in the panel TRSM and in the update between two halves -- their tiles lie below the diagonal, ordinary tiles of the same launches,
// and a tile's bits do not depend on how many tile rows its launch has.  The leaf of block column k0 of problem b writes its block
// inverse to linv + b * linv_stride + (k0 / 128) * leaf_step (leaf_step 0: one slot per problem, overwritten step by step).  solve_only:
// the square is factored already and every leaf inverse kept (leaf_step > 0): no leaves, the TRSM and the updates on the rows from dim
// on only -- tile for tile the operations the full pass applies to those rows.  Every GEMM carries an explicit K range, so that it takes
// the 128-tile kernel whatever Bs is (a plain one-problem launch of a few tiles would take the 64-tile kernel: other bits).
static int batch_recursion(fvgp_handle *h, int64_t n, double *K0, int64_t ld, int64_t stride, int64_t dim, int64_t rows, double *linv,
                           int64_t linv_stride, int64_t leaf_step, double *logdet, int *info, int64_t Bs, bool solve_only) {
    // one 128-column step: leaf, then the TRSM of every row below by the block inverse
    auto step = [&](int64_t k0) -> int {
        const int64_t nv = n - k0, r0 = solve_only ? dim : k0 + TILE, R = rows - r0;
        double *li = linv + (k0 / TILE) * leaf_step;
        if (!solve_only) {
            int r = launch_leaf_batch(h, K0 + k0 * ld + k0, ld, stride, li, logdet + k0, dim, info, (int)k0,
                                      nv >= TILE ? TILE : (nv > 0 ? (int)nv : 0), Bs, linv_stride);
            if (r) return r;
        }
        if (R <= 0) return 0;
        double *P = K0 + r0 * ld + k0;
        // rows below <- rows below * inv(L_kk)^T, in place
        return launch_gemm(h, gemm_desc(0, 0, R, TILE, TILE, 1.0, P, ld, li, TILE, 0.0, P, ld).k_end(TILE).batched(Bs, stride, linv_stride, stride));
    };
    // recursive halving over the block columns (panel_factor_recursive's order, the whole square one panel): left half, ONE update
    // of the right half's columns (every row below them, lower tiles) with K = the left half's width, right half.  The same flops
    // as an update after every 128 columns, with far fewer read-modify-write passes over the trailing tiles.  The schedule
    // depends on dim only.
    std::function<int(int64_t, int64_t)> factor = [&](int64_t J0, int64_t Jend) -> int {
        const int64_t blocks = (Jend - J0) / TILE;
        if (blocks <= 1) return step(J0);
        const int64_t mid = J0 + (blocks / 2) * TILE;
        int r = factor(J0, mid); if (r) return r;
        // rows [r0, rows) x columns [mid, Jend) -= L[r0:, J0:mid] L[mid:Jend, J0:mid]^T from r0 = mid on the lower tiles; solve_only: the rows
        // from dim on only, all their tiles (they lie below every diagonal tile)
        const int64_t r0 = solve_only ? dim : mid;
        GemmDesc u = gemm_desc(0, 0, rows - r0, Jend - mid, mid - J0, -1.0, K0 + r0 * ld + J0, ld, K0 + mid * ld + J0, ld, 1.0, K0 + r0 * ld + mid, ld)
                         .k_end(mid - J0).batched(Bs, stride, stride, stride);
        if (!solve_only) u.lower_tiles();
        r = launch_gemm(h, u); if (r) return r;
        return factor(mid, Jend);
    };
    return factor(0, dim);
}

// the batched evaluation of Bs problems whose squares start at K0 (stride apart; stride 0 for one): assembly, appended rows, the
// factorisation by recursive halving (batch_recursion over the square alone), tail -> red (2 per problem)
static int batch_factor(fvgp_handle *h, int kind, const double *x, int64_t n, int d, const double *tab, const double *vdiag, int64_t vdiag_stride,
                        const double *ymean, int64_t ymean_stride, int ncol, double *K0, int64_t ld, int64_t stride, int64_t dim,
                        double *linv, int64_t linv_stride, int64_t leaf_step, double *logdet, int *info, double *red, int64_t Bs) {
    int rc = launch_kmat_batch(h, kind, x, n, d, tab, vdiag, vdiag_stride, K0, ld, stride, dim, Bs); if (rc) return rc;
    rc = launch_rhs_rows_batch(h, K0, stride, n, ld, ymean, ymean_stride, ncol, vdiag, vdiag_stride, Bs); if (rc) return rc;
    rc = batch_recursion(h, n, K0, ld, stride, dim, dim, linv, linv_stride, leaf_step, logdet, info, Bs, false); if (rc) return rc;
    return launch_loglik_tail_batch(h, logdet, dim, K0, stride, ld, n, ncol, red, Bs);
}

// {log-likelihood, log|KV|, quad / ncol} of problem b from its two reductions, NaN where info says the factorisation failed
static void batch_results(int64_t n, int ncol, int64_t B, const double *r, const int *inf, double *out_host, int *info_host) {
    for (int64_t b = 0; b < B; ++b) {
        const int ib = inf[b] > n ? 0 : inf[b];        // (cannot exceed n: the padding is an identity block)
        if (info_host) info_host[b] = ib;
        if (ib != 0) { out_host[3 * b] = out_host[3 * b + 1] = out_host[3 * b + 2] = NAN; continue; }
        const double logdet_b = 2.0 * r[2 * b], quad = r[2 * b + 1] / (double)ncol;
        out_host[3 * b] = -0.5 * (quad + logdet_b + (double)n * log(2.0 * M_PI));
        out_host[3 * b + 1] = logdet_b;
        out_host[3 * b + 2] = quad;
    }
}

// B independent evaluations side by side (batch.hip): assembly, appended rows, then the factorisation by recursive halving over the
// block columns (batch_recursion) -- per 128 columns one leaf launch and one panel TRSM (product with the block inverse), between the
// two halves of every halving ONE update of the right half's lower tiles with K = the left half's width --, each launch over every
// problem, then one tail.
int fvgp_hip_loglik_batch(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                          const double *thetas, int ntheta, int64_t B,
                          const double *vdiag, int64_t vdiag_stride, const double *ymean, int64_t ymean_stride, int ncol,
                          double *KV, int64_t ld, int64_t kv_stride, double *out_host, int *info_host) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (n > FVGP_BATCH_MAX_DIM) { fvgp_set_error("loglik_batch: n exceeds FVGP_BATCH_MAX_DIM"); return -4; }
    if (!thetas) return -6;
    if (B < 1) { fvgp_set_error("loglik_batch: B >= 1"); return -8; }
    KmatDesc k0d{};
    int rc = kmat_desc_from_theta(kernel_id, d, thetas, ntheta, &k0d);
    if (rc) return batch_theta_rc(rc);
    if (!vdiag) { fvgp_set_error("loglik_batch needs the noise variances (vdiag)"); return -9; }
    if (vdiag_stride < 0) return -10;
    if (!ymean) return -11;
    if (ymean_stride < 0) return -12;
    if (ncol < 1 || ncol > FVGP_MAX_RHS_VEC) { fvgp_set_error("1 <= ncol <= 8"); return -13; }
    const int64_t dim = fvgp_hip_loglik_batch_dim(n, ncol);
    if (dim <= 0) { fvgp_set_error("loglik_batch: fvgp_hip_loglik_batch_dim(n, ncol) exceeds FVGP_BATCH_MAX_DIM"); return -4; }
    if (!KV || ((uintptr_t)KV & 15)) { fvgp_set_error("loglik_batch: KV must be 16-byte aligned"); return -14; }
    if (ld < dim || (ld & 1)) { fvgp_set_error("loglik_batch: the leading dimension must be even and >= fvgp_hip_loglik_batch_dim(n, ncol)"); return -15; }
    if (B > 1 && (kv_stride < dim * ld || (kv_stride & 1))) { fvgp_set_error("loglik_batch: kv_stride must be even and >= dim * ld"); return -16; }
    if (!out_host) return -17;
    HIPCHK(hipSetDevice(h->device));
    BatchWs l;
    rc = batch_workspace(h, BATCH_VALUE, n, dim, B, &l); if (rc) return rc;
    constexpr int TW = 1 + FVGP_MAX_DIM;
    double *linv = l.linv, *logdet = l.logdet, *tab = l.tab, *red = l.red;
    int *info = l.info;
    rc = batch_theta_table(h, kernel_id, d, thetas, ntheta, B, tab); if (rc) return rc;
    HIPCHK(hipMemsetAsync(info, 0, (size_t)B * sizeof(int), h->stream));
    const int64_t stride = B > 1 ? kv_stride : 0;
    // grid dimensions y / z take at most 65535: the problems go in groups of that many (results do not depend on the grouping)
    constexpr int64_t GROUP = 65535;
    for (int64_t b0 = 0; b0 < B; b0 += GROUP) {
        const int64_t Bs = B - b0 < GROUP ? B - b0 : GROUP;
        rc = batch_factor(h, k0d.kind, x, n, d, tab + b0 * TW, vdiag + b0 * vdiag_stride, vdiag_stride, ymean + b0 * ymean_stride, ymean_stride, ncol,
                          KV + b0 * stride, ld, stride, dim, linv + b0 * LEAF_DOUBLES, LEAF_DOUBLES, 0, logdet + b0 * dim, info + b0, red + 2 * b0, Bs);
        if (rc) return rc;
    }
    // ONE host round trip: the B reductions and the B info words in one copy
    h->bat_out_host.resize(l.back_bytes);
    HIPCHK(hipMemcpyAsync(h->bat_out_host.data(), red, l.back_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const double *r = reinterpret_cast<const double *>(h->bat_out_host.data());
    batch_results(n, ncol, B, r, reinterpret_cast<const int *>(r + 2 * B), out_host, info_host);
    return 0;
}

// the value and the kernel-owned gradient at B hyperparameter vectors (grad_batch.hip): the factorisation of fvgp_hip_loglik_batch with
// every leaf inverse kept, then per problem W = L^-1 (recursive halving), b = W^T z, KV^-1 = W^T W, the fused trace and its per-problem
// reduction; one host copy of {reductions, gradients, info words} at the end
int fvgp_hip_loglik_grad_batch(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                               const double *thetas, int ntheta, int64_t B,
                               const double *vdiag, int64_t vdiag_stride, const double *ymean, int64_t ymean_stride,
                               int ncol, int component,
                               double *KV, int64_t ld, int64_t kv_stride,
                               double *work, int64_t ldw, int64_t work_stride,
                               double *out_host, double *grad_host, int *info_host,
                               double *b_out, double *diag_out) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (n > FVGP_BATCH_MAX_DIM) { fvgp_set_error("loglik_grad_batch: n exceeds FVGP_BATCH_MAX_DIM"); return -4; }
    if (!thetas) return -6;
    if (B < 1) { fvgp_set_error("loglik_grad_batch: B >= 1"); return -8; }
    KmatDesc k0d{};
    int rc = kmat_desc_from_theta(kernel_id, d, thetas, ntheta, &k0d);
    if (rc) return batch_theta_rc(rc);
    if (!vdiag) { fvgp_set_error("loglik_grad_batch needs the noise variances (vdiag)"); return -9; }
    if (vdiag_stride < 0) return -10;
    if (!ymean) return -11;
    if (ymean_stride < 0) return -12;
    if (ncol < 1 || ncol > FVGP_MAX_RHS_VEC) { fvgp_set_error("1 <= ncol <= 8"); return -13; }
    if (component < 0 || component >= ncol) { fvgp_set_error("loglik_grad_batch: 0 <= component < ncol"); return -14; }
    const int64_t dim = fvgp_hip_loglik_batch_dim(n, ncol), np = pad128(n);
    if (dim <= 0) { fvgp_set_error("loglik_grad_batch: fvgp_hip_loglik_batch_dim(n, ncol) exceeds FVGP_BATCH_MAX_DIM"); return -4; }
    if (!KV || ((uintptr_t)KV & 15)) { fvgp_set_error("loglik_grad_batch: KV must be 16-byte aligned"); return -15; }
    if (ld < dim || (ld & 1)) { fvgp_set_error("loglik_grad_batch: the leading dimension must be even and >= fvgp_hip_loglik_batch_dim(n, ncol)"); return -16; }
    if (B > 1 && (kv_stride < dim * ld || (kv_stride & 1))) { fvgp_set_error("loglik_grad_batch: kv_stride must be even and >= dim * ld"); return -17; }
    if (!work || ((uintptr_t)work & 15)) { fvgp_set_error("loglik_grad_batch: work must be 16-byte aligned"); return -18; }
    if (ldw < np || (ldw & 1)) { fvgp_set_error("loglik_grad_batch: ldw must be even and >= padded_dim(n)"); return -19; }
    if (B > 1 && (work_stride < np * ldw || (work_stride & 1))) { fvgp_set_error("loglik_grad_batch: work_stride must be even and >= padded_dim(n) * ldw"); return -20; }
    if (!out_host) return -21;
    if (!grad_host) return -22;
    HIPCHK(hipSetDevice(h->device));
    BatchWs l;
    rc = batch_workspace(h, BATCH_GRAD, n, dim, B, &l); if (rc) return rc;
    constexpr int TW = 1 + FVGP_MAX_DIM;
    const int64_t ntiles = l.ntiles, lstride = l.lstride, zstride = l.zstride, pstride = l.pstride;
    double *linv = l.linv, *logdet = l.logdet, *tab = l.tab, *zb = l.zb, *partial = l.partial, *red = l.red, *grad = l.grad;
    int *info = l.info;
    rc = batch_theta_table(h, kernel_id, d, thetas, ntheta, B, tab); if (rc) return rc;
    HIPCHK(hipMemsetAsync(info, 0, (size_t)B * sizeof(int), h->stream));
    const int kind = k0d.kind, iso = k0d.iso, nk = kernel_param_count(kernel_id, d);
    const int64_t stride = B > 1 ? kv_stride : 0, wstride = B > 1 ? work_stride : 0;
    constexpr int64_t GROUP = 65535;
    for (int64_t b0 = 0; b0 < B; b0 += GROUP) {
        const int64_t Bs = B - b0 < GROUP ? B - b0 : GROUP;
        double *K0 = KV + b0 * stride, *W0 = work + b0 * wstride, *li = linv + b0 * lstride, *z = zb + b0 * zstride;
        rc = batch_factor(h, kind, x, n, d, tab + b0 * TW, vdiag + b0 * vdiag_stride, vdiag_stride, ymean + b0 * ymean_stride, ymean_stride, ncol,
                          K0, ld, stride, dim, li, lstride, LEAF_DOUBLES, logdet + b0 * dim, info + b0, red + 2 * b0, Bs);
        if (rc) return rc;
        rc = launch_grad_init_batch(h, K0, stride, ld, n, component, li, lstride, z, zstride, Bs); if (rc) return rc;
        // W = L^-1 over the padded np x np factor, in place, by recursive halving: inv([[A,0],[C,D]]) = [[A^-1,0],[-D^-1 C A^-1, D^-1]]
        std::function<int(int64_t, int64_t)> invert = [&](int64_t J0, int64_t Jend) -> int {
            const int64_t blocks = (Jend - J0) / TILE;
            if (blocks <= 1) return 0;
            const int64_t mid = J0 + (blocks / 2) * TILE;
            int r = invert(J0, mid); if (r) return r;
            r = invert(mid, Jend); if (r) return r;
            const int64_t wa = mid - J0, wd = Jend - mid;
            double *Cb = K0 + mid * ld + J0, *XT = W0 + J0 * ldw + mid;
            // X^T = A^-1^T C^T -> work[J0:mid, mid:Jend] (A^-1 read k-major; lower: k >= row tile)
            r = launch_gemm(h, gemm_desc(1, 0, wa, wd, wa, 1.0, K0 + J0 * ld + J0, ld, Cb, ld, 0.0, XT, ldw)
                                   .k_begin(0, TILE, 0).k_end(wa).batched(Bs, stride, stride, wstride)); if (r) return r;
            // C <- -D^-1 X  (D^-1 lower: k < (row tile + 1) * 128)
            return launch_gemm(h, gemm_desc(0, 0, wd, wa, wd, -1.0, K0 + mid * ld + mid, ld, XT, ldw, 0.0, Cb, ld)
                                      .k_end(TILE, TILE, 0).batched(Bs, stride, wstride, stride));
        };
        rc = invert(0, np); if (rc) return rc;
        rc = launch_wtz_batch(h, K0, stride, ld, n, z, z + np, zstride, Bs); if (rc) return rc;
        // KV^-1 = W^T W = (W^T)(W^T)^T: W^T into work, the lower tiles of the product over W (k >= row tile)
        rc = launch_transpose_lower_batch(h, K0, stride, ld, W0, wstride, ldw, np, Bs); if (rc) return rc;
        rc = launch_gemm(h, gemm_desc(0, 0, np, np, np, 1.0, W0, ldw, W0, ldw, 0.0, K0, ld).lower_tiles()
                                .k_begin(0, TILE, 0).k_end(np).batched(Bs, wstride, wstride, stride)); if (rc) return rc;
        rc = launch_grad_trace_batch(h, kind, iso, x, n, d, K0, stride, ld, z + np, zstride, tab + b0 * TW, partial + b0 * pstride, pstride, Bs);
        if (rc) return rc;
        rc = launch_grad_reduce_batch(h, partial + b0 * pstride, pstride, ntiles, nk, grad + b0 * TW, Bs); if (rc) return rc;
        if (b_out || diag_out) {
            rc = launch_grad_outputs_batch(h, z + np, zstride, K0, stride, ld, n, b_out ? b_out + b0 * n : nullptr, diag_out ? diag_out + b0 * n : nullptr, Bs);
            if (rc) return rc;
        }
    }
    // ONE host round trip: reductions, gradients and info words in one copy
    h->bat_out_host.resize(l.back_bytes);
    HIPCHK(hipMemcpyAsync(h->bat_out_host.data(), red, l.back_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const double *r = reinterpret_cast<const double *>(h->bat_out_host.data()), *g = r + 2 * B;
    const int *inf = reinterpret_cast<const int *>(g + B * TW);
    batch_results(n, ncol, B, r, inf, out_host, info_host);
    for (int64_t b = 0; b < B; ++b) {
        const bool bad = inf[b] != 0 && inf[b] <= n;
        for (int i = 0; i < ntheta; ++i) grad_host[b * ntheta + i] = bad ? NAN : (i < nk ? g[b * TW + i] : 0.0);
    }
    return 0;
}

// the posterior mean, variance and covariance at B hyperparameter vectors (posterior_batch.hip): the factorisation of fvgp_hip_loglik_batch
// (the same launches on the same data for the top squares, every leaf inverse kept) with one chunk of prediction rows k(x*, x; theta_b)
// under each square, which leaves it as V^T; an epilogue per chunk; further chunks by a solve-only pass; S from one strided-batch GEMM
int fvgp_hip_posterior_batch(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                             const double *thetas, int ntheta, int64_t B,
                             const double *vdiag, int64_t vdiag_stride, const double *ymean, int64_t ymean_stride, int ncol,
                             const double *xpred, int64_t P,
                             double *KV, int64_t kv_rows, int64_t ld, int64_t kv_stride,
                             double *mean_out, double *var_out, double *S_out, int64_t lds, int64_t s_stride,
                             double *out_host, int *info_host) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (n > FVGP_BATCH_MAX_DIM) { fvgp_set_error("posterior_batch: n exceeds FVGP_BATCH_MAX_DIM"); return -4; }
    if (!thetas) return -6;
    if (B < 1) { fvgp_set_error("posterior_batch: B >= 1"); return -8; }
    KmatDesc k0d{};
    int rc = kmat_desc_from_theta(kernel_id, d, thetas, ntheta, &k0d);
    if (rc) return batch_theta_rc(rc);
    if (!vdiag) { fvgp_set_error("posterior_batch needs the noise variances (vdiag)"); return -9; }
    if (vdiag_stride < 0) return -10;
    if (!ymean) return -11;
    if (ymean_stride < 0) return -12;
    if (ncol < 1 || ncol > FVGP_MAX_RHS_VEC) { fvgp_set_error("1 <= ncol <= 8"); return -13; }
    const int64_t dim = fvgp_hip_loglik_batch_dim(n, ncol), np = pad128(n);
    if (dim <= 0) { fvgp_set_error("posterior_batch: fvgp_hip_loglik_batch_dim(n, ncol) exceeds FVGP_BATCH_MAX_DIM"); return -4; }
    if (!xpred) { fvgp_set_error("posterior_batch needs the prediction points (xpred)"); return -14; }
    if (P < 1) { fvgp_set_error("posterior_batch: P >= 1"); return -15; }
    if (!KV || ((uintptr_t)KV & 15)) { fvgp_set_error("posterior_batch: KV must be 16-byte aligned"); return -16; }
    const int64_t P_chunk = kv_rows - dim;
    if (P_chunk < TILE || P_chunk % TILE) {
        fvgp_set_error("posterior_batch: kv_rows must be fvgp_hip_loglik_batch_dim(n, ncol) plus a multiple of 128 (>= 128) prediction rows"); return -17;
    }
    if (ld < dim || (ld & 1)) { fvgp_set_error("posterior_batch: the leading dimension must be even and >= fvgp_hip_loglik_batch_dim(n, ncol)"); return -18; }
    if (B > 1 && (kv_stride < kv_rows * ld || (kv_stride & 1))) { fvgp_set_error("posterior_batch: kv_stride must be even and >= kv_rows * ld"); return -19; }
    if (!mean_out) { fvgp_set_error("posterior_batch needs mean_out"); return -20; }
    const int64_t Pp = pad128(P);
    if (S_out) {
        if (P > P_chunk) { fvgp_set_error("posterior_batch: S_out needs all prediction points in one chunk (P <= kv_rows - dim)"); return -22; }
        if ((uintptr_t)S_out & 15) { fvgp_set_error("posterior_batch: S_out must be 16-byte aligned"); return -22; }
        if (lds < Pp || (lds & 1)) { fvgp_set_error("posterior_batch: lds must be even and >= padded_dim(P)"); return -23; }
        if (B > 1 && (s_stride < Pp * lds || (s_stride & 1))) { fvgp_set_error("posterior_batch: s_stride must be even and >= padded_dim(P) * lds"); return -24; }
    }
    HIPCHK(hipSetDevice(h->device));
    BatchWs l;
    rc = batch_workspace(h, BATCH_POSTERIOR, n, dim, B, &l); if (rc) return rc;
    constexpr int TW = 1 + FVGP_MAX_DIM;
    const int64_t lstride = l.lstride;
    double *linv = l.linv, *logdet = l.logdet, *tab = l.tab, *red = l.red;
    int *info = l.info;
    rc = batch_theta_table(h, kernel_id, d, thetas, ntheta, B, tab); if (rc) return rc;
    HIPCHK(hipMemsetAsync(info, 0, (size_t)B * sizeof(int), h->stream));
    const int kind = k0d.kind;
    const int64_t stride = B > 1 ? kv_stride : 0, sstride = B > 1 ? s_stride : 0;
    constexpr int64_t GROUP = 65535;
    for (int64_t b0 = 0; b0 < B; b0 += GROUP) {
        const int64_t Bs = B - b0 < GROUP ? B - b0 : GROUP;
        double *K0 = KV + b0 * stride, *li = linv + b0 * lstride;
        const double *tb = tab + b0 * TW;
        rc = launch_kmat_batch(h, kind, x, n, d, tb, vdiag + b0 * vdiag_stride, vdiag_stride, K0, ld, stride, dim, Bs); if (rc) return rc;
        rc = launch_rhs_rows_batch(h, K0, stride, n, ld, ymean + b0 * ymean_stride, ymean_stride, ncol, vdiag + b0 * vdiag_stride, vdiag_stride, Bs);
        if (rc) return rc;
        for (int64_t p0 = 0; p0 < P; p0 += P_chunk) {
            const int64_t pc = P - p0 < P_chunk ? P - p0 : P_chunk, prow = pad128(pc);
            // the chunk's rows: k(x*_p, x_j; theta_b) for j < n, zeros in the columns n .. dim - 1 and in the rows past the last point
            rc = launch_cross_batch(h, kind, xpred + p0 * d, pc, x, n, d, tb, K0 + dim * ld, ld, stride, prow, dim, 0, Bs); if (rc) return rc;
            rc = batch_recursion(h, n, K0, ld, stride, dim, dim + prow, li, lstride, LEAF_DOUBLES, logdet + b0 * dim, info + b0, Bs, p0 > 0);
            if (rc) return rc;
            if (p0 == 0) { rc = launch_loglik_tail_batch(h, logdet + b0 * dim, dim, K0, stride, ld, n, ncol, red + 2 * b0, Bs); if (rc) return rc; }
            rc = launch_post_epilogue_batch(h, kind, K0, stride, ld, n, dim, ncol, info + b0, tb, mean_out + b0 * P * ncol,
                                            var_out ? var_out + b0 * P : nullptr, P, p0, pc, Bs);
            if (rc) return rc;
        }
        if (S_out) {
            // S = k(x*, x*) - V^T-rows V^T-rows^T on the lower tiles: K ends at padded n, where the epilogue has zeroed the columns from
            // n on (the appended-rows columns do not enter); explicit K range: the 128-tile kernel whatever Bs and P are
            double *S0 = S_out + b0 * sstride;
            rc = launch_cross_batch(h, kind, xpred, P, xpred, P, d, tb, S0, lds, sstride, Pp, Pp, 1, Bs); if (rc) return rc;
            const double *VT = K0 + dim * ld;
            rc = launch_gemm(h, gemm_desc(0, 0, Pp, Pp, np, -1.0, VT, ld, VT, ld, 1.0, S0, lds).lower_tiles()
                                    .k_end(np).batched(Bs, stride, stride, sstride)); if (rc) return rc;
            rc = launch_s_finish_batch(h, S0, sstride, lds, Pp, info + b0, n, Bs); if (rc) return rc;
        }
    }
    // ONE host round trip: the B reductions and the B info words in one copy
    h->bat_out_host.resize(l.back_bytes);
    HIPCHK(hipMemcpyAsync(h->bat_out_host.data(), red, l.back_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const double *r = reinterpret_cast<const double *>(h->bat_out_host.data());
    const int *inf = reinterpret_cast<const int *>(r + 2 * B);
    if (out_host) batch_results(n, ncol, B, r, inf, out_host, info_host);
    else if (info_host) for (int64_t b = 0; b < B; ++b) info_host[b] = inf[b] > n ? 0 : inf[b];
    return 0;
}

}  // extern "C"
