// Host side of the C ABI: the fused single evaluations -- log-likelihood, its gradient (POTRI + fused trace) and the posterior.
#include "common.h"
#include "kernel_family.h"
#include <math.h>

// g_i = 1/2 sum_jk (W_jk - b_j b_k) dK_jk/dtheta_i over the lower triangle of the symmetric W (b may be null):
// one fused pass that re-evaluates dK/dtheta in registers, per-tile partial sums reduced on the host in a fixed order
static int grad_trace_host(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
                           const double *W, int64_t ldw, const double *b, int64_t ldb, double *partial, double *grad_host,
                           int64_t col0 = 0, int64_t ncols = 0) {
    GradDesc g{};
    g.col0 = col0; g.ncols = ncols;
    int rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &g.k); if (rc) return rc;
    g.k.x1 = x; g.k.n1 = n; g.k.x2 = x; g.k.n2 = n;
    const int nk = kernel_param_count(kernel_id, d);     // kernel-owned hyperparameters; the rest get a zero gradient
    g.ntheta = nk;
    g.W = W; g.ldw = ldw; g.b = b; g.ldb = ldb;
    g.partial = partial;
    int nblocks = 0;
    rc = launch_grad_trace(h, g, &nblocks); if (rc) return rc;
    // nblocks <= ~80k doubles per theta
    std::vector<double> part((size_t)nblocks * nk);
    HIPCHK(hipMemcpyAsync(part.data(), partial, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < ntheta; ++i) grad_host[i] = 0.0;
    for (int i = 0; i < nk; ++i) {
        long double s = 0.0L;
        for (int bb = 0; bb < nblocks; ++bb) s += part[(size_t)bb * nk + i];
        grad_host[i] = 0.5 * (double)s;
    }
    return 0;
}

extern "C" {

int fvgp_hip_loglik(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                    const double *theta, int ntheta, const double *vdiag, const double *ymean, int ncol,
                    double *KV, int64_t ld, double *alpha, double *out_host, int *info_host) {
    // the contract of this entry: KV holds padded_dim(n) rows, whatever its leading dimension; nothing below them is touched
    const int rc = fvgp_hip_loglik_rows(h, kernel_id, x, n, d, theta, ntheta, vdiag, ymean, ncol, KV, pad128(n), ld, alpha, out_host, info_host);
    return rc <= -13 && rc > -100 ? rc + 1 : rc;        // argument numbers of THIS signature (kv_rows is argument 12 there)
}

int fvgp_hip_loglik_rows(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                         const double *theta, int ntheta, const double *vdiag, const double *ymean, int ncol,
                         double *KV, int64_t kv_rows, int64_t ld, double *alpha, double *out_host, int *info_host) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (!theta) return -6;
    if (!vdiag) { fvgp_set_error("loglik needs the noise variances (vdiag)"); return -8; }
    if (!ymean) return -9;
    if (ncol < 1 || ncol > FVGP_MAX_RHS_VEC) { fvgp_set_error("1 <= ncol <= 8"); return -10; }
    int rc = check_square(KV, n, ld, 11, 4, 13);
    if (rc) return rc;
    if (kv_rows < pad128(n)) { fvgp_set_error("loglik: the scratch needs at least padded_dim(n) rows"); return -12; }
    if (!out_host) return -15;
    HIPCHK(hipSetDevice(h->device));
    const int64_t np = pad128(n);
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    k.x1 = x; k.n1 = n; k.x2 = x; k.n2 = n; k.vdiag = vdiag; k.K = KV; k.ldk = ld; k.uplo = FVGP_LOWER; k.pad = 1;
    if (h->profile) {
        for (auto &e : h->ev_stage) if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(h->ev_stage[0], h->stream));
    }
    rc = launch_kmat(h, k); if (rc) return rc;
    if (h->profile) HIPCHK(hipEventRecord(h->ev_stage[1], h->stream));
    // forward solve fused into the factorisation: (y-m)^T is appended as rows n..n+ncol-1 of the padded
    // matrix (diagonal entry large enough to keep the block PD); the panel TRSM / trailing updates then
    // leave z^T = (L^-1 (y-m))^T in those rows and quad = |z|^2.  Needs ncol free padding rows: where padded_dim(n) leaves
    // fewer (n a multiple of 128), the rows go into one more block row -- if the caller SAYS its scratch has it
    // (kv_rows and ld >= fvgp_hip_loglik_dim(n, ncol); never inferred from the leading dimension: a pitched buffer or a row slice
    // of a larger arena holds padded_dim(n) rows only); else the forward solve is a sweep of its own after the factorisation.
    const bool room = (np - n) >= ncol;
    const int64_t npf = room ? np : pad128(n + ncol);
    const bool fused = room || (kv_rows >= npf && ld >= npf);
    if (fused) {
        if (npf > np) { rc = launch_pad_identity(h, KV, np, npf, ld); if (rc) return rc; }
        rc = launch_rhs_rows(h, KV, n, ld, ymean, ncol, vdiag); if (rc) return rc;
    }
    // ONE host round trip per evaluation: the factorisation is only enqueued, its info word comes back with the scalars at the end
    // (what follows a failed factorisation computes on garbage and is thrown away; the profile option times the factorisation with
    // events and keeps the round trip in the middle)
    int info = 0;
    const bool defer = !h->profile;
    const int64_t npd = fused ? npf : 0;
    const bool own_inverses = fused && (h->leaf_tiles || h->panel_chain);      // (see below: the block inverses wait until the appended rows are out again)
    if (defer) { rc = potrf_driver(h, KV, n, ld, nullptr, nullptr, true, npd, own_inverses); if (rc) return rc; }
    else {
        rc = potrf_driver(h, KV, n, ld, &info, nullptr, false, npd, own_inverses); if (rc) return rc;
        if (info_host) *info_host = info;
        if (info != 0) { out_host[0] = out_host[1] = out_host[2] = NAN; return 0; }
    }
    if (h->profile) HIPCHK(hipEventRecord(h->ev_stage[2], h->stream));
    if (fused) {
        // ONE launch: sum log L_ii from the leaves' 1 / L_ii (1 on padding rows), |z|^2 of the appended rows, z (rows of L) -> the
        // (np x C) vector layout of the backward sweep, alpha <- 0
        const int C = ncol <= 1 ? 1 : ncol <= 2 ? 2 : ncol <= 4 ? 4 : 8;
        if (alpha) { rc = ensure_scratch(h, np); if (rc) return rc; }
        rc = launch_loglik_tail(h, h->logdet_parts, npf, KV, ld, n, ncol, h->red, alpha ? h->vec : nullptr, C, np, alpha); if (rc) return rc;
        // hand back the clean factor of blockdiag(K+V, I): identity padding rows again; the 128 x 128 block inverses the sweeps, the
        // posterior and POTRI take are computed from THAT (one batched launch; the last diagonal block without the appended rows)
        rc = launch_pad_identity(h, KV, n, npf, ld); if (rc) return rc;
        if (own_inverses) {
            rc = launch_leaf_inverse_batched(h, KV, ld, npf / TILE, h->linv); if (rc) return rc;
            h->linv_L = KV; h->linv_n = n; h->linv_ld = ld;
        } else if (room) {
            rc = launch_leaf(h, KV + (np - TILE) * ld + (np - TILE), ld, h->linv + (np / TILE - 1) * LEAF_DOUBLES, nullptr, 0, 0, TILE);
            if (rc) return rc;
        }
        if (alpha) {
            if (h->bwd_sweep && ncol == 1) { rc = launch_bwd_sweep(h, KV, ld, np, h->linv, h->vec, alpha, ncol, ncol); if (rc) return rc; }
            else
            for (int64_t k0 = np - TILE; k0 >= 0; k0 -= TILE) {
                rc = launch_bwd_step(h, KV, ld, np, k0, h->linv + (k0 / TILE) * LEAF_DOUBLES, h->vec, alpha, ncol, ncol);
                if (rc) return rc;
            }
        }
    } else {
        rc = launch_neg_log_sum(h, h->logdet_parts, np, h->red); if (rc) return rc;
        if (!alpha) { fvgp_set_error("loglik without alpha needs ncol free padding rows (n % 128 <= 128 - ncol) or a scratch of fvgp_hip_loglik_dim(n, ncol) rows"); return -14; }
        rc = launch_copy_cols(h, ymean, ncol, alpha, ncol, n, ncol, np, ncol); if (rc) return rc;
        rc = potrs_vec(h, KV, n, ld, alpha, ncol, ncol, true); if (rc) return rc;
        rc = launch_dot_rows(h, ymean, ncol, alpha, ncol, n, ncol, h->red + 1); if (rc) return rc;
    }
    if (h->profile) HIPCHK(hipEventRecord(h->ev_stage[3], h->stream));
    double r[2];
    int *hinfo = reinterpret_cast<int *>(h->hpin + RED_SLOTS - 2);
    if (defer) HIPCHK(hipMemcpyAsync(hinfo, h->dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    rc = fvgp_read_back(h, h->red, r, 2); if (rc) return rc;
    if (defer) {
        info = *hinfo;
        if (info == 0x7fffffff) { fvgp_set_error("panel chain: a workgroup waited longer than 3 s for a hand-off and the launch was abandoned"); return 1999; }
        if (info > n) info = 0;   // cannot happen: the padding is an identity block
        if (info_host) *info_host = info;
        if (info != 0) { out_host[0] = out_host[1] = out_host[2] = NAN; return 0; }
    }
    if (h->profile) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev_stage[0], h->ev_stage[1])); h->prof_kmat_ms = ms;
        HIPCHK(hipEventElapsedTime(&ms, h->ev_stage[2], h->ev_stage[3])); h->prof_tail_ms = ms;
        // lower 128-tiles written once (+ the padded diagonal), x read once
        const double tiles = (double)(np / TILE) * (double)(np / TILE + 1) * 0.5;
        h->prof_kmat_bytes = tiles * TILE * TILE * 8.0 + (double)n * d * 8.0;
    }
    const double logdet = 2.0 * r[0], quad = r[1] / (double)ncol;
    out_host[0] = -0.5 * (quad + logdet + (double)n * log(2.0 * M_PI));
    out_host[1] = logdet;
    out_host[2] = quad;
    return 0;
}

int fvgp_hip_loglik_grad(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                         const double *theta, int ntheta, const double *alpha, int ncol, int component,
                         double *KV, int64_t ld, double *work, int64_t ldw, double *grad_host) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (!theta) return -6;
    if (!alpha) return -8;
    if (ncol < 1) return -9;
    if (component < 0 || component >= ncol) return -10;
    if (!grad_host) return -15;
    HIPCHK(hipSetDevice(h->device));
    int rc = fvgp_hip_potri(h, KV, n, ld, work, ldw);
    if (rc) return rc;
    // inv(L) in `work` is dead by now: reuse it as the partial-sum buffer
    return grad_trace_host(h, kernel_id, x, n, d, theta, ntheta, KV, ld, alpha + component, ncol, work, grad_host);
}

int fvgp_hip_grad_trace(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                        const double *theta, int ntheta, const double *W, int64_t ldw,
                        const double *b, int64_t ldb, double *partial, double *grad_host) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (!theta) return -6;
    if (!W) return -8;
    // a wave loads whole 128-column tile rows of W before it tests the column: every row must own its tile columns
    if (ldw < pad128(n) || (ldw & 1) || ((uintptr_t)W & 15)) { fvgp_set_error("grad_trace needs ldw >= padded_dim(n), even, 16-byte aligned W"); return -9; }
    if (b && ldb < 1) return -11;
    if (!partial) return -12;
    if (!grad_host) return -13;
    HIPCHK(hipSetDevice(h->device));
    return grad_trace_host(h, kernel_id, x, n, d, theta, ntheta, W, ldw, b, ldb, partial, grad_host);
}

int fvgp_hip_grad_trace_cols(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                             const double *theta, int ntheta, const double *W, int64_t ldw, int64_t col0, int64_t ncols,
                             const double *b, int64_t ldb, double *partial, double *grad_host) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (!theta) return -6;
    if (!W) return -8;
    if (col0 < 0 || col0 % TILE || col0 >= n) return -10;
    if (ncols <= 0) return -11;
    if (ldw < pad128(ncols) || (ldw & 1) || ((uintptr_t)W & 15)) { fvgp_set_error("grad_trace_cols needs ldw >= 128 * ceil(ncols / 128), even, 16-byte aligned W"); return -9; }
    if (b && ldb < 1) return -13;
    if (!partial) return -14;
    if (!grad_host) return -15;
    HIPCHK(hipSetDevice(h->device));
    return grad_trace_host(h, kernel_id, x, n, d, theta, ntheta, W, ldw, b, ldb, partial, grad_host, col0, ncols);
}

int fvgp_hip_posterior_prepare(fvgp_handle *h, const double *L, int64_t n, int64_t ldl) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (!h->block_inverses || pad128(n) < 2 * TILE) return 0;
    // what the first fvgp_hip_posterior on this factor would build before its sweep: the inverted diagonal blocks at the width a call
    // with up to 1024 points takes (enqueue only)
    return ensure_winv(h, L, n, ldl, h->posterior_block, h->posterior_block);
}

int fvgp_hip_posterior(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                       const double *theta, int ntheta, const double *L, int64_t ldl,
                       const double *alpha, int ncol, const double *xpred, int64_t P,
                       double *kx, int64_t ldk, double *mean_out, double *var_out, double *S_out, int64_t lds) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (!theta) return -6;
    int rc = check_square(L, n, ldl, 8, 4, 9);
    if (rc) return rc;
    if (!alpha) return -10;
    if (ncol < 1 || ncol > 128) return -11;
    if (!xpred) return -12;
    if (P <= 0) return -13;
    const int64_t np = pad128(n), Pp = pad128(P);
    if (!kx || ((uintptr_t)kx & 15)) return -14;
    if (ldk < Pp || (ldk & 1)) return -15;
    if (S_out && (lds < Pp || (lds & 1) || ((uintptr_t)S_out & 15))) return -19;
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    if (P == 1 && h->fwd_sweep && ncol <= FVGP_MAX_RHS_VEC) {
        // ---- ONE prediction point (gradient-based acquisition optimisers ask for one at a time): the cross covariance is a
        //      column, L^-1 k the one-launch forward sweep (N = 20k: 1.1 ms against 1.7 ms of the block sweep below, and no
        //      inverted blocks to build after a new factor); fixed-order sums throughout
        k.x1 = x; k.n1 = n; k.x2 = xpred; k.n2 = 1; k.vdiag = nullptr; k.K = kx; k.ldk = ldk; k.uplo = FVGP_FULL; k.pad = 2;
        rc = launch_kmat(h, k); if (rc) return rc;
        if (mean_out)
            for (int cc = 0; cc < ncol; ++cc) { rc = launch_dot_rows(h, kx, ldk, alpha + cc, ncol, n, 1, mean_out + cc); if (rc) return rc; }
        if (var_out || S_out) {
            rc = ensure_linv(h, L, n, ldl); if (rc) return rc;
            rc = ensure_scratch(h, np / 8 + 16); if (rc) return rc;
            rc = launch_fwd_sweep(h, L, ldl, np, h->linv, kx, ldk, h->vec); if (rc) return rc;          // h->vec <- L^-1 k
            if (var_out) { rc = launch_rows_sumsq_base(h, h->vec, np, np, 1, k.sig, var_out); if (rc) return rc; }      // sigma^2 - |L^-1 k|^2
            if (S_out) {
                KmatDesc kk = k;
                kk.x1 = xpred; kk.n1 = 1; kk.x2 = xpred; kk.n2 = 1; kk.K = S_out; kk.ldk = lds; kk.uplo = FVGP_FULL; kk.pad = 2;
                rc = launch_kmat(h, kk); if (rc) return rc;
                rc = launch_rows_sumsq_base(h, h->vec, np, np, 1, 0.0, h->red + 4); if (rc) return rc;       // -|L^-1 k|^2
                rc = launch_add_matrix(h, S_out, lds, h->red + 4, 1, 1, 1, 1.0); if (rc) return rc;
            }
        }
        return 0;
    }
    // ---- every product runs on the TRANSPOSED cross covariance k(x_pred, x_data), Pp x np with leading dimension np
    //      in the caller's scratch: the substitution then runs on the factorisation's own (M,K) x (N,K) kernels
    //      (trsm_fwd_gemm_t) and S -= V^T V is A A^T of contiguous rows.  Also for a handful of points: the sweep over
    //      2048-blocks is ten dependent steps at N = 20k, 1.7 ms whatever P <= 64, where per-block vector launches took
    //      4.6 / 9.0 ms at P = 2 / 4
    double *KT = kx;
    k.x1 = xpred; k.n1 = P; k.x2 = x; k.n2 = n; k.vdiag = nullptr; k.K = KT; k.ldk = np; k.uplo = FVGP_FULL; k.pad = 2;
    rc = launch_kmat(h, k); if (rc) return rc;
    if (mean_out && ncol <= FVGP_MAX_RHS_VEC) {
        rc = launch_rows_dot(h, KT, np, alpha, ncol, ncol, n, P, mean_out, ncol); if (rc) return rc;
    } else if (mean_out) {
        // many columns of y: GEMM with alpha widened to 128 columns in the handle scratch;
        // the (Pp x 128) result goes to the tail of the same scratch
        rc = ensure_scratch(h, np * 16 + Pp * 16); if (rc) return rc;
        double *aw = h->vec;
        rc = launch_copy_cols(h, alpha, ncol, aw, 128, np, ncol, np, 128); if (rc) return rc;
        double *mw = h->vec + np * 128;
        rc = launch_gemm(h, gemm_desc(0, 1, Pp, 128, np, 1.0, KT, np, aw, 128, 0.0, mw, 128)); if (rc) return rc;      // mean (widened) = KT alpha
        rc = launch_copy_cols(h, mw, 128, mean_out, ncol, P, ncol, P, ncol); if (rc) return rc;
    }
    if (var_out || S_out) {
        rc = trsm_fwd_gemm_t(h, L, n, ldl, KT, Pp, np); if (rc) return rc;             // KT <- (L^-1 k)^T
        if (S_out) {
            KmatDesc kk = k;
            kk.x1 = xpred; kk.n1 = P; kk.x2 = xpred; kk.n2 = P; kk.K = S_out; kk.ldk = lds; kk.uplo = FVGP_FULL; kk.pad = 2;
            rc = launch_kmat(h, kk); if (rc) return rc;
            // S -= V^T V = KT KT^T on the 128-tiles on and below the block diagonal only (S is symmetric: 36 of 64 tiles at
            // 1024 points), the rest mirrored; few output tiles and K = np: split K so that the launch fills the chip once
            GemmDesc g = gemm_desc(0, 0, Pp, Pp, np, -1.0, KT, np, KT, np, 1.0, S_out, lds).lower_tiles();
            const int64_t tr = Pp / TILE, tiles = tr * (tr + 1) / 2;
            // an XCD (64 workgroup slots) gets ceil(tiles / 8) tiles of every K slice: 36 tiles -> 5 -> 12 slices, not 14
            int64_t split = tiles >= 512 ? 1 : 64 / ((tiles + 7) / 8);
            const int64_t max_split = np / 512 > 0 ? np / 512 : 1;       // at least 512 of K per workgroup
            if (tiles >= 512) {
                // more tiles than slots: unsplit, 528 tiles (4096 points) take TWO rounds of 512 for 1.03 rounds of work; s slices per
                // tile take ceil(tiles s / 512) / s rounds -- the smallest s <= 8 that brings that within 15 % of the work
                double best = (double)((tiles + 511) / 512);
                for (int64_t sp = 2; sp <= 8 && sp <= max_split; ++sp) {
                    const double rounds = (double)((tiles * sp + 511) / 512) / (double)sp;
                    if (rounds < best * 0.97) { best = rounds; split = sp; }
                    if (best <= 1.15 * (double)tiles / 512.0) break;
                }
            }
            if (split > max_split) split = max_split;
            if (split > 1) {
                rc = ensure_scratch(h, (split * Pp * Pp + 7) / 8); if (rc) return rc;
                g.split = (int)split; g.split_ws = h->vec;
            }
            rc = launch_gemm(h, g); if (rc) return rc;
            rc = launch_transpose_lower_tiles(h, S_out, lds, S_out, lds, Pp); if (rc) return rc;
        }
        if (var_out) {
            // v_p = k(x_p,x_p) - |L^-1 k_p|^2 ; stationary kernels: k(x,x) = signal variance
            rc = launch_rows_sumsq_base(h, KT, np, np, P, k.sig, var_out); if (rc) return rc;
        }
    }
    return 0;
}

}  // extern "C"
