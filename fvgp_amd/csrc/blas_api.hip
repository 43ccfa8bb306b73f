// Host side of the C ABI: thin entries over one launch or a few -- covariance assembly, BLAS-like products, reductions, diagnostics.
#include "common.h"

extern "C" {

int fvgp_hip_kmat(fvgp_handle *h, int kernel_id, const double *x1, int64_t n1, const double *x2, int64_t n2,
                  int d, const double *theta, int ntheta, const double *vdiag, double *K, int64_t ldk, int uplo, int pad) {
    if (!h) return -1;
    if (!x1) return -3;
    if (n1 <= 0) return -4;
    if (!x2) return -5;
    if (n2 <= 0) return -6;
    if (!theta) return -8;
    if (!K) return -11;
    if (ldk < (pad ? pad128(n2) : n2)) { fvgp_set_error("ldk too small"); return -12; }
    if (uplo != FVGP_FULL && uplo != FVGP_LOWER) return -13;
    if (pad < 0 || pad > 2) return -14;
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    int rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k);
    if (rc) return rc;
    k.x1 = x1; k.n1 = n1; k.x2 = x2; k.n2 = n2; k.vdiag = vdiag; k.K = K; k.ldk = ldk; k.uplo = uplo; k.pad = pad;
    return launch_kmat(h, k);
}

int fvgp_hip_syrk_rowshard(fvgp_handle *h, int64_t M, int64_t N, int64_t K, const double *A, int64_t lda,
                            const double *B, int64_t ldb, double *C, int64_t ldc, int scale, int off,
                            int b_ranks, int b_blocks, int b_off) {
    if (!h) return -1;
    if (!A) return -5;
    if (!B) return -7;
    if (!C) return -9;
    if (scale < 1) return -11;
    if (b_ranks < 1) return -13;
    if (b_off < 0 || (b_ranks > 1 && b_blocks < 1)) return -14;
    if (b_blocks > 0 && N > 0 && (b_off + N / TILE - 1) / b_ranks >= b_blocks) {
        fvgp_set_error("syrk_rowshard: the tile columns run past the gathered blocks"); return -14;
    }
    HIPCHK(hipSetDevice(h->device));
    // C -= A B^T on the tiles with tj <= ti * scale + off, B as the all-gather left it
    GemmDesc g = gemm_desc(0, 0, M, N, K, -1.0, A, lda, B, ldb, 1.0, C, ldc).lower_rowshard(scale, off).with_role(1);
    g.bc_ranks = b_ranks; g.bc_blocks = b_blocks; g.bc_off = b_off;
    // only launches of the kernel the roofline names are timed, and no more than 8192 of them between two get_profile calls
    if (!h->profile || gemm_takes_small_tiles(h, g) || h->rs_used >= 2 * 8192) return launch_gemm(h, g);
    // timed with events on the launch stream; algorithmic flops = the tiles with tj <= ti * scale + off
    while (h->rs_ev.size() < h->rs_used + 2) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); h->rs_ev.push_back(e); }
    double tiles = 0.0;
    for (int64_t ti = 0; ti < M / TILE; ++ti) {
        int64_t wdt = ti * scale + off + 1;
        if (wdt > N / TILE) wdt = N / TILE;
        if (wdt > 0) tiles += (double)wdt;
    }
    HIPCHK(hipEventRecord(h->rs_ev[h->rs_used], h->stream));
    int rc = launch_gemm(h, g);
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->rs_ev[h->rs_used + 1], h->stream));
    h->rs_used += 2;
    h->rs_flops.push_back(tiles * 128.0 * 128.0 * 2.0 * (double)K);
    return 0;
}

int fvgp_hip_panel_trsm(fvgp_handle *h, const double *D, int64_t nd, int64_t ldd, double *P, int64_t rows, int64_t ldp) {
    if (!h) return -1;
    int rc = check_square(D, nd, ldd, 2, 3, 4);
    if (rc) return rc;
    if (nd % TILE) { fvgp_set_error("panel_trsm: the diagonal block must be a multiple of 128"); return -3; }
    if (!P) return -5;
    if (rows < 0 || rows % TILE) return -6;
    if (ldp < nd || (ldp & 1) || ((uintptr_t)P & 15)) return -7;
    if (rows == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    rc = ensure_linv(h, D, nd, ldd); if (rc) return rc;
    // X = P * L^-T by 128-column blocks:  X_k = (P_k - sum_{j<k} X_j L_kj^T) * inv(L_kk)^T
    for (int64_t k0 = 0; k0 < nd; k0 += TILE) {
        if (k0 > 0) {      // P_k -= sum_{j<k} X_j L_kj^T
            rc = launch_gemm(h, gemm_desc(0, 0, rows, TILE, k0, -1.0, P, ldp, D + k0 * ldd, ldd, 1.0, P + k0, ldp)); if (rc) return rc;
        }
        // X_k = P_k inv(L_kk)^T, in place
        rc = launch_gemm(h, gemm_desc(0, 0, rows, TILE, TILE, 1.0, P + k0, ldp, h->linv + (k0 / TILE) * LEAF_DOUBLES, TILE, 0.0, P + k0, ldp)); if (rc) return rc;
    }
    return 0;
}

int fvgp_hip_gemm(fvgp_handle *h, int a_kmajor, int b_nmajor, int lower, int64_t M, int64_t N, int64_t K,
                  double alpha, const double *A, int64_t lda, const double *B, int64_t ldb,
                  double beta, double *C, int64_t ldc) {
    if (!h) return -1;
    if (!A) return -9;
    if (!B) return -11;
    if (!C) return -14;
    HIPCHK(hipSetDevice(h->device));
    GemmDesc g = gemm_desc(a_kmajor, b_nmajor, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
    // any non-zero `lower` is the lower-tile form (the header's contract); GemmDesc's lower == 2, the row-sharded predicate with its
    // scale and offset, is fvgp_hip_syrk_rowshard's and never comes through here
    if (lower) g.lower_tiles();
    // few output tiles and a long K (the Schur complement of an append, c - v^T v with K = N: ONE tile walking 4096 of K took
    // 564 us; k^T KV^-1 k of the callables' posterior): K split over workgroups, partials added in a fixed order (handle scratch).
    // An XCD (64 slots) gets ceil(tiles / 8) tiles of every slice; at least 256 of K per slice.
    if (K >= 1024 && M > 0 && N > 0 && M % TILE == 0 && N % TILE == 0 && !(ldc & 1) && !((uintptr_t)C & 15)) {      // (shorter K: the small-tile kernels)
        const int64_t tm = M / TILE, tn = N / TILE, tiles = lower ? tm * (tm + 1) / 2 : tm * tn;
        int64_t split = tiles >= 256 ? 1 : 64 / ((tiles + 7) / 8);
        if (split > K / 256) split = K / 256;
        if (split > 1) {
            int rc = ensure_scratch(h, (split * M * N + 7) / 8); if (rc) return rc;
            g.split = (int)split; g.split_ws = h->vec;
        }
    }
    return launch_gemm(h, g);
}

int fvgp_hip_mfma_selftest(fvgp_handle *h, const double *A, const double *B, double *D) {
    if (!h) return -1;
    HIPCHK(hipSetDevice(h->device));
    return launch_mfma_selftest(h, A, B, D);
}

int64_t fvgp_hip_debug_tile_map(int tiles_m, int tiles_n, int lower, int scale, int off, int *out_ti, int *out_tj, int64_t cap) {
    if (tiles_m < 1 || tiles_n < 1 || !out_ti || !out_tj) return -1;
    if (lower < 0 || lower > 2 || (lower == 2 && scale < 1)) return -3;
    return gemm_debug_tile_map(tiles_m, tiles_n, lower, scale, off, out_ti, out_tj, cap);
}

int64_t fvgp_hip_debug_tile_table(int tiles_m, int tiles_n, int lower, int scale, int off, int *out, int64_t cap) {
    if (tiles_m < 1 || tiles_n < 1 || tiles_m >= 32768 || tiles_n >= 32768 || !out) return -1;
    if (lower < 0 || lower > 2 || (lower == 2 && scale < 1)) return -3;
    return gemm_debug_tile_table(tiles_m, tiles_n, lower, scale, off, out, cap);
}

int fvgp_hip_mfma_peak(fvgp_handle *h, double *out, int blocks, int iters) {
    if (!h) return -1;
    if (!out) return -2;
    if (blocks < 1 || iters < 1) return -3;
    HIPCHK(hipSetDevice(h->device));
    return launch_mfma_peak(h, out, blocks, iters);
}

int fvgp_hip_add_lower(fvgp_handle *h, double *A, int64_t n, int64_t lda, const double *B, int64_t ldb, double alpha) {
    if (!h) return -1;
    if (!A) return -2;
    if (n <= 0) return -3;
    if (lda < n) return -4;
    if (!B) return -5;
    if (ldb < n) return -6;
    HIPCHK(hipSetDevice(h->device));
    return launch_add_lower(h, A, lda, B, ldb, n, alpha);
}

int fvgp_hip_trace_dot(fvgp_handle *h, const double *W, int64_t ldw, const double *D, int64_t ldd, const double *b, int64_t ldb,
                       int64_t n, double *out_host) {
    if (!h) return -1;
    if (!W) return -2;
    if (n <= 0) return -8;
    if (ldw < n) return -3;
    if (!D) return -4;
    if (ldd < n) return -5;
    if (b && ldb < 1) return -7;
    if (!out_host) return -9;
    HIPCHK(hipSetDevice(h->device));
    int nblocks = 0;
    int rc = launch_trace_dot(h, W, ldw, D, ldd, b, ldb, n, h->red + 8, &nblocks); if (rc) return rc;      // <= 2048 partial sums
    rc = launch_sum(h, h->red + 8, nblocks, h->red); if (rc) return rc;
    return fvgp_read_back(h, h->red, out_host, 1);
}

int fvgp_hip_add_matrix(fvgp_handle *h, double *A, int64_t lda, const double *B, int64_t ldb, int64_t rows, int64_t cols, double alpha) {
    if (!h) return -1;
    if (!A) return -2;
    if (!B) return -4;
    if (rows <= 0) return -6;
    if (cols <= 0 || lda < cols || ldb < cols) return -7;
    HIPCHK(hipSetDevice(h->device));
    return launch_add_matrix(h, A, lda, B, ldb, rows, cols, alpha);
}

int fvgp_hip_dot(fvgp_handle *h, const double *a, int64_t lda, const double *b, int64_t ldb, int64_t n, int c, double *out_host) {
    if (!h) return -1;
    if (!a) return -2;
    if (!b) return -4;
    if (n <= 0) return -6;
    if (c < 1 || lda < c || ldb < c) return -7;
    if (!out_host) return -8;
    HIPCHK(hipSetDevice(h->device));
    int rc = launch_dot_rows(h, a, lda, b, ldb, n, c, h->red); if (rc) return rc;
    return fvgp_read_back(h, h->red, out_host, 1);
}

int fvgp_hip_coldot(fvgp_handle *h, const double *A, int64_t lda, const double *B, int64_t ldb, int64_t rows, int64_t cols, double *out) {
    if (!h) return -1;
    if (!A) return -2;
    if (!B) return -4;
    if (rows <= 0) return -6;
    if (cols <= 0 || lda < cols || ldb < cols) return -7;
    if (!out) return -8;
    HIPCHK(hipSetDevice(h->device));
    return launch_coldot(h, A, lda, B, ldb, rows, cols, out);
}

int fvgp_hip_colsumsq(fvgp_handle *h, const double *V, int64_t rows, int64_t ldv, int64_t ncols, double *out) {
    if (!h) return -1;
    if (!V) return -2;
    if (rows <= 0) return -3;
    if (ncols <= 0 || ldv < ncols) return -4;
    if (!out) return -6;
    HIPCHK(hipSetDevice(h->device));
    return launch_colsumsq(h, V, rows, ldv, ncols, 0.0, out, -1.0);
}

int fvgp_hip_symmetrize(fvgp_handle *h, double *A, int64_t n, int64_t lda) {
    if (!h) return -1;
    if (!A) return -2;
    if (n <= 0) return -3;
    if (lda < n) return -4;
    HIPCHK(hipSetDevice(h->device));
    return launch_symmetrize(h, A, n, lda);
}

}  // extern "C"
