// Scalar, column and row reductions (HBM-bound work): every sum in a fixed order, the single-value ones through reduce.h.
#include "common.h"
#include "reduce.h"

namespace {

// s += x with the rounding of the addition kept in c (two-sum: exact for any two doubles)
__device__ __forceinline__ void comp_add(double &s, double &c, const double x) {
    const double t = s + x, z = t - s;
    c += (s - (t - z)) + (x - z);
    s = t;
}

// out[0] = 2 sum log |L_ii|, fixed order.  The sum is compensated, so the result is rounded once.  A plain sum is an ulp or two of
// the result off at a thousand rows (2.1e-12 at n = 1300 on B B^T + n I, log det = 1e4, one ulp = 1.8e-12) -- not wrong by any
// usual measure, but the bar tests/test_gpu_chol.py holds the log-determinant to, n eps cond_2(A), is 1.4e-12 on that matrix:
// BELOW one ulp of the result, and only a sum that is rounded once (half an ulp, 0.9e-12) can meet it
__global__ void diag_logsum_kernel(const double *L, long n, long ldl, double *out) {
    __shared__ double sw[16], sc[16];
    double s = 0.0, c = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) comp_add(s, c, log(fabs(L[i * ldl + i])));
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_down(s, off, 64), oc = __shfl_down(c, off, 64);
        comp_add(s, c, os);
        c += oc;
    }
    if ((threadIdx.x & 63) == 0) { sw[threadIdx.x >> 6] = s; sc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0, tc = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { comp_add(t, tc, sw[w]); tc += sc[w]; }
        out[0] = 2.0 * (t + tc);
    }
}

__global__ void sum_kernel(const double *v, long n, double *out) {
    __shared__ double sw[16];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) s += v[i];
    const double t = block_sum(s, sw);
    if (threadIdx.x == 0) out[0] = t;
}

// out[0] = -sum log v[i]  (v = the reciprocal diagonal the leaves leave: sum log L_ii), fixed order
__global__ void neg_log_sum_kernel(const double *v, long n, double *out) {
    __shared__ double sw[16];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) s -= log(v[i]);
    const double t = block_sum(s, sw);
    if (threadIdx.x == 0) out[0] = t;
}

// out[0] = sum_{i<n, cc<c} a[i*lda+cc] * b[i*ldb+cc]
__global__ void dot_rows_kernel(const double *a, long lda, const double *b, long ldb, long n, int c, double *out) {
    __shared__ double sw[16];
    double s = 0.0;
    const long tot = n * c;
    for (long e = threadIdx.x; e < tot; e += blockDim.x) { const long i = e / c; const int cc = (int)(e - i * c); s = fma(a[i * lda + cc], b[i * ldb + cc], s); }
    const double t = block_sum(s, sw);
    if (threadIdx.x == 0) out[0] = t;
}

// out[p] = base - sum_{i<rows} V[i*ldv+p]^2, p < P   (posterior variance: k(x_p,x_p) - |L^-1 k_p|^2)
__global__ void colsumsq_kernel(const double *V, long rows, long ldv, long P, double base, double *out, double sign) {
    __shared__ double sp[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long p = (long)blockIdx.x * 32 + tx;
    double s = 0.0;
    if (p < P) for (long i = ty; i < rows; i += 8) { const double v = V[i * ldv + p]; s = fma(v, v, s); }
    sp[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && p < P) { double t = 0.0; for (int k = 0; k < 8; ++k) t += sp[k][tx]; out[p] = base - sign * t; }
}

// out[p] = sum_{i<rows} A[i*lda+p] * B[i*ldb+p], p < P   (column-wise dot products: k^T (KV^-1 k) per prediction point)
__global__ void coldot_kernel(const double *A, long lda, const double *B, long ldb, long rows, long P, double *out) {
    __shared__ double sp[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long p = (long)blockIdx.x * 32 + tx;
    double s = 0.0;
    if (p < P) for (long i = ty; i < rows; i += 8) s = fma(A[i * lda + p], B[i * ldb + p], s);
    sp[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && p < P) { double t = 0.0; for (int k = 0; k < 8; ++k) t += sp[k][tx]; out[p] = t; }
}

// row-wise twins of the two kernels above for the transposed cross-covariance block KT (P x n): one workgroup per
// prediction point streams its row (16-byte loads, coalesced), block sums in a fixed order
template <int C>
__global__ __launch_bounds__(256) void rows_dot_kernel(const double *KT, long ldk, const double *alpha, long lda, int ncol, long n,
                                                       double *out, long ldo) {
    __shared__ double sp[4][C];
    const long p = blockIdx.x;
    const double *row = KT + p * ldk;
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (long i = 2L * threadIdx.x; i < n; i += 512) {        // n is read up to the even index below it; the odd tail follows
        if (i + 1 < n) {
            const double2_t kv = *reinterpret_cast<const double2_t *>(row + i);
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (c < ncol) acc[c] = fma(kv[1], alpha[(i + 1) * lda + c], fma(kv[0], alpha[i * lda + c], acc[c]));
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) if (c < ncol) acc[c] = fma(row[i], alpha[i * lda + c], acc[c]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += __shfl_down(acc[c], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < C; ++c) sp[threadIdx.x >> 6][c] = acc[c];
    __syncthreads();
    if (threadIdx.x < ncol) out[p * ldo + threadIdx.x] = (sp[0][threadIdx.x] + sp[1][threadIdx.x]) + (sp[2][threadIdx.x] + sp[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void rows_sumsq_base_kernel(const double *KT, long ldk, long n, double base, double *out) {
    __shared__ double sp[4];
    const long p = blockIdx.x;
    const double *row = KT + p * ldk;
    double s = 0.0;
    for (long i = 2L * threadIdx.x; i < n; i += 512) {
        if (i + 1 < n) { const double2_t v = *reinterpret_cast<const double2_t *>(row + i); s = fma(v[1], v[1], fma(v[0], v[0], s)); }
        else s = fma(row[i], row[i], s);
    }
    const double t = block_sum4(s, sp);
    if (threadIdx.x == 0) out[p] = base - t;
}

// partial[block] = sum over the block's rows i and all j < n of (W[i][j] - b_i b_j) D[i][j]: the trace term of the gradient
// for a derivative matrix D that exists as numbers (host kernel callables, matrix-valued noise derivatives),
// tr(KV^-1 dK) - b^T dK b with W = KV^-1 symmetric and full (gp_marginal_likelihood.py:301-306); b may be null
__global__ __launch_bounds__(256) void trace_dot_kernel(const double *W, long ldw, const double *D, long ldd, const double *b, long ldb,
                                                        long n, double *partial) {
    __shared__ double sw[4];
    double s = 0.0;
    for (long i = blockIdx.x; i < n; i += gridDim.x) {
        const double bi = b ? b[i * ldb] : 0.0;
        for (long j = threadIdx.x; j < n; j += 256) {
            const double bj = b ? b[j * ldb] : 0.0;
            s = fma(W[i * ldw + j] - bi * bj, D[i * ldd + j], s);
        }
    }
    const double t = block_sum4(s, sw);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// rows n..n+ncol-1 of the padded K+V <- (y-m)^T with a diagonal entry 1 + sum|y-m|^2 / min(V), which
// dominates |L^-1 (y-m)|^2 <= |y-m|^2 / lambda_min(K+V) and so keeps the appended block positive definite
__global__ void rhs_rows_kernel(double *A, long n, long lda, const double *ymean, int ncol, const double *vdiag) {
    __shared__ double ssum[16], smin[16];
    __shared__ double sbig;
    double s = 0.0, mn = 1e300;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        for (int c = 0; c < ncol; ++c) { const double v = ymean[i * ncol + c]; s = fma(v, v, s); }
        const double vv = vdiag[i]; mn = vv < mn ? vv : mn;
    }
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off, 64); const double o = __shfl_down(mn, off, 64); mn = o < mn ? o : mn; }
    if ((threadIdx.x & 63) == 0) { ssum[threadIdx.x >> 6] = s; smin[threadIdx.x >> 6] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0, m2 = 1e300;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { t += ssum[w]; m2 = smin[w] < m2 ? smin[w] : m2; }
        sbig = 1.0 + t / m2;
    }
    __syncthreads();
    const double big = sbig;
    for (long e = threadIdx.x; e < (long)ncol * (n + ncol); e += blockDim.x) {
        const int c = (int)(e / (n + ncol)); const long j = e % (n + ncol);
        double v;
        if (j < n) v = ymean[j * ncol + c];
        else v = (j - n == c) ? big : 0.0;
        if (j <= n + c) A[(n + c) * lda + j] = v;
    }
}

// out[0] = sum over rows row0..row0+nrows-1, cols 0..ncols-1 of A^2
__global__ void rowsumsq_kernel(const double *A, long lda, long row0, int nrows, long ncols, double *out) {
    __shared__ double sw[16];
    double s = 0.0;
    for (int rr = 0; rr < nrows; ++rr)
        for (long j = threadIdx.x; j < ncols; j += blockDim.x) { const double v = A[(row0 + rr) * lda + j]; s = fma(v, v, s); }
    const double t = block_sum(s, sw);
    if (threadIdx.x == 0) out[0] = t;
}

// What follows the fused factorisation of fvgp_hip_loglik in ONE launch (four launches of ~5 us each at the training loop's sizes):
// block 0: out[0] = -sum log v[i] (neg_log_sum_kernel); block 1: out[1] = the squared norm of the appended rows (rowsumsq_kernel);
// the other blocks: vec <- the appended rows transposed, alpha <- 0.  The two sums are those kernels' own: the same 1024 threads
// striding the input, the same block_sum.
__global__ __launch_bounds__(1024) void loglik_tail_kernel(const double *v, long nlog, const double *A, long lda, long row0, int nrows, double *out,
                                                         double *vec, int C, long np, double *alpha, int ncol) {
    __shared__ double sw[16];
    if (blockIdx.x <= 1) {
        double s = 0.0;
        if (blockIdx.x == 0) { for (long i = threadIdx.x; i < nlog; i += blockDim.x) s -= log(v[i]); }
        else {
            for (int rr = 0; rr < nrows; ++rr)
                for (long j = threadIdx.x; j < row0; j += blockDim.x) { const double a = A[(row0 + rr) * lda + j]; s = fma(a, a, s); }
        }
        const double t = block_sum(s, sw);
        if (threadIdx.x == 0) out[blockIdx.x] = t;
        return;
    }
    if (!vec) return;
    const long stride = (long)(gridDim.x - 2) * blockDim.x, first = (long)(blockIdx.x - 2) * blockDim.x + threadIdx.x;
    for (long e = first; e < np * C; e += stride) {
        const long i = e / C; const int c = (int)(e % C);
        vec[e] = (i < row0 && c < nrows) ? A[(row0 + c) * lda + i] : 0.0;
    }
    for (long e = first; e < np * ncol; e += stride) alpha[e] = 0.0;
}

}  // namespace

int launch_loglik_tail(fvgp_handle *h, const double *v, int64_t nlog, const double *A, int64_t lda, int64_t n, int ncol, double *out2_dev,
                       double *vec, int C, int64_t np, double *alpha) {
    long blocks = vec ? (np * C + 1023) / 1024 : 0; if (blocks > 1024) blocks = 1024;
    HIPLAUNCH(loglik_tail_kernel, dim3((unsigned)(2 + blocks)), dim3(1024), h->stream, v, (long)nlog, A, (long)lda, (long)n, ncol, out2_dev,
              vec, C, (long)np, alpha, ncol);
    return 0;
}

int launch_rhs_rows(fvgp_handle *h, double *A, int64_t n, int64_t lda, const double *ymean, int ncol, const double *vdiag) {
    HIPLAUNCH(rhs_rows_kernel, dim3(1), dim3(1024), h->stream, A, (long)n, (long)lda, ymean, ncol, vdiag);
    return 0;
}

int launch_rowsumsq(fvgp_handle *h, const double *A, int64_t lda, int64_t row0, int nrows, int64_t ncols, double *out_dev) {
    HIPLAUNCH(rowsumsq_kernel, dim3(1), dim3(1024), h->stream, A, (long)lda, (long)row0, nrows, (long)ncols, out_dev);
    return 0;
}

int launch_diag_logsum(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *out_dev) {
    HIPLAUNCH(diag_logsum_kernel, dim3(1), dim3(1024), h->stream, L, (long)n, (long)ldl, out_dev);
    return 0;
}

int launch_sum(fvgp_handle *h, const double *v, int64_t n, double *out_dev) {
    HIPLAUNCH(sum_kernel, dim3(1), dim3(1024), h->stream, v, (long)n, out_dev);
    return 0;
}

int launch_neg_log_sum(fvgp_handle *h, const double *v, int64_t n, double *out_dev) {
    HIPLAUNCH(neg_log_sum_kernel, dim3(1), dim3(1024), h->stream, v, (long)n, out_dev);
    return 0;
}

int launch_dot_rows(fvgp_handle *h, const double *a, int64_t lda, const double *b, int64_t ldb, int64_t n, int c, double *out_dev) {
    HIPLAUNCH(dot_rows_kernel, dim3(1), dim3(1024), h->stream, a, (long)lda, b, (long)ldb, (long)n, c, out_dev);
    return 0;
}

int launch_colsumsq(fvgp_handle *h, const double *V, int64_t rows, int64_t ldv, int64_t P, double base, double *out, double sign) {
    HIPLAUNCH(colsumsq_kernel, dim3((unsigned)((P + 31) / 32)), dim3(256), h->stream, V, (long)rows, (long)ldv, (long)P, base, out, sign);
    return 0;
}

int launch_coldot(fvgp_handle *h, const double *A, int64_t lda, const double *B, int64_t ldb, int64_t rows, int64_t P, double *out) {
    HIPLAUNCH(coldot_kernel, dim3((unsigned)((P + 31) / 32)), dim3(256), h->stream, A, (long)lda, B, (long)ldb, (long)rows, (long)P, out);
    return 0;
}

int launch_rows_dot(fvgp_handle *h, const double *KT, int64_t ldk, const double *alpha, int64_t lda, int ncol, int64_t n, int64_t P,
                    double *out, int64_t ldo) {
    if (ncol < 1 || ncol > 8) return -5;
    if ((ldk & 1) || ((uintptr_t)KT & 15)) return -2;
    return dispatch_rhs_width(ncol, [&](auto C) {
        HIPLAUNCH((rows_dot_kernel<decltype(C)::value>), dim3((unsigned)P), dim3(256), h->stream, KT, (long)ldk, alpha, (long)lda, ncol, (long)n, out, (long)ldo);
        return 0;
    });
}

int launch_rows_sumsq_base(fvgp_handle *h, const double *KT, int64_t ldk, int64_t n, int64_t P, double base, double *out) {
    if ((ldk & 1) || ((uintptr_t)KT & 15)) return -2;
    HIPLAUNCH(rows_sumsq_base_kernel, dim3((unsigned)P), dim3(256), h->stream, KT, (long)ldk, (long)n, base, out);
    return 0;
}

int launch_trace_dot(fvgp_handle *h, const double *W, int64_t ldw, const double *D, int64_t ldd, const double *b, int64_t ldb, int64_t n,
                     double *partial, int *nblocks) {
    const long blocks = n < 2048 ? n : 2048;
    HIPLAUNCH(trace_dot_kernel, dim3((unsigned)blocks), dim3(256), h->stream, W, (long)ldw, D, (long)ldd, b, (long)ldb, (long)n, partial);
    *nblocks = (int)blocks;
    return 0;
}
