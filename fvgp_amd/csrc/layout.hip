// Small data-movement kernels (HBM-bound work): copies, transposes, additions, padding and the seed of the block inverses.
#include "common.h"

namespace {

// dst (rows_pad, ldd) <- src (rows, lds) for [rows x cols], zero elsewhere up to rows_pad x cols_pad
__global__ void copy_cols_kernel(const double *src, long lds, double *dst, long ldd, long rows, long cols, long rows_pad, long cols_pad) {
    const long tot = rows_pad * cols_pad;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
        const long i = e / cols_pad, j = e - i * cols_pad;
        dst[i * ldd + j] = (i < rows && j < cols) ? src[i * lds + j] : 0.0;
    }
}

__global__ void symmetrize_kernel(double *A, long n, long lda) {
    // 32x32 tile transpose through LDS; only tiles with bi > bj (and the diagonal tiles in place)
    __shared__ double t[32][33];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: ty 0..7
    for (int rr = ty; rr < 32; rr += 8) {
        const long i = (long)bi * 32 + rr, j = (long)bj * 32 + tx;
        t[rr][tx] = (i < n && j < n) ? A[i * lda + j] : 0.0;
    }
    __syncthreads();
    for (int rr = ty; rr < 32; rr += 8) {
        const long i = (long)bj * 32 + rr, j = (long)bi * 32 + tx;   // target (i,j) in the upper triangle = source (j,i)
        if (i < n && j < n && j > i) A[i * lda + j] = t[tx][rr];
    }
}

// seed of the 1024-block inverses: block row b (128 x 1024) of W <- zeros, with inv(L_bb) at its place on the diagonal of
// the 1024-block the row belongs to
__global__ __launch_bounds__(256) void winv_seed_kernel(const double *linv, double *W, int wshift) {
    const long b = blockIdx.x;
    const int w = 1 << wshift;                       // width of the blocks being inverted (1024; 512 ... 2048 for a panel's square)
    const int c0 = (int)(b & ((w >> 7) - 1)) * 128;
    const double *src = linv + b * 128 * 128;
    double *dst = W + b * 128 * w;
    // blockIdx.y: sixteen rows of the block row each (eight workgroups per 128 rows: a panel's seed is on the chain's path)
    for (int e = (blockIdx.y * 16 << wshift) + threadIdx.x * 2; e < ((blockIdx.y + 1) * 16 << wshift); e += 512) {
        const int i = e >> wshift, j = e & (w - 1);
        double2_t v = {0.0, 0.0};
        if (j >= c0 && j < c0 + 128) v = *reinterpret_cast<const double2_t *>(src + i * 128 + (j - c0));
        *reinterpret_cast<double2_t *>(dst + e) = v;
    }
}

// copy the 128x128 tiles on and below the block diagonal (np a multiple of 128)
__global__ void copy_lower_tiles_kernel(const double *src, long lds, double *dst, long ldd) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (tj > ti) return;
    for (int e = threadIdx.x; e < 128 * 64; e += blockDim.x) {
        const int rr = e >> 6, c2 = (e & 63) * 2;
        const long off_s = ((long)ti * 128 + rr) * lds + (long)tj * 128 + c2;
        const long off_d = ((long)ti * 128 + rr) * ldd + (long)tj * 128 + c2;
        *reinterpret_cast<double2_t *>(dst + off_d) = *reinterpret_cast<const double2_t *>(src + off_s);
    }
}

// dst (cols x rows) <- src^T for a rows x cols matrix, both multiples of 32, in 32 x 32 pieces through LDS
__global__ void transpose_kernel(const double *src, long lds, double *dst, long ldd) {
    __shared__ double t[32][33];
    const long bj = blockIdx.x, bi = blockIdx.y;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int rr = ty; rr < 32; rr += 8) t[rr][tx] = src[(bi * 32 + rr) * lds + bj * 32 + tx];
    __syncthreads();
    for (int rr = ty; rr < 32; rr += 8) dst[(bj * 32 + rr) * ldd + bi * 32 + tx] = t[tx][rr];
}

// dst tile (tj, ti) <- transpose of src tile (ti, tj) for the 128 x 128 tiles on and below the block diagonal, in 32 x 32
// pieces through LDS (the upper part of src's diagonal tiles is explicit zeros, so dst's diagonal tiles come out with a zero
// lower part): W = inv(L) (lower, k-major for W^T W) becomes W^T (upper, k-minor: the (M,K) x (N,K) layout of the fast GEMM)
// `mirror`: in place (dst == src), only the pieces strictly below the diagonal -- a symmetric matrix whose 128-tiles on and below
// the block diagonal were computed gets its upper part (the diagonal tiles were computed whole)
__global__ void transpose_lower_tiles_kernel(const double *src, long lds, double *dst, long ldd, int mirror) {
    __shared__ double t[32][33];
    const int bj = blockIdx.x, bi = blockIdx.y;           // 32-granular block coordinates in src
    if ((bj >> 2) > (bi >> 2)) return;
    if (mirror && bj >= bi) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int rr = ty; rr < 32; rr += 8) t[rr][tx] = src[((long)bi * 32 + rr) * lds + (long)bj * 32 + tx];
    __syncthreads();
    for (int rr = ty; rr < 32; rr += 8) dst[((long)bj * 32 + rr) * ldd + (long)bi * 32 + tx] = t[tx][rr];
}

// A[i][j] += alpha * B[i][j] on the lower triangle (j <= i < n): K + V for a matrix-valued noise model (gp_kv.py:654-657)
__global__ void add_lower_kernel(double *A, long lda, const double *B, long ldb, long n, double alpha) {
    for (long i = blockIdx.y; i < n; i += gridDim.y)
        for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j <= i; j += (long)gridDim.x * blockDim.x)
            A[i * lda + j] = fma(alpha, B[i * ldb + j], A[i * lda + j]);
}

// A[i][j] += alpha * B[i][j] on a rows x cols rectangle
__global__ void add_matrix_kernel(double *A, long lda, const double *B, long ldb, long rows, long cols, double alpha) {
    const long tot = rows * cols;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
        const long i = e / cols, j = e - i * cols;
        A[i * lda + j] = fma(alpha, B[i * ldb + j], A[i * lda + j]);
    }
}

// rows n..np-1 of a padded square matrix <- identity rows (lower part; the strict upper is never read)
__global__ void pad_identity_kernel(double *A, long n, long np, long lda) {
    const long rows = np - n;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < rows * np; e += (long)gridDim.x * blockDim.x) {
        const long i = n + e / np, j = e % np;
        if (j <= i) A[i * lda + j] = (i == j) ? 1.0 : 0.0;
    }
}

}  // namespace

int launch_add_lower(fvgp_handle *h, double *A, int64_t lda, const double *B, int64_t ldb, int64_t n, double alpha) {
    long bx = (n + 255) / 256; if (bx > 64) bx = 64;
    const long by = n < 65535 ? n : 65535;                 // gridDim.y is limited to 65535: the rows are walked with that stride
    HIPLAUNCH(add_lower_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), h->stream, A, (long)lda, B, (long)ldb, (long)n, alpha);
    return 0;
}

int launch_add_matrix(fvgp_handle *h, double *A, int64_t lda, const double *B, int64_t ldb, int64_t rows, int64_t cols, double alpha) {
    long tot = rows * cols;
    if (tot <= 0) return 0;
    long blocks = (tot + 255) / 256; if (blocks > 8192) blocks = 8192;
    HIPLAUNCH(add_matrix_kernel, dim3((unsigned)blocks), dim3(256), h->stream, A, (long)lda, B, (long)ldb, (long)rows, (long)cols, alpha);
    return 0;
}

int launch_pad_identity(fvgp_handle *h, double *A, int64_t n, int64_t np, int64_t lda) {
    if (np <= n) return 0;
    long tot = (np - n) * np;
    long blocks = (tot + 255) / 256; if (blocks > 2048) blocks = 2048;
    HIPLAUNCH(pad_identity_kernel, dim3((unsigned)blocks), dim3(256), h->stream, A, (long)n, (long)np, (long)lda);
    return 0;
}

int launch_copy_cols(fvgp_handle *h, const double *src, int64_t lds, double *dst, int64_t ldd, int64_t rows, int64_t cols,
                     int64_t rows_pad, int64_t cols_pad) {
    long tot = rows_pad * cols_pad;
    if (tot <= 0) return 0;
    long blocks = (tot + 255) / 256; if (blocks > 4096) blocks = 4096;
    HIPLAUNCH(copy_cols_kernel, dim3((unsigned)blocks), dim3(256), h->stream, src, (long)lds, dst, (long)ldd, (long)rows, (long)cols, (long)rows_pad, (long)cols_pad);
    return 0;
}

int launch_symmetrize(fvgp_handle *h, double *A, int64_t n, int64_t lda) {
    unsigned nb = (unsigned)((n + 31) / 32);
    HIPLAUNCH(symmetrize_kernel, dim3(nb, nb), dim3(256), h->stream, A, (long)n, (long)lda);
    return 0;
}

int launch_winv_seed(fvgp_handle *h, const double *linv, int64_t nblk, double *W, int64_t w) {
    if (nblk <= 0) return 0;
    int wshift = 7;
    while ((1L << wshift) < w) ++wshift;
    if ((1L << wshift) != w || w > 8192) { fvgp_set_error("block inverses: the width must be 128 times a power of two"); return -5; }
    HIPLAUNCH(winv_seed_kernel, dim3((unsigned)nblk, 8), dim3(256), h->stream, linv, W, wshift);
    return 0;
}

int launch_transpose(fvgp_handle *h, const double *src, int64_t lds, double *dst, int64_t ldd, int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    if (rows % 32 || cols % 32) { fvgp_set_error("transpose: multiples of 32"); return -5; }
    HIPLAUNCH(transpose_kernel, dim3((unsigned)(cols / 32), (unsigned)(rows / 32)), dim3(256), h->stream, src, (long)lds, dst, (long)ldd);
    return 0;
}

int launch_transpose_lower_tiles(fvgp_handle *h, const double *src, int64_t lds, double *dst, int64_t ldd, int64_t np) {
    unsigned nb = (unsigned)(np / 32);
    if (nb == 0) return 0;
    HIPLAUNCH(transpose_lower_tiles_kernel, dim3(nb, nb), dim3(256), h->stream, src, (long)lds, dst, (long)ldd, src == dst ? 1 : 0);
    return 0;
}

int launch_copy_lower_tiles(fvgp_handle *h, const double *src, int64_t lds, double *dst, int64_t ldd, int64_t np) {
    unsigned nb = (unsigned)(np / 128);
    if (nb == 0) return 0;
    HIPLAUNCH(copy_lower_tiles_kernel, dim3(nb, nb), dim3(256), h->stream, src, (long)lds, dst, (long)ldd);
    return 0;
}
