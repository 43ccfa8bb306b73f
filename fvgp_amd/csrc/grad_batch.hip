// Batched log-likelihood gradient: GPMarginalLikelihood.neg_log_likelihood_gradient's kernel part (gp_marginal_likelihood.py:224-309)
// at B hyperparameter vectors on the same x, in one call (fvgp_hip_loglik_grad_batch, batch_api.hip) -- what a multi-start gradient
// optimiser asks for at every step.  After the batched factorisation of batch.hip (every leaf's block inverse kept), per problem on
// its own square:
//     z from the appended rows, identity padding back, the leaf inverses into the diagonal tiles (grad_init_batch_kernel) ->
//     W = L^-1 in place by recursive halving over the block columns, inv([[A,0],[C,D]]) = [[A^-1,0],[-D^-1 C A^-1, D^-1]]
//     (two strided-batch GEMMs per halving, batch_api.hip) ->
//     b = W^T z = KV^-1 (y - m) (wtz_batch_kernel) ->
//     W^T into the second square (transpose_lower_batch_kernel), KV^-1 = W^T W over W (one strided-batch GEMM, potri_kminor's layout) ->
//     fused trace (grad_trace_batch_kernel: grad_trace_kernel's arithmetic) -> per-problem fixed-order sum (grad_reduce_batch_kernel).
// As in batch.hip every launch covers all B problems, nothing waits inside a launch, and no result depends on the batch.
#include "radial.h"
#include "kernel_family.h"

namespace {

constexpr int TW = 1 + FVGP_MAX_DIM;       // theta table row / gradient row: sigma^2, then one entry per dimension

// per (block column jt, problem): z = row n + component of the factor over this tile's columns (0 past n); then this tile column of
// rows n .. np - 1 becomes identity again and the diagonal tile takes the kept leaf inverse (zeros above its diagonal, identity rows
// from n on: the inverse of blockdiag(L11, I)).  A workgroup reads and writes its own 128 columns only.
__global__ __launch_bounds__(256) void grad_init_batch_kernel(double *KV, long kv_stride, long ld, long n, long np, int component,
                                                              const double *linv, long linv_stride, double *z, long z_stride) {
    const int jt = blockIdx.x;
    const long b = blockIdx.y;
    double *A = KV + b * kv_stride;
    const double *li = linv + b * linv_stride + (long)jt * LEAF_DOUBLES;
    double *zb = z + b * z_stride;
    const long c0 = (long)jt * TILE;
    const int tid = threadIdx.x;
    if (tid < TILE) {
        const long j = c0 + tid;
        zb[j] = j < n ? A[(n + component) * ld + j] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < TILE * TILE; e += 256) {
        const int rr = e >> 7, cc = e & 127;
        const long r = c0 + rr, c = c0 + cc;
        const double v = r >= n ? (r == c ? 1.0 : 0.0) : (cc > rr ? 0.0 : li[e]);
        A[r * ld + c] = v;
    }
    if (c0 + TILE < np)
        for (long e = tid; e < (np - n) * TILE; e += 256) A[(n + e / TILE) * ld + c0 + (e & 127)] = 0.0;
}

// b = W^T z per (block column jt, problem): b_j = sum over rows i >= 128 jt, i < n (z is 0 beyond) of W_ij z_i.  Two halves of the
// workgroup take alternate rows, their sums added in a fixed order; 0 past n.
__global__ __launch_bounds__(256) void wtz_batch_kernel(const double *KV, long kv_stride, long ld, long n, const double *z, double *bv,
                                                        long z_stride) {
    __shared__ double sp[TILE];
    const int jt = blockIdx.x;
    const long b = blockIdx.y;
    const double *A = KV + b * kv_stride, *zb = z + b * z_stride;
    const int tid = threadIdx.x, col = tid & 127, half = tid >> 7;
    const long j = (long)jt * TILE + col;
    double s = 0.0;
    for (long i = (long)jt * TILE + half; i < n; i += 2) s = fma(A[i * ld + j], zb[i], s);
    if (half) sp[col] = s;
    __syncthreads();
    if (!half) bv[b * z_stride + j] = j < n ? s + sp[col] : 0.0;
}

// lower triangular tile index t -> (ti, tj), ti >= tj
__device__ __forceinline__ void lower_tile(const long t, int &ti, int &tj) {
    ti = (int)((__builtin_sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long)(ti + 1) * (ti + 2) / 2 <= t) ++ti;
    while ((long)ti * (ti + 1) / 2 > t) --ti;
    tj = (int)(t - (long)ti * (ti + 1) / 2);
}

// dst <- src^T over the lower 128-tiles of every problem (the upper tiles of dst, diagonal tiles transposed): per (64 x 64 quarter of
// a lower tile, problem), through LDS
__global__ __launch_bounds__(256) void transpose_lower_batch_kernel(const double *src, long s_stride, long lds, double *dst, long d_stride,
                                                                    long ldd) {
    __shared__ double t[64][65];
    int ti, tj;
    lower_tile((long)(blockIdx.x >> 2), ti, tj);
    const int q = blockIdx.x & 3;
    const long r0 = (long)ti * TILE + (q >> 1) * 64, c0 = (long)tj * TILE + (q & 1) * 64;
    const double *S = src + blockIdx.y * s_stride;
    double *D = dst + blockIdx.y * d_stride;
    const int tid = threadIdx.x, cc = tid & 63, rq = tid >> 6;
    for (int r = rq; r < 64; r += 4) t[r][cc] = S[(r0 + r) * lds + c0 + cc];
    __syncthreads();
    for (int r = rq; r < 64; r += 4) D[(c0 + r) * ldd + r0 + cc] = t[cc][r];
}

struct GBArgs {
    const double *x; const double *W; const double *b; const double *tab; double *partial;
    long n, ldw, w_stride, b_stride, p_stride;    // per problem: W (lower triangle of KV^-1), b, TW doubles of partial sums per tile
    int d, iso;
};

// grad_trace_kernel (kmat.hip) with the problem index in blockIdx.y: partial[b][tile][i] = sum over the lower tile of
// w_jk (W_jk - b_j b_k) dK_jk/dtheta_i, w = 1 on the diagonal, 2 below it; sigma^2 and 1 / l from the problem's theta table row
template <int KIND, int D>   // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(256) void grad_trace_batch_kernel(GBArgs a) {
    int ti, tj;
    const long pidx = blockIdx.x, pb = blockIdx.y;
    lower_tile(pidx, ti, tj);
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    const int d = D ? D : a.d;
    __shared__ double sx[128 * DD];
    __shared__ double sb[128];
    __shared__ double sred[4][DD + 1];
    const double *tab = a.tab + pb * TW;
    const double sig = tab[0];
    const double *W = a.W + pb * a.w_stride, *bb = a.b + pb * a.b_stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)ti * 128, col0 = (long)tj * 128;
    for (int e = tid; e < 128 * d; e += 256) {
        int rr = e / d, kk = e - rr * d;
        long gr = row0 + rr; if (gr >= a.n) gr = a.n - 1;
        sx[rr * DD + kk] = a.x[gr * d + kk];
    }
    if (tid < 128) { long gr = row0 + tid; sb[tid] = gr < a.n ? bb[gr] : 0.0; }
    const long c0 = col0 + 2 * lane, c1 = c0 + 1;
    double u0[DD], u1[DD], il[DD];
    const long g0 = c0 < a.n ? c0 : a.n - 1, g1 = c1 < a.n ? c1 : a.n - 1;
#pragma unroll
    for (int k = 0; k < DD; ++k) {
        if (k < d) { u0[k] = a.x[g0 * d + k]; u1[k] = a.x[g1 * d + k]; il[k] = tab[1 + k]; }
        else { u0[k] = 0.0; u1[k] = 0.0; il[k] = 0.0; }
    }
    const double bc0 = c0 < a.n ? bb[c0] : 0.0, bc1 = c1 < a.n ? bb[c1] : 0.0;
    __syncthreads();

    double gs = 0.0;          // d/dsig accumulator
    double gl[DD];            // d/dl_k accumulators, WITHOUT the factor 1 / l_k (applied once at the end)
#pragma unroll
    for (int k = 0; k < DD; ++k) gl[k] = 0.0;

    auto entry = [&](const int rr, const int h, const double wt) {
        double e2[DD];
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            if (k < d) {
                const double e = (sx[rr * DD + k] - (h ? u1[k] : u0[k])) * il[k];
                e2[k] = e * e; r2 += e2[k];
            } else e2[k] = 0.0;
        }
        double phi, cf;
        radial_grad<KIND>(r2, sig, phi, cf);
        gs = fma(wt, phi, gs);
        const double wc = wt * cf;
#pragma unroll
        for (int k = 0; k < DD; ++k) if (k < d) gl[k] = fma(wc, e2[k], gl[k]);
    };
    const double *Wp = W + (row0 + wave) * a.ldw + c0;
    if (row0 + 128 <= a.n && ti != tj) {
        for (int rr = wave; rr < 128; rr += 8, Wp += 8 * a.ldw) {
            const double2_t wa = *reinterpret_cast<const double2_t *>(Wp), wb = *reinterpret_cast<const double2_t *>(Wp + 4 * a.ldw);
            const double bra = sb[rr], brb = sb[rr + 4];
            entry(rr, 0, 2.0 * (wa[0] - bra * bc0));
            entry(rr, 1, 2.0 * (wa[1] - bra * bc1));
            entry(rr + 4, 0, 2.0 * (wb[0] - brb * bc0));
            entry(rr + 4, 1, 2.0 * (wb[1] - brb * bc1));
        }
    } else {
        for (int rr = wave; rr < 128; rr += 4, Wp += 4 * a.ldw) {
            const long row = row0 + rr;
            if (row >= a.n) break;
            const double2_t w2 = *reinterpret_cast<const double2_t *>(Wp);
            const double br = sb[rr];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const long c = h ? c1 : c0;
                if (c > row || c >= a.n) continue;
                entry(rr, h, (c == row ? 1.0 : 2.0) * ((h ? w2[1] : w2[0]) - br * (h ? bc1 : bc0)));
            }
        }
    }
#pragma unroll
    for (int k = 0; k < DD; ++k) gl[k] *= il[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        gs += __shfl_down(gs, off, 64);
#pragma unroll
        for (int k = 0; k < DD; ++k) if (k < d) gl[k] += __shfl_down(gl[k], off, 64);
    }
    if (lane == 0) {
        sred[wave][0] = gs;
#pragma unroll
        for (int k = 0; k < DD; ++k) if (k < d) sred[wave][1 + k] = gl[k];
    }
    __syncthreads();
    if (tid == 0) {
        double *out = a.partial + pb * a.p_stride + pidx * TW;
        out[0] = sred[0][0] + sred[1][0] + sred[2][0] + sred[3][0];
        if (a.iso) {
            double acc = 0.0;
            for (int k = 0; k < d; ++k) acc += sred[0][1 + k] + sred[1][1 + k] + sred[2][1 + k] + sred[3][1 + k];
            out[1] = acc;
        } else {
            for (int k = 0; k < d; ++k) out[1 + k] = sred[0][1 + k] + sred[1][1 + k] + sred[2][1 + k] + sred[3][1 + k];
        }
    }
}

// grad[b][i] = 1/2 sum over the tiles, in tile order, of partial[b][tile][i] (one lane per hyperparameter, compensated sum: the
// single evaluation sums in long double on the host); 0 for i >= nk
__global__ __launch_bounds__(64) void grad_reduce_batch_kernel(const double *partial, long p_stride, long ntiles, int nk, double *grad) {
    const long b = blockIdx.x;
    const int i = threadIdx.x;
    if (i >= TW) return;
    const double *p = partial + b * p_stride + i;
    double s = 0.0, c = 0.0;
    if (i < nk)
        for (long t = 0; t < ntiles; ++t) {
            const double v = p[t * TW], u = s + v;
            c += fabs(s) >= fabs(v) ? (s - u) + v : (v - u) + s;
            s = u;
        }
    grad[b * TW + i] = 0.5 * (s + c);
}

// the optional outputs: b (b_out, n per problem) and diag(KV^-1) (diag_out, n per problem)
__global__ __launch_bounds__(256) void grad_outputs_batch_kernel(const double *bv, long bv_stride, const double *KV, long kv_stride, long ld,
                                                                 long n, double *b_out, double *diag_out) {
    const long b = blockIdx.y, j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (b_out) b_out[b * n + j] = bv[b * bv_stride + j];
    if (diag_out) diag_out[b * n + j] = KV[b * kv_stride + j * ld + j];
}

}  // namespace

int launch_grad_init_batch(fvgp_handle *h, double *KV, int64_t kv_stride, int64_t ld, int64_t n, int component, const double *linv,
                           int64_t linv_stride, double *z, int64_t z_stride, int64_t B) {
    const int64_t np = pad128(n);
    hipLaunchKernelGGL(grad_init_batch_kernel, dim3((unsigned)(np / TILE), (unsigned)B), dim3(256), 0, h->stream, KV, (long)kv_stride, (long)ld,
                       (long)n, (long)np, component, linv, (long)linv_stride, z, (long)z_stride);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_wtz_batch(fvgp_handle *h, const double *KV, int64_t kv_stride, int64_t ld, int64_t n, const double *z, double *bv, int64_t z_stride,
                     int64_t B) {
    hipLaunchKernelGGL(wtz_batch_kernel, dim3((unsigned)(pad128(n) / TILE), (unsigned)B), dim3(256), 0, h->stream, KV, (long)kv_stride, (long)ld,
                       (long)n, z, bv, (long)z_stride);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_transpose_lower_batch(fvgp_handle *h, const double *src, int64_t s_stride, int64_t lds, double *dst, int64_t d_stride, int64_t ldd,
                                 int64_t np, int64_t B) {
    const int64_t T = np / TILE;
    hipLaunchKernelGGL(transpose_lower_batch_kernel, dim3((unsigned)(T * (T + 1) / 2 * 4), (unsigned)B), dim3(256), 0, h->stream, src,
                       (long)s_stride, (long)lds, dst, (long)d_stride, (long)ldd);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_grad_trace_batch(fvgp_handle *h, int kind, int iso, const double *x, int64_t n, int d, const double *W, int64_t w_stride, int64_t ldw,
                            const double *b, int64_t b_stride, const double *tab, double *partial, int64_t p_stride, int64_t B) {
    GBArgs a;
    a.x = x; a.W = W; a.b = b; a.tab = tab; a.partial = partial;
    a.n = n; a.ldw = ldw; a.w_stride = w_stride; a.b_stride = b_stride; a.p_stride = p_stride; a.d = d; a.iso = iso;
    const int64_t T = pad128(n) / TILE;
    const dim3 grid((unsigned)(T * (T + 1) / 2), (unsigned)B), block(256);
    dispatch_kind_dim(kind, d, [&](auto KIND, auto D) {
        hipLaunchKernelGGL((grad_trace_batch_kernel<decltype(KIND)::value, decltype(D)::value>), grid, block, 0, h->stream, a);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_grad_reduce_batch(fvgp_handle *h, const double *partial, int64_t p_stride, int64_t ntiles, int nk, double *grad, int64_t B) {
    hipLaunchKernelGGL(grad_reduce_batch_kernel, dim3((unsigned)B), dim3(64), 0, h->stream, partial, (long)p_stride, (long)ntiles, nk, grad);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_grad_outputs_batch(fvgp_handle *h, const double *bv, int64_t bv_stride, const double *KV, int64_t kv_stride, int64_t ld, int64_t n,
                              double *b_out, double *diag_out, int64_t B) {
    hipLaunchKernelGGL(grad_outputs_batch_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, h->stream, bv, (long)bv_stride,
                       KV, (long)kv_stride, (long)ld, (long)n, b_out, diag_out);
    HIPCHK(hipGetLastError());
    return 0;
}
