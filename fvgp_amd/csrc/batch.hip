// Batched log-likelihood: GPMarginalLikelihood.log_likelihood (gp_marginal_likelihood.py:137-179) at B hyperparameter vectors on
// the same x, in one call (fvgp_hip_loglik_batch, batch_api.hip).  The callers are population-based optimisers -- the reference's
// differential_evolution (fvgp/gp_training.py:66-76) scores a whole population per generation -- and grid scans.
//
// At the sizes training runs at one evaluation leaves most of the chip idle: a padded 512 x 512 factor is four latency-bound
// 128-column steps.  B independent factorisations side by side fill it.  Every launch here covers all B problems (one more grid
// dimension for the problem index), sequenced by fvgp_hip_loglik_batch (batch_api.hip):
//     assembly (kmat_batch_kernel) -> appended rows (rhs_rows_batch_kernel) ->
//     factorisation by recursive halving over the block columns: per 128 columns a leaf (leaf_batch_kernel) and a panel TRSM
//     (strided-batch GEMM by the block inverse), between two halves ONE update of the trailing lower tiles (strided-batch GEMM,
//     K = the left half's width) ->
//     tail (loglik_tail_batch_kernel): per problem sum log L_ii and |z|^2 of the appended rows.
// Launch order is the only synchronisation: no workgroup waits for another inside a launch.
//
// Results do not depend on the batch: every kernel variant is chosen from the per-problem shape only, each problem has its own
// info word, log-det slots and fixed-order reductions, and no product splits K.
#include "radial.h"
#include "kernel_family.h"
#include "leaf_body.h"

namespace {

struct KBArgs {
    const double *x; const double *vdiag; double *K;
    const double *tab;        // B x (1 + FVGP_MAX_DIM): sigma^2, then the 1 / l per dimension (kmat_desc_from_theta)
    long n, ldk, kv_stride, vd_stride;
    int d;
};

// kmat_kernel (kmat.hip) with the problem index in blockIdx.z, lower tiles of the whole dim x dim square (the extra block row of
// fvgp_hip_loglik_dim included), the noise diagonal fused and identity padding -- entry for entry the same operations
template <int KIND, int D>   // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(256) void kmat_batch_kernel(KBArgs a) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (tj > ti) return;
    const long b = blockIdx.z;
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    const int d = D ? D : a.d;
    __shared__ double sx[128 * DD];
    const double *tab = a.tab + b * (1 + FVGP_MAX_DIM);
    const double sig = tab[0];
    const double *vdiag = a.vdiag + b * a.vd_stride;
    double *K = a.K + b * a.kv_stride;
    const long n = a.n;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)ti * 128, col0 = (long)tj * 128;
    for (int e = tid; e < 128 * d; e += 256) {
        int rr = e / d, kk = e - rr * d;
        long gr = row0 + rr; if (gr >= n) gr = n - 1;
        sx[rr * DD + kk] = a.x[gr * d + kk];
    }
    const long c0 = col0 + 2 * lane, c1 = c0 + 1;
    double u0[DD], u1[DD], il[DD];
    {
        long g0 = c0 < n ? c0 : n - 1, g1 = c1 < n ? c1 : n - 1;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            if (k < d) { u0[k] = a.x[g0 * d + k]; u1[k] = a.x[g1 * d + k]; il[k] = tab[1 + k]; }
            else { u0[k] = 0.0; u1[k] = 0.0; il[k] = 0.0; }
        }
    }
    __syncthreads();

    const bool ok0 = c0 < n, ok1 = c1 < n;
    if (row0 + 128 <= n && col0 + 128 <= n && ti != tj) {          // interior tile: distance, radial function, store
        double *dst = K + (row0 + wave) * a.ldk + c0;
        const long step = 4 * a.ldk;
        for (int rb = wave; rb < 128; rb += 8, dst += 2 * step) {
            double v[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int rr = rb + 4 * u;
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int k = 0; k < DD; ++k) {
                    if (k < d) {
                        const double xr = sx[rr * DD + k];
                        const double e0 = (xr - u0[k]) * il[k], e1 = (xr - u1[k]) * il[k];
                        s0 = fma(e0, e0, s0); s1 = fma(e1, e1, s1);
                    }
                }
                v[u][0] = radial<KIND>(s0, sig); v[u][1] = radial<KIND>(s1, sig);
            }
            __builtin_nontemporal_store((double2_t){v[0][0], v[0][1]}, reinterpret_cast<double2_t *>(dst));
            __builtin_nontemporal_store((double2_t){v[1][0], v[1][1]}, reinterpret_cast<double2_t *>(dst + step));
        }
        return;
    }
    for (int rb = wave; rb < 128; rb += 8) {
        double v[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rr = rb + 4 * u;
            const long row = row0 + rr;
            const bool rok = row < n;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                if (k < d) {
                    const double xr = sx[rr * DD + k];
                    const double e0 = (xr - u0[k]) * il[k], e1 = (xr - u1[k]) * il[k];
                    s0 = fma(e0, e0, s0); s1 = fma(e1, e1, s1);
                }
            }
            double v0 = radial<KIND>(s0, sig), v1 = radial<KIND>(s1, sig);
            if (!(rok && ok0)) v0 = (row == c0) ? 1.0 : 0.0;
            if (!(rok && ok1)) v1 = (row == c1) ? 1.0 : 0.0;
            if (rok) {
                if (row == c0 && ok0) v0 += vdiag[row];
                if (row == c1 && ok1) v1 += vdiag[row];
            }
            v[u][0] = v0; v[u][1] = v1;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            double *dst = K + (row0 + rb + 4 * u) * a.ldk + c0;
            __builtin_nontemporal_store((double2_t){v[u][0], v[u][1]}, reinterpret_cast<double2_t *>(dst));
        }
    }
}

// rhs_rows_kernel (reduce.hip) per problem (blockIdx.x): rows n .. n + ncol - 1 of the square <- (y - m)^T, diagonal entry
// 1 + |y - m|^2 / min V (keeps the appended block positive definite; the factorisation leaves z^T = (L^-1 (y - m))^T there)
__global__ __launch_bounds__(1024) void rhs_rows_batch_kernel(double *KV, long kv_stride, long n, long lda, const double *ymean, long ym_stride,
                                                               int ncol, const double *vdiag, long vd_stride) {
    __shared__ double ssum[16], smin[16];
    __shared__ double sbig;
    const long b = blockIdx.x;
    double *A = KV + b * kv_stride;
    const double *ym = ymean + b * ym_stride, *vd = vdiag + b * vd_stride;
    double s = 0.0, mn = 1e300;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        for (int c = 0; c < ncol; ++c) { const double v = ym[i * ncol + c]; s = fma(v, v, s); }
        const double vv = vd[i]; mn = vv < mn ? vv : mn;
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
        if (j < n) v = ym[j * ncol + c];
        else v = (j - n == c) ? big : 0.0;
        if (j <= n + c) A[(n + c) * lda + j] = v;
    }
}

// the 128 x 128 diagonal-block Cholesky of one step for every problem (blockIdx.x): leaf_kernel (leaf.hip) with an info word per problem
__global__ __launch_bounds__(512, 4) void leaf_batch_kernel(LeafArgs g, long logdet_stride) {
    __shared__ double sT[NT * TSZ];
    __shared__ double srd[LEAF_SRD];
    const long b = blockIdx.x;
    LeafArgs gb = g;
    gb.info = g.info + b;
    leaf_body<false>(gb, g.A + b * g.a_stride, g.linv + b * g.linv_stride, g.logdet_part + b * logdet_stride, g.info_base, sT, srd, (int)threadIdx.x);
}

// per problem (blockIdx.x): out[2b] = -sum log v[i] over the dim reciprocal pivots the leaves left (sum log L_ii; 1 on padding rows),
// out[2b + 1] = |z|^2 over the appended rows n .. n + ncol - 1, columns 0 .. n - 1.  Fixed order: 256 threads striding the input,
// wave shuffles, four wave sums in turn.
__global__ __launch_bounds__(256) void loglik_tail_batch_kernel(const double *v, long dim, const double *KV, long kv_stride, long lda, long n,
                                                                 int ncol, double *out) {
    __shared__ double sw[2][4];
    const long b = blockIdx.x;
    const double *vb = v + b * dim, *A = KV + b * kv_stride;
    double s0 = 0.0, s1 = 0.0;
    for (long i = threadIdx.x; i < dim; i += blockDim.x) s0 -= log(vb[i]);
    for (int rr = 0; rr < ncol; ++rr)
        for (long j = threadIdx.x; j < n; j += blockDim.x) { const double a = A[(n + rr) * lda + j]; s1 = fma(a, a, s1); }
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off, 64); s1 += __shfl_down(s1, off, 64); }
    if ((threadIdx.x & 63) == 0) { sw[0][threadIdx.x >> 6] = s0; sw[1][threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.0;
        for (int w = 0; w < 4; ++w) t += sw[threadIdx.x][w];
        out[2 * b + threadIdx.x] = t;
    }
}

}  // namespace

int launch_kmat_batch(fvgp_handle *h, int kind, const double *x, int64_t n, int d, const double *tab, const double *vdiag, int64_t vd_stride,
                      double *KV, int64_t ld, int64_t kv_stride, int64_t dim, int64_t B) {
    KBArgs a;
    a.x = x; a.vdiag = vdiag; a.K = KV; a.tab = tab; a.n = n; a.ldk = ld; a.kv_stride = kv_stride; a.vd_stride = vd_stride; a.d = d;
    const dim3 grid((unsigned)(dim / TILE), (unsigned)(dim / TILE), (unsigned)B), block(256);
    dispatch_kind_dim(kind, d, [&](auto KIND, auto D) {
        hipLaunchKernelGGL((kmat_batch_kernel<decltype(KIND)::value, decltype(D)::value>), grid, block, 0, h->stream, a);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_rhs_rows_batch(fvgp_handle *h, double *KV, int64_t kv_stride, int64_t n, int64_t ld, const double *ymean, int64_t ym_stride, int ncol,
                          const double *vdiag, int64_t vd_stride, int64_t B) {
    hipLaunchKernelGGL(rhs_rows_batch_kernel, dim3((unsigned)B), dim3(1024), 0, h->stream, KV, (long)kv_stride, (long)n, (long)ld, ymean,
                       (long)ym_stride, ncol, vdiag, (long)vd_stride);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_leaf_batch(fvgp_handle *h, double *A, int64_t lda, int64_t a_stride, double *linv, double *logdet_part, int64_t logdet_stride,
                      int *info, int info_base, int nvalid, int64_t B, int64_t linv_stride) {
    LeafArgs g;
    g.A = A; g.lda = lda; g.linv = linv; g.logdet_part = logdet_part; g.info = info; g.info_base = info_base;
    g.do_factor = 1; g.a_stride = a_stride; g.linv_stride = linv_stride; g.nvalid = nvalid; g.stamps = nullptr;
    g.tiles_only = 0; g.preloaded = 0; g.yield = nullptr; g.col_flag = nullptr; g.col_base = 0;
    hipLaunchKernelGGL(leaf_batch_kernel, dim3((unsigned)B), dim3(512), 0, h->stream, g, (long)logdet_stride);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_loglik_tail_batch(fvgp_handle *h, const double *v, int64_t dim, const double *KV, int64_t kv_stride, int64_t ld, int64_t n, int ncol,
                             double *out, int64_t B) {
    hipLaunchKernelGGL(loglik_tail_batch_kernel, dim3((unsigned)B), dim3(256), 0, h->stream, v, (long)dim, KV, (long)kv_stride, (long)ld, (long)n,
                       ncol, out);
    HIPCHK(hipGetLastError());
    return 0;
}
