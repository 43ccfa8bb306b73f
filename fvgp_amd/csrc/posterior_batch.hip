// Batched posterior: GPposterior.posterior_mean / posterior_covariance (gp_posterior.py:139-182, 229-288, 120-136) at B hyperparameter
// vectors on the same x and the same prediction points, in one call (fvgp_hip_posterior_batch, batch_api.hip) -- what averaging a prediction
// over the theta samples of an MCMC run, comparing the end points of a multi-start optimiser or scanning a theta grid ask for.
//
// With V = L^-1 k(x, x*) and z = L^-1 (y - m):   mean = V^T z,   var = k(x*, x*) - colsumsq(V),   S = k(x*, x*) - V^T V
// -- no backward solve.  The batched factorisation of batch.hip already carries (y - m)^T as appended rows; the prediction points are
// more appended rows: k(x*, x; theta_b) placed UNDER each problem's square leaves the factorisation as V^T.  Per problem the scratch is
//     rows 0 .. dim - 1            the square of fvgp_hip_loglik_batch (z^T in rows n .. n + ncol - 1, columns 0 .. n - 1)
//     rows dim .. dim + chunk - 1  one chunk of prediction rows, columns 0 .. n - 1 = V^T after the factorisation
// and the launches, each over all B problems (sequenced in batch_api.hip), are
//     cross assembly (cross_batch_kernel) -> the recursion of batch.hip over rows >= dim (or, for a later chunk of points, its
//     solve-only pass by the kept leaf inverses) -> epilogue (post_epilogue_batch_kernel): per prediction row the mean per y column and
//     the variance, then the row's columns n .. dim - 1 zeroed (after the factorisation column n + c holds -mean_c / L_jj: no part of
//     any sum) -> with S: k(x*, x*) into S (cross_batch_kernel), one strided-batch GEMM S -= V^T-rows V^T-rows^T over K = padded n on
//     the lower tiles, the mirror into the upper triangle (s_finish_batch_kernel).
// As in batch.hip launch order is the only synchronisation and no result depends on the batch: every sum of a prediction row sees that
// row and its problem's factor only, in a fixed order.
#include "radial.h"
#include "kernel_family.h"

namespace {

struct CBArgs {
    const double *xr; const double *xc; double *K;
    const double *tab;        // B x (1 + FVGP_MAX_DIM): sigma^2, then the 1 / l per dimension
    long nr, nc, ldk, k_stride;
    int d, lower;
};

// kmat_kernel (kmat.hip, zero padding, no diagonal term) with the problem index in blockIdx.z: K_b[r][c] = k(xr_r, xc_c; theta_b) for
// r < nr, c < nc and 0 elsewhere over the whole grid of 128-tiles -- entry for entry the operations of kmat_kernel, so that a row has the
// bits fvgp_hip_kmat gives it.  lower: tiles above the block diagonal are skipped.
template <int KIND, int D>   // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(256) void cross_batch_kernel(CBArgs a) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (a.lower && tj > ti) return;
    const long b = blockIdx.z;
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    const int d = D ? D : a.d;
    __shared__ double sx[128 * DD];
    const double *tab = a.tab + b * (1 + FVGP_MAX_DIM);
    const double sig = tab[0];
    double *K = a.K + b * a.k_stride;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)ti * 128, col0 = (long)tj * 128;
    for (int e = tid; e < 128 * d; e += 256) {
        int rr = e / d, kk = e - rr * d;
        long gr = row0 + rr; if (gr >= a.nr) gr = a.nr - 1;
        sx[rr * DD + kk] = a.xr[gr * d + kk];
    }
    const long c0 = col0 + 2 * lane, c1 = c0 + 1;
    double u0[DD], u1[DD], il[DD];
    {
        long g0 = c0 < a.nc ? c0 : a.nc - 1, g1 = c1 < a.nc ? c1 : a.nc - 1;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            if (k < d) { u0[k] = a.xc[g0 * d + k]; u1[k] = a.xc[g1 * d + k]; il[k] = tab[1 + k]; }
            else { u0[k] = 0.0; u1[k] = 0.0; il[k] = 0.0; }
        }
    }
    __syncthreads();

    const bool ok0 = c0 < a.nc, ok1 = c1 < a.nc;
    for (int rb = wave; rb < 128; rb += 8) {
        double v[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rr = rb + 4 * u;
            const bool rok = row0 + rr < a.nr;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                if (k < d) {
                    const double xr = sx[rr * DD + k];
                    const double e0 = (xr - u0[k]) * il[k], e1 = (xr - u1[k]) * il[k];
                    s0 = fma(e0, e0, s0); s1 = fma(e1, e1, s1);
                }
            }
            const double v0 = radial<KIND>(s0, sig), v1 = radial<KIND>(s1, sig);
            v[u][0] = (rok && ok0) ? v0 : 0.0;
            v[u][1] = (rok && ok1) ? v1 : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            double *dst = K + (row0 + rb + 4 * u) * a.ldk + c0;
            __builtin_nontemporal_store((double2_t){v[u][0], v[u][1]}, reinterpret_cast<double2_t *>(dst));
        }
    }
}

struct PEArgs {
    double *KV;               // problem b's scratch at KV + b * kv_stride
    const int *info;          // the factorisation's info word per problem
    const double *tab;
    double *mean, *var;       // mean + (b * P + p0 + p) * ncol, var + b * P + p0 + p (var may be null)
    long kv_stride, ld, n, dim, P, p0, pc;
    int ncol;
};

constexpr int PE_ROWS = 4;    // prediction rows per workgroup: one wave each

// per (group of PE_ROWS prediction rows of the chunk, problem): the wave of row p streams V^T[p][0 .. n) once, two adjacent columns per
// lane and 256 columns per trip, with the ncol rows of z^T beside it (cache resident: every row of the problem reads the same):
//     mean[p][c] = sum_j V_pj z_cj,   var[p] = kk - sum_j V_pj^2,   kk = the radial function at r = 0 scaled by sigma^2.
// Fixed order: each lane adds its columns in ascending order (the two columns of a load into separate sums), then sum0 + sum1, then the
// shuffle tree over the wave -- a function of the row's contents alone.  NaN where the problem's factorisation failed.  Then the columns
// n .. dim - 1 of the row are zeroed (what the factorisation left there belongs to no sum; the S product reads up to padded n).
template <int KIND>
__global__ __launch_bounds__(64 * PE_ROWS) void post_epilogue_batch_kernel(PEArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long p = (long)blockIdx.x * PE_ROWS + wave, b = blockIdx.y;
    if (p >= a.pc) return;
    double *A = a.KV + b * a.kv_stride;
    double *row = A + (a.dim + p) * a.ld;
    const double *z = A + a.n * a.ld;
    const int ncol = a.ncol;
    const long n = a.n;
    double m0[FVGP_MAX_RHS_VEC], m1[FVGP_MAX_RHS_VEC];
#pragma unroll
    for (int c = 0; c < FVGP_MAX_RHS_VEC; ++c) { m0[c] = 0.0; m1[c] = 0.0; }
    double q0 = 0.0, q1 = 0.0;
    const long nfull = n & ~255L;
    long j = 2 * lane;
    for (; j < nfull; j += 256) {
        const double2_t va = *reinterpret_cast<const double2_t *>(row + j), vb = *reinterpret_cast<const double2_t *>(row + j + 128);
        q0 = fma(va[0], va[0], q0); q1 = fma(va[1], va[1], q1);
#pragma unroll
        for (int c = 0; c < FVGP_MAX_RHS_VEC; ++c)
            if (c < ncol) {
                const double2_t za = *reinterpret_cast<const double2_t *>(z + c * a.ld + j);
                m0[c] = fma(va[0], za[0], m0[c]); m1[c] = fma(va[1], za[1], m1[c]);
            }
        q0 = fma(vb[0], vb[0], q0); q1 = fma(vb[1], vb[1], q1);
#pragma unroll
        for (int c = 0; c < FVGP_MAX_RHS_VEC; ++c)
            if (c < ncol) {
                const double2_t zb = *reinterpret_cast<const double2_t *>(z + c * a.ld + j + 128);
                m0[c] = fma(vb[0], zb[0], m0[c]); m1[c] = fma(vb[1], zb[1], m1[c]);
            }
    }
    for (; j < n; j += 128) {                 // the last columns: j + 1 may be column n (not part of the sums)
        const double2_t va = *reinterpret_cast<const double2_t *>(row + j);       // (j + 1 <= n < ld: inside the row)
        const bool two = j + 1 < n;
        q0 = fma(va[0], va[0], q0);
        if (two) q1 = fma(va[1], va[1], q1);
#pragma unroll
        for (int c = 0; c < FVGP_MAX_RHS_VEC; ++c)
            if (c < ncol) {
                const double2_t za = *reinterpret_cast<const double2_t *>(z + c * a.ld + j);
                m0[c] = fma(va[0], za[0], m0[c]);
                if (two) m1[c] = fma(va[1], za[1], m1[c]);
            }
    }
    double q = q0 + q1;
    double m[FVGP_MAX_RHS_VEC];
#pragma unroll
    for (int c = 0; c < FVGP_MAX_RHS_VEC; ++c) m[c] = m0[c] + m1[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        q += __shfl_down(q, off, 64);
#pragma unroll
        for (int c = 0; c < FVGP_MAX_RHS_VEC; ++c) if (c < ncol) m[c] += __shfl_down(m[c], off, 64);
    }
    if (lane == 0) {
        const int inf = a.info[b];
        const bool bad = inf != 0 && inf <= n;
        const double nan = __builtin_nan("");
        double *mo = a.mean + (b * a.P + a.p0 + p) * ncol;
#pragma unroll
        for (int c = 0; c < FVGP_MAX_RHS_VEC; ++c) if (c < ncol) mo[c] = bad ? nan : m[c];
        if (a.var) a.var[b * a.P + a.p0 + p] = bad ? nan : radial<KIND>(0.0, a.tab[b * (1 + FVGP_MAX_DIM)]) - q;
    }
    for (long c = n + lane; c < a.dim; c += 64) row[c] = 0.0;
}

// S_b <- its lower triangle mirrored into the upper one (bitwise symmetric by construction), all NaN where the problem's factorisation
// failed: per (64 x 64 quarter of a lower 128-tile, problem), through LDS.  Of a diagonal tile the two diagonal quarters mirror their
// own strict lower triangle, the lower-left quarter fills the upper-right one.
__global__ __launch_bounds__(256) void s_finish_batch_kernel(double *S, long s_stride, long lds, const int *info, long n) {
    __shared__ double t[64][65];
    const long tt = blockIdx.x >> 2;
    int ti = (int)((__builtin_sqrt(8.0 * (double)tt + 1.0) - 1.0) * 0.5);
    while ((long)(ti + 1) * (ti + 2) / 2 <= tt) ++ti;
    while ((long)ti * (ti + 1) / 2 > tt) --ti;
    const int tj = (int)(tt - (long)ti * (ti + 1) / 2);
    const int q = blockIdx.x & 3;
    if (ti == tj && q == 1) return;            // above the diagonal: written as the mirror of quarter 2
    const bool diag = ti == tj && (q == 0 || q == 3);
    const long r0 = (long)ti * TILE + (q >> 1) * 64, c0 = (long)tj * TILE + (q & 1) * 64;
    const long b = blockIdx.y;
    double *Sb = S + b * s_stride;
    const int inf = info[b];
    const bool bad = inf != 0 && inf <= n;
    const int tid = threadIdx.x, cc = tid & 63, rq = tid >> 6;
    if (bad) {
        const double nan = __builtin_nan("");
        for (int r = rq; r < 64; r += 4) { Sb[(r0 + r) * lds + c0 + cc] = nan; Sb[(c0 + r) * lds + r0 + cc] = nan; }
        return;
    }
    for (int r = rq; r < 64; r += 4) t[r][cc] = Sb[(r0 + r) * lds + c0 + cc];
    __syncthreads();
    for (int r = rq; r < 64; r += 4)
        if (!diag || cc > r) Sb[(c0 + r) * lds + r0 + cc] = t[cc][r];
}

}  // namespace

int launch_cross_batch(fvgp_handle *h, int kind, const double *xr, int64_t nr, const double *xc, int64_t nc, int d, const double *tab,
                       double *K, int64_t ldk, int64_t k_stride, int64_t rows, int64_t cols, int lower, int64_t B) {
    CBArgs a;
    a.xr = xr; a.xc = xc; a.K = K; a.tab = tab; a.nr = nr; a.nc = nc; a.ldk = ldk; a.k_stride = k_stride; a.d = d; a.lower = lower;
    const dim3 grid((unsigned)(cols / TILE), (unsigned)(rows / TILE), (unsigned)B), block(256);
    dispatch_kind_dim(kind, d, [&](auto KIND, auto D) {
        hipLaunchKernelGGL((cross_batch_kernel<decltype(KIND)::value, decltype(D)::value>), grid, block, 0, h->stream, a);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_post_epilogue_batch(fvgp_handle *h, int kind, double *KV, int64_t kv_stride, int64_t ld, int64_t n, int64_t dim, int ncol,
                               const int *info, const double *tab, double *mean, double *var, int64_t P, int64_t p0, int64_t pc, int64_t B) {
    PEArgs a;
    a.KV = KV; a.info = info; a.tab = tab; a.mean = mean; a.var = var;
    a.kv_stride = kv_stride; a.ld = ld; a.n = n; a.dim = dim; a.P = P; a.p0 = p0; a.pc = pc; a.ncol = ncol;
    const dim3 grid((unsigned)((pc + PE_ROWS - 1) / PE_ROWS), (unsigned)B), block(64 * PE_ROWS);
    dispatch_kind(kind, [&](auto KIND) {
        hipLaunchKernelGGL(post_epilogue_batch_kernel<decltype(KIND)::value>, grid, block, 0, h->stream, a);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_s_finish_batch(fvgp_handle *h, double *S, int64_t s_stride, int64_t lds, int64_t Pp, const int *info, int64_t n, int64_t B) {
    const int64_t T = Pp / TILE;
    hipLaunchKernelGGL(s_finish_batch_kernel, dim3((unsigned)(T * (T + 1) / 2 * 4), (unsigned)B), dim3(256), 0, h->stream, S, (long)s_stride,
                       (long)lds, info, (long)n);
    HIPCHK(hipGetLastError());
    return 0;
}
