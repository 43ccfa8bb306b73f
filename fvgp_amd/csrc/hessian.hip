// The exact Hessian of the negative log marginal likelihood in the kernel's own hyperparameters (fvgp_hip_loglik_hess).
// With W = KV^-1 (POTRI), b = W (y - m), K_i = dK/dtheta_i, K_ij = d2K/dtheta_i dtheta_j:
//     g_i  = 1/2 sum_ab (W - b b^T)_ab (K_i)_ab
//     H_ij = 1/2 sum_ab (W - b b^T)_ab (K_ij)_ab - [ 1/2 tr(G_i K_j) - b^T K_j w_i ],      G_i = W K_i W,  w_i = W K_i b
// The first sum is ONE pass over the lower-stored W that re-evaluates every second derivative in registers (hess_trace_kernel, the
// sibling of kmat.hip's grad_trace_kernel; the gradient falls out of the same pass).  The bracket is what the two-vector trace kernel
// returns for (W, b, b2) := (G_i, b, 2 w_i), all j at once: per hyperparameter one assembly of K_i (kmat_grad_kernel), two N^3 products
// on the trailing update's kernel (T = W K_i, G_i = T W on the lower tiles), one matrix-vector product and one trace launch.
//
// Schedule on the handle's stream: POTRI -> second-derivative trace -> mirror W -> per i { K_i -> T -> w_i -> G_i -> trace } -> ONE copy
// of every partial sum and ONE synchronisation.  No atomics: a workgroup owns its row of partial sums and the host adds the rows in
// index order, so the same inputs give the same bits.  K_i is zero in the padding and W finite there, so nothing of the padding
// reaches an entry < n.
//
// KV is destroyed: it holds KV^-1, both triangles, on return -- nothing writes it after the mirror (the products only read it).  The
// header states this as part of the contract; the tests read W back from there (tests/test_gpu_hessian_family.py).
#include "radial.h"
#include "kernel_family.h"
#include "reduce.h"
#include <math.h>

namespace {

struct HArgs {
    const double *x; const double *W; const double *b; double *partial;
    long n, ldw, ldb;
    int d;
    double sig;
    double invl[FVGP_MAX_DIM];
};

// values a workgroup leaves: D > 0: gs, gl_0 .. gl_{D-1}, Q_km (k <= m, row by row); D == 0: gs, gl_k, Q_k0 .. Q_k15 of ITS k
__host__ __device__ constexpr int hess_row_width(int D) { return D ? 1 + D + D * (D + 1) / 2 : 2 + FVGP_MAX_DIM; }

// partial[block][..] = sums over the block's tile of wt (W_jk - b_j b_k) times
//      phi (gs),   cf e2_k (gl_k),   c2 e2_k e2_m (Q_km)          wt = 1 on the diagonal, 2 below it; e2_k = D_k^2 / l_k^2
// -- the 1 / l factors of the derivatives are applied once, by the host, to the reduced sums.  D > 0: every accumulator in registers,
// grid = (lower tiles).  D == 0 (runtime dimension <= FVGP_MAX_DIM): 136 sums Q_km would spill, so the grid has a second dimension over k
// and a workgroup owns row k of Q (16 sums); gs and gl_k ride along.
template <int KIND, int D>
__global__ __launch_bounds__(256) void hess_trace_kernel(HArgs a) {
    const long t = blockIdx.x;                 // enumerates the lower-triangular tiles
    int ti = (int)((__builtin_sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long)(ti + 1) * (ti + 2) / 2 <= t) ++ti;
    while ((long)ti * (ti + 1) / 2 > t) --ti;
    const int tj = (int)(t - (long)ti * (ti + 1) / 2);
    const int k0 = D ? 0 : (int)blockIdx.y;    // D == 0: this workgroup's row of Q
    const long pidx = (long)blockIdx.y * gridDim.x + blockIdx.x;

    constexpr int DD = D ? D : FVGP_MAX_DIM;
    constexpr int NV = hess_row_width(D);
    constexpr int NQ = D ? D * (D + 1) / 2 : FVGP_MAX_DIM;
    const int d = D ? D : a.d;
    __shared__ double sx[128 * DD];
    __shared__ double sb[128];
    __shared__ double sred[4][NV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)ti * 128, col0 = (long)tj * 128;
    for (int e = tid; e < 128 * d; e += 256) {
        int rr = e / d, kk = e - rr * d;
        long gr = row0 + rr; if (gr >= a.n) gr = a.n - 1;
        sx[rr * DD + kk] = a.x[gr * d + kk];
    }
    if (tid < 128) { long gr = row0 + tid; sb[tid] = gr < a.n ? a.b[gr * a.ldb] : 0.0; }
    const long c0 = col0 + 2 * lane, c1 = c0 + 1;
    double u0[DD], u1[DD], il[DD];
    const long g0 = c0 < a.n ? c0 : a.n - 1, g1 = c1 < a.n ? c1 : a.n - 1;
    // D == 0: the column points' coordinate k0 and its 1 / l, picked by comparison (a runtime index into u0 / u1 / il would move the
    // arrays to scratch)
    double uk0 = 0.0, uk1 = 0.0, ilk = 0.0;
#pragma unroll
    for (int k = 0; k < DD; ++k) {
        if (k < d) { u0[k] = a.x[g0 * d + k]; u1[k] = a.x[g1 * d + k]; il[k] = a.invl[k]; }
        else { u0[k] = 0.0; u1[k] = 0.0; il[k] = 0.0; }
        if (!D && k == k0) { uk0 = u0[k]; uk1 = u1[k]; ilk = il[k]; }
    }
    const double bc0 = c0 < a.n ? a.b[c0 * a.ldb] : 0.0, bc1 = c1 < a.n ? a.b[c1 * a.ldb] : 0.0;
    __syncthreads();

    double gs = 0.0, glk = 0.0;
    double gl[DD], q[NQ];
#pragma unroll
    for (int k = 0; k < DD; ++k) gl[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NQ; ++k) q[k] = 0.0;

    // one entry: weight wt, row point rr, column point h
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
        double phi, cf, c2;
        radial_hess<KIND>(r2, a.sig, phi, cf, c2);
        gs = fma(wt, phi, gs);
        const double wc = wt * cf;
        if constexpr (D != 0) {
            int idx = 0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                gl[k] = fma(wc, e2[k], gl[k]);
                const double wk = wt * (c2 * e2[k]);          // c2 meets an e2 factor before it meets the weight: 0 on a coincident pair
#pragma unroll
                for (int m = k; m < DD; ++m) { q[idx] = fma(wk, e2[m], q[idx]); ++idx; }
            }
        } else {
            const double ek = (sx[rr * DD + k0] - (h ? uk1 : uk0)) * ilk, ek2 = ek * ek;
            glk = fma(wc, ek2, glk);
            const double wk = wt * (c2 * ek2);
#pragma unroll
            for (int m = 0; m < DD; ++m) if (m < d) q[m] = fma(wk, e2[m], q[m]);
        }
    };
    const double *Wp = a.W + (row0 + wave) * a.ldw + c0;
    if (row0 + 128 <= a.n && ti != tj) {
        // interior tile strictly below the diagonal: every entry counts twice, two rows per trip
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
    // the workgroup's row: wave sums by shuffles, then the four waves in index order
    double v[NV];
    v[0] = gs;
    if constexpr (D != 0) {
#pragma unroll
        for (int k = 0; k < DD; ++k) v[1 + k] = gl[k];
#pragma unroll
        for (int k = 0; k < NQ; ++k) v[1 + DD + k] = q[k];
    } else {
        v[1] = glk;
#pragma unroll
        for (int k = 0; k < NQ; ++k) v[2 + k] = q[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += __shfl_down(v[k], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) sred[wave][k] = v[k];
    }
    __syncthreads();
    if (tid < NV) a.partial[pidx * NV + tid] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
}

// the full matrix dK/dtheta_i of ONE hyperparameter, both triangles, zero in the padding rows and columns up to np (a multiple of 128):
// kmat_kernel's layout -- a workgroup per 128 x 128 tile, a wave owns whole rows, a lane two adjacent columns, every store one contiguous
// 1 KiB row segment, non-temporal (the products read it from HBM).  which < 0: d/dsigma^2 = phi; else d/dl of dimension `which`
// (cf e2_which / l), of every dimension summed for an isotropic length scale.
struct KGArgs {
    const double *x; double *K;
    long n, ldk;
    int d, which, iso;
    double sig, ilw;          // ilw: 1 / l of the differentiated length scale
    double invl[FVGP_MAX_DIM];
};

template <int KIND, int D>
__global__ __launch_bounds__(256) void kmat_grad_kernel(KGArgs a) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    const int d = D ? D : a.d;
    __shared__ double sx[128 * DD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)ti * 128, col0 = (long)tj * 128;
    for (int e = tid; e < 128 * d; e += 256) {
        int rr = e / d, kk = e - rr * d;
        long gr = row0 + rr; if (gr >= a.n) gr = a.n - 1;
        sx[rr * DD + kk] = a.x[gr * d + kk];
    }
    const long c0 = col0 + 2 * lane, c1 = c0 + 1;
    double u0[DD], u1[DD], il[DD];
    {
        const long g0 = c0 < a.n ? c0 : a.n - 1, g1 = c1 < a.n ? c1 : a.n - 1;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            if (k < d) { u0[k] = a.x[g0 * d + k]; u1[k] = a.x[g1 * d + k]; il[k] = a.invl[k]; }
            else { u0[k] = 0.0; u1[k] = 0.0; il[k] = 0.0; }
        }
    }
    __syncthreads();
    const bool ok0 = c0 < a.n, ok1 = c1 < a.n;
    for (int rb = wave; rb < 128; rb += 8) {
        double v[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rr = rb + 4 * u;
            const bool rok = row0 + rr < a.n;
            double s0 = 0.0, s1 = 0.0, p0 = 0.0, p1 = 0.0;      // r2 and the part of it the differentiated length scale owns
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                if (k < d) {
                    const double xr = sx[rr * DD + k];
                    const double e0 = (xr - u0[k]) * il[k], e1 = (xr - u1[k]) * il[k];
                    const double q0 = e0 * e0, q1 = e1 * e1;
                    s0 += q0; s1 += q1;
                    if (a.iso || k == a.which) { p0 += q0; p1 += q1; }
                }
            }
            double phi0, cf0, phi1, cf1;
            radial_grad<KIND>(s0, a.sig, phi0, cf0);
            radial_grad<KIND>(s1, a.sig, phi1, cf1);
            const double v0 = a.which < 0 ? phi0 : cf0 * p0 * a.ilw, v1 = a.which < 0 ? phi1 : cf1 * p1 * a.ilw;
            v[u][0] = (rok && ok0) ? v0 : 0.0; v[u][1] = (rok && ok1) ? v1 : 0.0;
        }
        double *dst = a.K + (row0 + rb) * a.ldk + c0;
        __builtin_nontemporal_store((double2_t){v[0][0], v[0][1]}, reinterpret_cast<double2_t *>(dst));
        __builtin_nontemporal_store((double2_t){v[1][0], v[1][1]}, reinterpret_cast<double2_t *>(dst + 4 * a.ldk));
    }
}

// out[p] = scale * sum_{k < n} T[p][k] b[k ldb], p < n: a workgroup streams its row (16-byte loads), sums in a fixed order
__global__ __launch_bounds__(256) void rowdot_scale_kernel(const double *T, long ldt, const double *b, long ldb, long n, double scale, double *out) {
    __shared__ double sp[4];
    const long p = blockIdx.x;
    const double *row = T + p * ldt;
    double s = 0.0;
    for (long i = 2L * threadIdx.x; i < n; i += 512) {
        if (i + 1 < n) {
            const double2_t tv = *reinterpret_cast<const double2_t *>(row + i);
            s = fma(tv[1], b[(i + 1) * ldb], fma(tv[0], b[i * ldb], s));
        } else s = fma(row[i], b[i * ldb], s);
    }
    const double t = block_sum4(s, sp);
    if (threadIdx.x == 0) out[p] = scale * t;
}

int launch_hess_trace(fvgp_handle *h, const KmatDesc &k, const double *W, int64_t ldw, const double *b, int64_t ldb, double *partial,
                      long *nblocks_out, int *width_out) {
    HArgs a;
    a.x = k.x1; a.W = W; a.b = b; a.partial = partial;
    a.n = k.n1; a.ldw = ldw; a.ldb = ldb; a.d = k.d; a.sig = k.sig;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.invl[i] = k.invl[i];
    const long T = (a.n + 127) / 128, nb = T * (T + 1) / 2;
    const bool runtime_d = k.d > 4;
    dim3 grid((unsigned)nb, runtime_d ? (unsigned)k.d : 1u), block(256);
    *nblocks_out = nb;
    *width_out = hess_row_width(runtime_d ? 0 : k.d);
    dispatch_kind_dim(k.kind, k.d, [&](auto KIND, auto D) {
        hipLaunchKernelGGL((hess_trace_kernel<decltype(KIND)::value, decltype(D)::value>), grid, block, 0, h->stream, a);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

// dK/dtheta_i, np x np, of the kernel-owned hyperparameter i (0: sigma^2, 1 + k: the length scale of dimension k, or the one there is)
int launch_kmat_grad(fvgp_handle *h, const KmatDesc &k, int i, double *K, int64_t ldk, int64_t np) {
    KGArgs a;
    a.x = k.x1; a.K = K; a.n = k.n1; a.ldk = ldk; a.d = k.d; a.iso = (k.iso && i > 0) ? 1 : 0; a.which = i - 1;
    a.sig = k.sig; a.ilw = i > 0 ? k.invl[k.iso ? 0 : i - 1] : 0.0;
    for (int j = 0; j < FVGP_MAX_DIM; ++j) a.invl[j] = k.invl[j];
    dim3 grid((unsigned)(np / TILE), (unsigned)(np / TILE)), block(256);
    dispatch_kind_dim(k.kind, k.d, [&](auto KIND, auto D) {
        hipLaunchKernelGGL((kmat_grad_kernel<decltype(KIND)::value, decltype(D)::value>), grid, block, 0, h->stream, a);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_rowdot_scale(fvgp_handle *h, const double *T, int64_t ldt, const double *b, int64_t ldb, int64_t n, double scale, double *out) {
    hipLaunchKernelGGL(rowdot_scale_kernel, dim3((unsigned)n), dim3(256), 0, h->stream, T, (long)ldt, b, (long)ldb, (long)n, scale, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// doubles of the second-derivative pass's partial sums for an input dimension d
int64_t hess_partial_doubles(int64_t nb, int d) { return nb * (d > 4 ? (int64_t)d * hess_row_width(0) : (int64_t)hess_row_width(d)); }

// fvgp_hip_loglik_hess's scratch: ONE piece that the host reads back in one copy -- the second-derivative pass's rows (hpart, nh doubles)
// and behind them, as the view tpart, the trace passes' (room for d + 1 passes of nb rows of d + 1 sums; a kernel with nk parameters
// fills nk passes of nb rows of nk) --, then the vector 2 w_i
struct HessWs { double *hpart, *tpart, *w2; int64_t nb, nh; };
HessWs hess_layout(Carve &c, int64_t n, int d) {
    const int64_t np = pad128(n), T = np / TILE, nk = d + 1, nb = T * (T + 1) / 2, nh = hess_partial_doubles(nb, d);
    double *sums = c.take<double>(nh + nk * nk * nb, sizeof(double));
    return {sums, c.view<double>(sums, nh), c.take<double>(np, sizeof(double)), nb, nh};
}

}  // namespace

extern "C" {

int64_t fvgp_hip_loglik_hess_workspace_bytes(int64_t n, int d) {
    if (n < 1 || d < 1 || d > FVGP_MAX_DIM) return -1;
    return carve_bytes(hess_layout, n, d);
}

int fvgp_hip_loglik_hess(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                         const double *theta, int ntheta, const double *alpha, int ncol, int component,
                         double *KV, int64_t ld, double *work, int64_t ldw, double *work2, int64_t ldw2,
                         double *ws, int64_t ws_bytes, double *grad_host, double *hess_host) {
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!x) return -3;
    if (n <= 0) return -4;
    int rc = check_kernel_args(kernel_id, d, theta, ntheta, 5, 6, 7); if (rc) return rc;
    const int nk = kernel_param_count(kernel_id, d);
    if (!alpha) return -8;
    if (ncol < 1) return -9;
    if (component < 0 || component >= ncol) { fvgp_set_error("loglik_hess: 0 <= component < ncol"); return -10; }
    rc = check_square(KV, n, ld, 11, 4, 12);
    if (rc) return rc;
    rc = check_square(work, n, ldw, 13, 4, 14);
    if (rc) return rc;
    rc = check_square(work2, n, ldw2, 15, 4, 16);
    if (rc) return rc;
    if (!ws || ((uintptr_t)ws & 7)) return -17;
    Carve c(ws); const HessWs l = hess_layout(c, n, d);
    if (ws_bytes < c.bytes()) { fvgp_set_error("loglik_hess: ws smaller than fvgp_hip_loglik_hess_workspace_bytes(n, d)"); return -18; }
    if (!grad_host) return -19;
    if (!hess_host) return -20;
    GradDesc g{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &g.k); if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const int64_t np = pad128(n), nb = l.nb;
    g.k.x1 = x; g.k.n1 = n; g.k.x2 = x; g.k.n2 = n;
    const double *b = alpha + component;
    double *hpart = l.hpart, *tpart = l.tpart, *w2 = l.w2;

    rc = fvgp_hip_potri(h, KV, n, ld, work, ldw); if (rc) return rc;                     // W in the lower tiles of KV; `work` is dead
    long hblocks = 0; int hw = 0;
    rc = launch_hess_trace(h, g.k, KV, ld, b, ncol, hpart, &hblocks, &hw); if (rc) return rc;
    rc = launch_symmetrize(h, KV, np, ld); if (rc) return rc;                            // the products read all of W (padding included)
    g.ntheta = nk;
    g.W = work2; g.ldw = ldw2; g.b = b; g.ldb = ncol; g.b2 = w2; g.ldb2 = 1;
    for (int i = 0; i < nk; ++i) {
        rc = launch_kmat_grad(h, g.k, i, work2, ldw2, np); if (rc) return rc;                                                            // C = K_i
        rc = launch_gemm(h, gemm_desc(0, 0, np, np, np, 1.0, KV, ld, work2, ldw2, 0.0, work, ldw)); if (rc) return rc;                   // B = T = W K_i
        rc = launch_rowdot_scale(h, work, ldw, b, ncol, n, 2.0, w2); if (rc) return rc;                                                  // 2 w_i = 2 T b
        rc = launch_gemm(h, gemm_desc(0, 0, np, np, np, 1.0, work, ldw, KV, ld, 0.0, work2, ldw2).lower_tiles()); if (rc) return rc;     // C = G_i = T W
        g.partial = tpart + (int64_t)i * nk * nb;
        int nblocks = 0;
        rc = launch_grad_trace(h, g, &nblocks); if (rc) return rc;
        if (nblocks != nb) { fvgp_set_error("loglik_hess: the trace pass left an unexpected number of rows"); return -100; }
    }
    const size_t nh = (size_t)l.nh, nt = (size_t)nk * nk * nb;
    std::vector<double> part(nh + nt);
    HIPCHK(hipMemcpyAsync(part.data(), hpart, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    rc = fvgp_ipc_check(h); if (rc) return rc;

    // ---- the reduced sums of the second-derivative pass (rows added in index order)
    long double gs = 0.0L, gl[FVGP_MAX_DIM], Q[FVGP_MAX_DIM][FVGP_MAX_DIM];
    for (int k = 0; k < d; ++k) { gl[k] = 0.0L; for (int m = 0; m < d; ++m) Q[k][m] = 0.0L; }
    if (d <= 4) {
        for (long bb = 0; bb < hblocks; ++bb) {
            const double *r = part.data() + (size_t)bb * hw;
            gs += r[0];
            int idx = 1 + d;
            for (int k = 0; k < d; ++k) { gl[k] += r[1 + k]; for (int m = k; m < d; ++m) Q[k][m] += r[idx++]; }
        }
    } else {
        for (int k = 0; k < d; ++k)
            for (long bb = 0; bb < hblocks; ++bb) {
                const double *r = part.data() + ((size_t)k * hblocks + bb) * hw;
                if (k == 0) gs += r[0];
                gl[k] += r[1];
                for (int m = k; m < d; ++m) Q[k][m] += r[2 + m];
            }
    }
    for (int k = 0; k < d; ++k) for (int m = 0; m < k; ++m) Q[k][m] = Q[m][k];
    // ---- A_ij = 1/2 sum (W - b b^T) K_ij and the gradient, with the 1 / l factors
    const long double s = g.k.sig;
    std::vector<long double> A((size_t)nk * nk, 0.0L), gr((size_t)nk, 0.0L);
    gr[0] = 0.5L * gs;
    if (g.k.iso) {
        const long double il = g.k.invl[0];
        long double sl = 0.0L, sq = 0.0L;
        for (int k = 0; k < d; ++k) { sl += gl[k]; for (int m = 0; m < d; ++m) sq += Q[k][m]; }
        gr[1] = 0.5L * sl * il;
        A[1] = A[nk] = gr[1] / s;
        A[nk + 1] = 0.5L * (sq - 3.0L * sl) * il * il;
    } else {
        for (int k = 0; k < d; ++k) {
            const long double ilk = g.k.invl[k];
            gr[1 + k] = 0.5L * gl[k] * ilk;
            A[1 + k] = A[(size_t)(1 + k) * nk] = gr[1 + k] / s;
            for (int m = 0; m < d; ++m)
                A[(size_t)(1 + k) * nk + 1 + m] = 0.5L * (Q[k][m] * ilk * (long double)g.k.invl[m] - (k == m ? 3.0L * gl[k] * ilk * ilk : 0.0L));
        }
    }
    for (int i = 0; i < ntheta; ++i) grad_host[i] = i < nk ? (double)gr[i] : 0.0;
    // ---- row i: A_ij minus half the two-vector trace of (G_i, b, 2 w_i) against K_j
    for (int i = 0; i < nk; ++i)
        for (int j = 0; j < nk; ++j) {
            long double tr = 0.0L;
            const double *p = part.data() + nh + (size_t)i * nk * nb;
            for (long bb = 0; bb < nb; ++bb) tr += p[(size_t)bb * nk + j];
            hess_host[(size_t)i * nk + j] = (double)(A[(size_t)i * nk + j] - 0.5L * tr);
        }
    return 0;
}

}  // extern "C"
