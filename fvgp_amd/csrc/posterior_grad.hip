// Posterior mean and variance WITH their exact gradients in the prediction points (fvgp_hip_posterior_grad): what a gradient-based
// acquisition optimiser asks for at every step.  The reference (gp_posterior.py:184-226, 290-331) differentiates the kernel by a forward
// difference of step 1e-8; for the stationary kernels of radial.h the derivative is closed form.  With D_k = x*_k - x_ik, e_k = D_k / l_k,
// r^2 = sum e_k^2 and cf the factor radial_grad<KIND> returns,
//     dk(x*, x_i) / dx*_k = -cf(r^2) e_k / l_k                          (RBF, Matern 3/2, 5/2; finite at r = 0 for all three)
// and with alpha = KVinvY[:, component], W = KV^-1 k(x, x*):
//     A_p = sum_i k_ip alpha_i        q_p = sum_i k_ip W_ip        dm_pk = sum_i dk_ip/dx*_k alpha_i        dv_pk = -2 sum_i dk_ip/dx*_k W_ip
// -- one pass over the n x P matrix W, no dk matrix, no P x P product.
//
// W is row-major with the prediction points contiguous, so LANES RUN ALONG p (a wave reads 512 contiguous bytes of a row of W) and every
// lane carries the 2 + 2 n_dirs sums of its point.  The data rows are split into slices of PG_ROWS = 256, one workgroup per (64 points,
// slice): the slice's x rows and alpha entries are staged in LDS once (every lane reads the same row: broadcast reads), each of the four
// waves takes 64 of the rows, the four waves' sums are added through LDS in wave order and stored as the slice's partial; a second launch
// adds the slices in ascending order.  No atomics, and the split is a function of n alone: a point's results have the same bits whatever
// P is, whichever points share the call and wherever the caller cuts a long list of points into calls.
// Per entry: one exp, one rsq (radial_grad), d subtractions and 2 d + 2 n_dirs + 2 (+ 2 n_dirs + 2 with W) fused multiply-adds.
#include "radial.h"
#include "kernel_family.h"
#include "slice_sum.h"

namespace {

constexpr int PG_ROWS = SLICE_ROWS;            // data rows per workgroup (slice_sum.h)
constexpr int PG_WAVE_ROWS = SLICE_WAVE_ROWS;  // ... per wave

struct PGArgs {
    const double *x, *xp, *alpha, *W;
    double *part;                 // (slices, 2 + 2 nd, P)
    long n, P, ldw;
    int d, nd, ncol, comp;
    double sig;
    double il[FVGP_MAX_DIM];
};

template <int KIND, int D, bool HASW>   // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(256) void posterior_grad_kernel(PGArgs a) {
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    constexpr int NACC = 2 + 2 * DD;
    constexpr int STAGE = PG_ROWS * (DD + 1), RED = 3 * NACC * 64;
    __shared__ double sm[STAGE > RED ? STAGE : RED];      // the staged rows; afterwards the sums of waves 1 .. 3
    double *sx = sm, *sa = sm + PG_ROWS * DD;
    const int d = D ? D : a.d, nd = a.nd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.y * PG_ROWS;
    const long p = (long)blockIdx.x * 64 + lane;
    const long pc = p < a.P ? p : a.P - 1;

    slice_stage<DD>(sx, sa, a.x, a.alpha + a.comp, a.ncol, a.n, d, row0, tid);
    double u[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) u[k] = k < d ? a.xp[pc * d + k] : 0.0;
    double sA = 0.0, sq = 0.0, gm[DD], gv[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) { gm[k] = 0.0; gv[k] = 0.0; }
    __syncthreads();

    const int r0 = wave * PG_WAVE_ROWS;
    const int rows = slice_wave_rows(a.n, row0, wave);        // rows of this wave that exist
    // (p < 64 ceil(P / 64) <= padded P <= ldw: inside the row for every lane)
    const double *Wp = HASW ? a.W + (row0 + r0) * a.ldw + p : nullptr;
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
        const double w = HASW ? Wp[(long)r * a.ldw] : 0.0;
        const double *xr = sx + (r0 + r) * DD;
        const double al = sa[r0 + r];
        double e[DD], r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < d) { e[k] = (u[k] - xr[k]) * a.il[k]; r2 = fma(e[k], e[k], r2); }
        double phi, cf;
        radial_grad<KIND>(r2, a.sig, phi, cf);
        const double kv = KIND == 0 ? cf : a.sig * phi;
        sA = fma(kv, al, sA);
        const double ca = cf * al;
        if (HASW) sq = fma(kv, w, sq);
        const double cw = cf * w;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < nd) {
                const double g = e[k] * a.il[k];
                gm[k] = fma(g, ca, gm[k]);
                if (HASW) gv[k] = fma(g, cw, gv[k]);
            }
    }

    __syncthreads();                                          // every wave is done with the staged rows
    if (wave > 0) {
        double *red = slice_parked(sm, NACC, wave, lane);
        red[0] = sA; red[64] = sq;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < nd) { red[(2 + k) * 64] = gm[k]; red[(2 + DD + k) * 64] = gv[k]; }
    }
    __syncthreads();
    if (wave != 0 || p >= a.P) return;
    const int nacc = 2 + 2 * nd;
    double *out = a.part + (long)blockIdx.y * nacc * a.P + p;
#pragma unroll
    for (int ww = 0; ww < 3; ++ww) {                             // ((wave 0 + wave 1) + wave 2) + wave 3
        const double *red = slice_parked(sm, NACC, ww + 1, lane);
        sA += red[0]; sq += red[64];
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < nd) { gm[k] += red[(2 + k) * 64]; gv[k] += red[(2 + DD + k) * 64]; }
    }
    out[0] = sA;
    if (HASW) out[a.P] = sq;
#pragma unroll
    for (int k = 0; k < DD; ++k)
        if (k < nd) {
            out[(2 + k) * a.P] = gm[k];
            if (HASW) out[(2 + nd + k) * a.P] = gv[k];
        }
}

// the slices' partial sums added in ascending order, one thread per (sum, point); the signs of the derivative go on here:
//     dm = -sum cf e / l alpha,   dv = +2 sum cf e / l W
__global__ __launch_bounds__(256) void posterior_grad_reduce_kernel(const double *part, long S, long P, int nd, int hasw,
                                                                    double *A, double *q, double *dm, double *dv) {
    const int nacc = 2 + 2 * nd;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nacc * P) return;
    const int s = (int)(idx / P);
    const long p = idx - s * P;
    if (!hasw && (s == 1 || s >= 2 + nd)) return;
    double t = 0.0;
    for (long j = 0; j < S; ++j) t += part[(j * nacc + s) * P + p];
    if (s == 0) A[p] = t;
    else if (s == 1) q[p] = t;
    else if (s < 2 + nd) dm[p * nd + (s - 2)] = -t;
    else dv[p * nd + (s - 2 - nd)] = 2.0 * t;
}

int64_t pg_slices(int64_t n) { return slice_count(n); }

// fvgp_hip_posterior_grad's scratch: every slice's partial sums, 2 + 2 n_dirs per prediction point
double *pg_layout(Carve &c, int64_t n, int64_t P, int n_dirs) { return c.take<double>(pg_slices(n) * (2 + 2 * (int64_t)n_dirs) * P, sizeof(double)); }

}  // namespace

int64_t fvgp_hip_posterior_grad_workspace_bytes(int64_t n, int64_t P, int n_dirs) {
    if (n < 1 || P < 1 || n_dirs < 1 || n_dirs > FVGP_MAX_DIM) return -1;
    return carve_bytes(pg_layout, n, P, n_dirs);
}

int fvgp_hip_posterior_grad(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                            const double *theta, int ntheta, const double *xpred, int64_t P,
                            const double *alpha, int ncol, int component, const double *W, int64_t ldw, int n_dirs,
                            double *work, int64_t work_bytes, double *A_out, double *q_out, double *dm_out, double *dv_out) {
    if (!h) return -1;
    if (!x) return -3;
    if (n <= 0) return -4;
    if (!theta) return -6;
    if (!xpred) return -8;
    if (P <= 0) return -9;
    if (!alpha) return -10;
    if (ncol < 1) return -11;
    if (component < 0 || component >= ncol) { fvgp_set_error("posterior_grad: 0 <= component < ncol"); return -12; }
    if (W && ldw < pad128(P)) { fvgp_set_error("posterior_grad: ldw >= padded_dim(P)"); return -14; }
    KmatDesc k{};
    int rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    if (n_dirs < 1 || n_dirs > d) { fvgp_set_error("posterior_grad: 1 <= n_dirs <= d"); return -15; }
    if (!work) return -16;
    Carve c(work); double *part = pg_layout(c, n, P, n_dirs);
    if (work_bytes < c.bytes()) {
        fvgp_set_error("posterior_grad: work smaller than fvgp_hip_posterior_grad_workspace_bytes(n, P, n_dirs)"); return -17;
    }
    if (!A_out) return -18;
    if (W && !q_out) return -19;
    if (!dm_out) return -20;
    if (W && !dv_out) return -21;
    HIPCHK(hipSetDevice(h->device));
    PGArgs a;
    a.x = x; a.xp = xpred; a.alpha = alpha; a.W = W; a.part = part;
    a.n = n; a.P = P; a.ldw = ldw; a.d = d; a.nd = n_dirs; a.ncol = ncol; a.comp = component;
    a.sig = k.sig;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.il[i] = k.invl[i];
    const int64_t S = pg_slices(n);
    if (S > 65535) { fvgp_set_error("posterior_grad: n too large"); return -4; }
    const dim3 grid((unsigned)((P + 63) / 64), (unsigned)S), block(256);
    dispatch_kind_dim(k.kind, d, [&](auto KIND, auto D) {
        constexpr int KD = decltype(KIND)::value, DIM = decltype(D)::value;
        if (W) hipLaunchKernelGGL((posterior_grad_kernel<KD, DIM, true>), grid, block, 0, h->stream, a);
        else hipLaunchKernelGGL((posterior_grad_kernel<KD, DIM, false>), grid, block, 0, h->stream, a);
    });
    HIPCHK(hipGetLastError());
    const int64_t total = (2 + 2 * (int64_t)n_dirs) * P;
    hipLaunchKernelGGL(posterior_grad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream,
                       (const double *)part, (long)S, (long)P, n_dirs, W ? 1 : 0, A_out, q_out, dm_out, dv_out);
    HIPCHK(hipGetLastError());
    return 0;
}
