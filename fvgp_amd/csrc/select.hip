// Greedy batch selection of measurement points (fvgp_hip_select_batch): the pivoted Cholesky of the posterior covariance of
// P candidates, q steps, without the P x P matrix.  With d the candidates' conditional latent variances, s their noise variances and
// j the candidate picked at step t (largest d_i, or largest d_i / s_i; ties to the lowest index),
//     r_i = k(x_i, x_j) - sum_n k(x_i, X_n) w_n,      w = KV^-1 k(X, x_j)                 (column j of the posterior covariance)
//     c_i = (r_i - sum_{s<t} G[s,i] G[s,j]) / sqrt(d_j + s_j),     G[t,i] = c_i,     d_i <- max(d_i - c_i^2, 0).
// The pick, the downdate and their state are the greedy pivot core (pivot.h), which fvgp_hip_pchol drives too; what is selection's own
// is the conditioning on the data.  Per step, all in stream order on the handle's stream, no host round trip:
//     pivot_pick_kernel       j_t, p_t = d_j + s_j and x_j into a slot, or `done`
//     launch_kmat, potrs_vec  k(X, x_slot) into a padded n-vector and the one-right-hand-side solve in place (the existing assembly and
//                             sweeps, unchanged: they do not read `done` and after exhaustion solve for the last slot once more)
//     select_cross_kernel     the slice partials of sum_n k(x_i, X_n) w_n, lanes along candidates (slice_sum.h)
//     pivot_downdate_kernel   <KIND, CROSS = true>: slices added in ascending order, the direct term, c_i, G, d, the next partials
// the last two once per block of at most `select_block` candidates.  The row split is a function of n alone and every sum has a fixed
// order: r_i, and with it row t of G at candidate i, has the same bits whatever P is, whichever candidates share the call and wherever
// the blocks are cut.  Cross pass per entry: one exp (plus the rsq of the Matern kinds), d subtractions, d + 1 fused multiply-adds.
#include "radial.h"
#include "kernel_family.h"
#include "slice_sum.h"
#include "pivot.h"
#include <math.h>

namespace {

constexpr int64_t SEL_BLOCK_MAX = 65536;     // largest (and default) `select_block`

// the slice partials of sum_n k(x_i, X_n) w_n for the candidates [c0, c0 + cn): grid (ceil(cn / 64), slices)
template <int KIND, int D>   // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(256) void select_cross_kernel(PivotArgs a) {
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    constexpr int STAGE = SLICE_ROWS * (DD + 1);
    __shared__ double sm[STAGE];                              // the staged rows (>= 3 * 64: afterwards the sums of waves 1 .. 3)
    if (a.st->done) return;
    double *sx = sm, *sw = sm + SLICE_ROWS * DD;
    const int d = D ? D : a.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.y * SLICE_ROWS;
    const long loc = (long)blockIdx.x * 64 + lane;            // place in the block of candidates
    const long i = a.c0 + (loc < a.cn ? loc : a.cn - 1);
    slice_stage<DD>(sx, sw, a.x, a.w, 1, a.n, d, row0, tid);
    double u[DD], il[DD];                                     // (il: a copy, so that the address of the kernel's arguments is never taken)
#pragma unroll
    for (int k = 0; k < DD; ++k) { u[k] = k < d ? a.xc[i * d + k] : 0.0; il[k] = a.il[k]; }
    __syncthreads();

    const int r0 = wave * SLICE_WAVE_ROWS, rows = slice_wave_rows(a.n, row0, wave);
    double s0[1] = {0.0}, s1[1] = {0.0};
    slice_rows<KIND, DD, 1>(sx, sw, r0, rows, d, u, il, a.sig, s0, s1);
    double s = s0[0] + s1[0];

    __syncthreads();                                          // every wave is done with the staged rows
    if (wave > 0) *slice_parked(sm, 1, wave, lane) = s;
    __syncthreads();
    if (wave != 0 || loc >= a.cn) return;
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) s += *slice_parked(sm, 1, ww, lane);      // ((wave 0 + wave 1) + wave 2) + wave 3
    a.part[(long)blockIdx.y * a.pcap + loc] = s;
}

// the workspace of a selection, every piece but the last a multiple of 16 bytes: the solves' padded n-vector, the core's pieces, G (q, P),
// the slice partials.  The pointers go into the run's arguments; the solves' vector comes back writable
double *sel_layout(Carve &c, int64_t n, int64_t P, int q, PivotArgs &a) {
    a.pcap = P < SEL_BLOCK_MAX ? P : SEL_BLOCK_MAX;
    double *kvec = c.take<double>(pad128(n));
    a.w = kvec;
    pivot_layout(c, P, 3, a);
    a.G = c.take<double>((int64_t)q * P);
    a.part = c.take<double>(slice_count(n) * a.pcap, sizeof(double));
    return kvec;
}

}  // namespace

extern "C" {

int64_t fvgp_hip_select_workspace_bytes(int64_t n, int64_t P, int q) {
    if (n < 1 || P < 1 || q < 1) return -1;
    return carve_bytes_for<PivotArgs>(sel_layout, n, P, q);
}

int fvgp_hip_select_batch(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                          const double *theta, int ntheta, const double *L, int64_t ldl,
                          const double *xcand, int64_t P, const double *noise, double *var,
                          int q, int criterion, int allow_repeats, double tol,
                          double *work, int64_t work_bytes, int64_t *idx_out, double *pick_var_out, double *G_out, int64_t ldg) {
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!x) return -3;
    if (n <= 0) return -4;
    int rc = check_kernel_args(kernel_id, d, theta, ntheta, 5, 6, 7); if (rc) return rc;
    rc = check_square(L, n, ldl, 8, 4, 9);
    if (rc) return rc;
    if (!xcand) return -10;
    if (P <= 0) return -11;
    if (criterion == 1 && !noise) { fvgp_set_error("select_batch: criterion 1 needs the candidates' noise variances (all > 0)"); return -12; }
    if (!var) return -13;
    if (q < 1) return -14;
    if (criterion != 0 && criterion != 1) return -15;
    if (!(tol >= 0.0)) return -17;
    if (!work || ((uintptr_t)work & 15)) { fvgp_set_error("select_batch: work must be 16-byte aligned"); return -18; }
    Carve c(work); PivotArgs a;
    double *kvec = sel_layout(c, n, P, q, a);
    if (work_bytes < c.bytes()) {
        fvgp_set_error("select_batch: work smaller than fvgp_hip_select_workspace_bytes(n, P, q)"); return -19;
    }
    if (!idx_out) return -20;
    if (!pick_var_out) return -21;
    if (G_out && ldg < P) return -23;
    const int64_t S = slice_count(n);
    if (S > 65535) { fvgp_set_error("select_batch: n too large"); return -4; }
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    // (its own codes, numbered by fvgp_hip_kmat's arguments, cannot come back: kernel_id, d and ntheta were checked above)
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    const int64_t np = pad128(n);
    const int64_t block = h->select_block < SEL_BLOCK_MAX ? h->select_block : SEL_BLOCK_MAX;
    // the handle's own buffers (block inverses of the factor, the sweeps' vector): allocated on the first call that needs them
    rc = ensure_linv(h, L, n, ldl); if (rc) return rc;
    rc = ensure_scratch(h, np); if (rc) return rc;

    a.x = x; a.xc = xcand; a.noise = noise; a.var = var;
    a.ldg_in = P; a.Gout = G_out; a.ldg = ldg;
    a.idx = reinterpret_cast<long long *>(idx_out); a.pickv = pick_var_out;
    a.n = n; a.P = P; a.c0 = 0; a.cn = 0;
    a.d = d; a.q = q; a.t = 0; a.crit = criterion; a.repeats = allow_repeats ? 1 : 0;
    a.sig = k.sig; a.tol = tol;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.il[i] = k.invl[i];

    HIPCHK(hipMemsetAsync(kvec, 0, (size_t)np * sizeof(double), h->stream));          // the padding rows stay 0 through every step
    hipLaunchKernelGGL(pivot_init_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    for (int t = 0; t < q; ++t) {
        a.t = t;
        hipLaunchKernelGGL(pivot_pick_kernel, dim3(1), dim3(256), 0, h->stream, a);
        HIPCHK(hipGetLastError());
        // k(x_slot, X) as one row of n entries (bitwise k(X, x_slot): the scaled differences are squared), then KV^-1 of it in place
        k.x1 = a.slot; k.n1 = 1; k.x2 = x; k.n2 = n; k.vdiag = nullptr; k.K = kvec; k.ldk = np; k.uplo = FVGP_FULL; k.pad = 0;
        rc = launch_kmat(h, k); if (rc) return rc;
        rc = potrs_vec(h, L, n, ldl, kvec, 1, 1, true); if (rc) return rc;
        for (int64_t c0 = 0; c0 < P; c0 += block) {
            a.c0 = c0; a.cn = P - c0 < block ? P - c0 : block;
            const dim3 grid((unsigned)((a.cn + 63) / 64), (unsigned)S);
            dispatch_kind_dim(k.kind, d, [&](auto KIND, auto D) {
                hipLaunchKernelGGL((select_cross_kernel<decltype(KIND)::value, decltype(D)::value>), grid, dim3(256), 0, h->stream, a);
            });
            HIPCHK(hipGetLastError());
            dispatch_kind(k.kind, [&](auto KIND) {
                hipLaunchKernelGGL((pivot_downdate_kernel<decltype(KIND)::value, true>), dim3((unsigned)((a.cn + 255) / 256)), dim3(256), 0,
                                   h->stream, a, (long)S);
            });
            HIPCHK(hipGetLastError());
        }
    }
    return 0;
}

}  // extern "C"
