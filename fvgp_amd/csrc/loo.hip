// Leave-one-out cross-validation of a GP in closed form, with the exact gradient of its log predictive probability
// (fvgp_hip_loo; Rasmussen & Williams 5.4.2).  With Q = KV^-1 (POTRI), q_i = Q_ii and alpha = Q (y - m):
//     y_i - mu_i = alpha_i / q_i          sigma^2_i = 1 / q_i          L = sum_i (log q_i - alpha_i^2 / q_i) / 2 - n / 2 log 2 pi
// and with w_i = alpha_i / q_i, c_i = (1 + alpha_i^2 / q_i) / (2 q_i) > 0, u = Q w, M = Q diag(c) Q = S S^T, S = Q diag(sqrt c):
//     dL/dtheta_j = u^T dKV_j alpha - sum_kl M_kl (dKV_j)_kl = sum_kl ((u_k alpha_l + alpha_k u_l) / 2 - M_kl) (dK_j)_kl
// -- ONE symmetric N^3 product for all hyperparameters (the textbook's Z_j = Q dK_j is 2 N^3 each), on the trailing update's kernel,
// and one pass of the fused trace kernel (kmat.hip, its two-vector switch) that re-evaluates dK/dtheta in registers.
//
// Schedule on the handle's stream: POTRI -> statistics (diagonal pass) -> u = Q w from the lower-stored Q -> S over Q
// (mirror + column scaling, in place) -> M = S S^T, lower tiles, into the second square -> diag M -> trace pass -> ONE synchronisation.
// No atomics anywhere: every partial sum has its own slot and the slots are added in a fixed order, so the same inputs give the same
// bits on every run.  Rows >= n of the scratch vectors are zero, so the identity padding of Q drops out of u, S and M.
#include "common.h"
#include "kernel_family.h"
#include "reduce.h"
#include <math.h>

namespace {

// one workgroup per 128 rows: the LOO statistics of its rows and its four partial sums
//     part[4 blk ..] = { sum (log q - alpha^2 / q) / 2,  sum resid^2,  sum log q,  rows whose q is not positive and finite }
__global__ __launch_bounds__(128) void loo_stats_kernel(const double *Q, long ld, const double *alpha, int ncol, int comp, long n,
                                                        double *resid, double *var, double *w, double *c, double *sc, double *part) {
    __shared__ double s[4][128];
    const int t = threadIdx.x;
    const long i = (long)blockIdx.x * 128 + t;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, wi = 0.0, ci = 0.0, si = 0.0;
    if (i < n) {
        const double q = Q[i * ld + i], a = alpha[i * ncol + comp];
        const double r = a / q, lq = log(q), ar = a * r;
        resid[i] = r;
        var[i] = 1.0 / q;
        wi = r;
        ci = 0.5 * (1.0 + ar) / q;
        si = sqrt(ci);
        v0 = 0.5 * (lq - ar); v1 = r * r; v2 = lq;
        v3 = (q > 0.0 && q < INFINITY) ? 0.0 : 1.0;
    }
    w[i] = wi; c[i] = ci; sc[i] = si;                     // (i < padded n: the grid covers exactly the padded rows)
    s[0][t] = v0; s[1][t] = v1; s[2][t] = v2; s[3][t] = v3;
    __syncthreads();
    for (int half = 64; half > 0; half >>= 1) {           // a fixed tree
        if (t < half) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k][t] += s[k][t + half];
        }
        __syncthreads();
    }
    if (t < 4) part[(long)blockIdx.x * 4 + t] = s[t][0];
}

// u = Q w for the symmetric Q of which only the 128-tiles on and below the block diagonal are valid.  One workgroup per such tile
// (ti, tj): the tile is read ONCE, for the rows' sums (Q_rc w_c -> u_r) and, as the transposed tile, for the columns' (Q_rc w_r -> u_c);
// a diagonal tile counts its strict lower triangle both ways and its diagonal once (its upper triangle is not read as data).
// part[row][slot]: row r of tile row I gets slot tj from tile (I, tj), tj <= I, and slot ti from tile (ti, I), ti > I -- every
// (row, slot < T) is written exactly once, symv_reduce_kernel adds the slots in ascending order.
__global__ __launch_bounds__(256) void symv_lower_kernel(const double *Q, long ld, const double *w, double *part, long ldp) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (tj > ti) return;
    __shared__ double scol[4][128];
    __shared__ double srow[128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)ti * 128, col0 = (long)tj * 128;
    const bool diag = ti == tj;
    const int cl = 2 * lane;
    const double wc0 = w[col0 + cl], wc1 = w[col0 + cl + 1];
    double a0 = 0.0, a1 = 0.0;
    const double *Qp = Q + (row0 + wave) * ld + col0 + cl;
    for (int rr = wave; rr < 128; rr += 4, Qp += 4 * ld) {
        const double2_t q = *reinterpret_cast<const double2_t *>(Qp);
        double q0 = q[0], q1 = q[1];
        if (diag) { if (cl > rr) q0 = 0.0; if (cl + 1 > rr) q1 = 0.0; }
        double rs = fma(q0, wc0, q1 * wc1);
        const double wr = w[row0 + rr];
        double t0 = q0, t1 = q1;
        if (diag) { if (cl == rr) t0 = 0.0; if (cl + 1 == rr) t1 = 0.0; }
        a0 = fma(t0, wr, a0); a1 = fma(t1, wr, a1);
        rs = wave_sum(rs);
        if (lane == 0) srow[rr] = rs;
    }
    scol[wave][cl] = a0; scol[wave][cl + 1] = a1;
    __syncthreads();
    if (tid < 128) {
        const double cs = (scol[0][tid] + scol[1][tid]) + (scol[2][tid] + scol[3][tid]);
        if (diag) part[(row0 + tid) * ldp + ti] = srow[tid] + cs;
        else { part[(row0 + tid) * ldp + tj] = srow[tid]; part[(col0 + tid) * ldp + ti] = cs; }
    }
}

__global__ __launch_bounds__(256) void symv_reduce_kernel(const double *part, long ldp, int T, long n, double *u) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < T; ++k) s += part[i * ldp + k];
    u[i] = s;
}

// S = mirror(Q) diag(sc) in place: a workgroup per 128-tile on or below the block diagonal reads the tile in 32 x 32 pieces and writes
// each piece scaled by the sc of its columns and, transposed, the piece of the mirrored tile scaled by the sc of ITS columns.  Only
// pieces on and below the diagonal are ever read, only this workgroup writes them and their mirrors: in place is safe.
__global__ __launch_bounds__(256) void mirror_scale_kernel(double *Q, long ld, const double *sc) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (tj > ti) return;
    __shared__ double t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int p = 0; p < 16; ++p) {
        const int bi = p >> 2, bj = p & 3;
        if (ti == tj && bj > bi) continue;
        const long r0 = (long)ti * 128 + bi * 32, c0 = (long)tj * 128 + bj * 32;
        const bool dg = ti == tj && bi == bj;
        for (int rr = ty; rr < 32; rr += 8) t[rr][tx] = Q[(r0 + rr) * ld + c0 + tx];
        __syncthreads();
        const double scc = sc[c0 + tx], scr = sc[r0 + tx];
        for (int rr = ty; rr < 32; rr += 8) {
            const double v = (dg && tx > rr) ? t[tx][rr] : t[rr][tx];
            Q[(r0 + rr) * ld + c0 + tx] = v * scc;
            if (!dg) Q[(c0 + rr) * ld + r0 + tx] = t[tx][rr] * scr;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void diag_copy_kernel(const double *M, long ldm, long n, double *out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = M[i * ldm + i];
}

constexpr long double LOG_2PI = 1.8378770664093454835606594728112353L;

}  // namespace

int launch_loo_stats(fvgp_handle *h, const double *Q, int64_t ld, const double *alpha, int ncol, int component, int64_t n, int64_t np,
                     double *resid, double *var, double *w, double *c, double *sc, double *part) {
    hipLaunchKernelGGL(loo_stats_kernel, dim3((unsigned)(np / TILE)), dim3(128), 0, h->stream, Q, (long)ld, alpha, ncol, component, (long)n,
                       resid, var, w, c, sc, part);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_symv_lower(fvgp_handle *h, const double *Q, int64_t ld, int64_t np, const double *w, double *part, int64_t ldp, int64_t n, double *u) {
    const unsigned T = (unsigned)(np / TILE);
    hipLaunchKernelGGL(symv_lower_kernel, dim3(T, T), dim3(256), 0, h->stream, Q, (long)ld, w, part, (long)ldp);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(symv_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const double *)part, (long)ldp, (int)T, (long)n, u);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_mirror_scale(fvgp_handle *h, double *Q, int64_t ld, int64_t np, const double *sc) {
    const unsigned T = (unsigned)(np / TILE);
    hipLaunchKernelGGL(mirror_scale_kernel, dim3(T, T), dim3(256), 0, h->stream, Q, (long)ld, sc);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_diag_copy(fvgp_handle *h, const double *M, int64_t ldm, int64_t n, double *out) {
    hipLaunchKernelGGL(diag_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, M, (long)ldm, (long)n, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// fvgp_hip_loo's vector scratch: w, c, sqrt c (padded n each); four partial sums per 128 rows
struct LooWs { double *w, *c, *sc, *spart; };
static LooWs loo_layout(Carve &cv, int64_t n) {
    const int64_t np = pad128(n);
    return {cv.take<double>(np, 8), cv.take<double>(np, 8), cv.take<double>(np, 8), cv.take<double>(4 * (np / TILE), 8)};
}

extern "C" {

int64_t fvgp_hip_loo_workspace_bytes(int64_t n) {
    if (n < 1) return -1;
    return carve_bytes(loo_layout, n);
}

int fvgp_hip_loo(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d,
                 const double *theta, int ntheta, const double *alpha, int ncol, int component,
                 double *KV, int64_t ld, double *work, int64_t ldw, double *ws, int64_t ws_bytes,
                 double *out_host, double *resid_out, double *var_out,
                 double *grad_host, double *u_out, double *mdiag_out) {
    if (!h) return -1;
    if (grad_host && !x) return -3;
    if (n <= 0) return -4;
    if (grad_host && !theta) return -6;
    if (!alpha) return -8;
    if (ncol < 1) return -9;
    if (component < 0 || component >= ncol) { fvgp_set_error("loo: 0 <= component < ncol"); return -10; }
    int rc = check_square(KV, n, ld, 11, 4, 12);
    if (rc) return rc;
    rc = check_square(work, n, ldw, 13, 4, 14);
    if (rc) return rc;
    if (!ws || ((uintptr_t)ws & 7)) return -15;
    Carve cv(ws); const LooWs l = loo_layout(cv, n);
    if (ws_bytes < cv.bytes()) { fvgp_set_error("loo: ws smaller than fvgp_hip_loo_workspace_bytes(n)"); return -16; }
    if (!out_host) return -17;
    if (!resid_out) return -18;
    if (!var_out) return -19;
    if (grad_host && !u_out) return -21;
    if (grad_host && !mdiag_out) return -22;
    GradDesc g{};
    int nk = 0;
    if (grad_host) {
        rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &g.k); if (rc) return rc;
        nk = kernel_param_count(kernel_id, d);
    }
    HIPCHK(hipSetDevice(h->device));
    const int64_t np = pad128(n), T = np / TILE;

    rc = fvgp_hip_potri(h, KV, n, ld, work, ldw); if (rc) return rc;                     // Q in the lower tiles of KV; `work` is dead
    rc = launch_loo_stats(h, KV, ld, alpha, ncol, component, n, np, resid_out, var_out, l.w, l.c, l.sc, l.spart); if (rc) return rc;
    std::vector<double> sp((size_t)(4 * T)), part;
    HIPCHK(hipMemcpyAsync(sp.data(), l.spart, sp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    int nblocks = 0;
    if (grad_host) {
        // the per-row slots of u = Q w live in `work` (np rows of T <= ldw slots) until M takes it over
        rc = launch_symv_lower(h, KV, ld, np, l.w, work, ldw, n, u_out); if (rc) return rc;
        rc = launch_mirror_scale(h, KV, ld, np, l.sc); if (rc) return rc;                  // KV <- S = Q diag(sqrt c), full
        rc = launch_gemm(h, gemm_desc(0, 0, np, np, np, 1.0, KV, ld, KV, ld, 0.0, work, ldw).lower_tiles()); if (rc) return rc;   // M = S S^T
        rc = launch_diag_copy(h, work, ldw, n, mdiag_out); if (rc) return rc;
        g.k.x1 = x; g.k.n1 = n; g.k.x2 = x; g.k.n2 = n;
        g.ntheta = nk;
        g.W = work; g.ldw = ldw; g.b = alpha + component; g.ldb = ncol; g.b2 = u_out; g.ldb2 = 1;
        g.partial = KV;                                                                  // S is dead: the tiles' partial sums go there
        rc = launch_grad_trace(h, g, &nblocks); if (rc) return rc;
        part.resize((size_t)nblocks * nk);
        HIPCHK(hipMemcpyAsync(part.data(), KV, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    rc = fvgp_ipc_check(h); if (rc) return rc;
    long double s0 = 0.0L, s1 = 0.0L, s2 = 0.0L, bad = 0.0L;
    for (int64_t b = 0; b < T; ++b) { s0 += sp[4 * b]; s1 += sp[4 * b + 1]; s2 += sp[4 * b + 2]; bad += sp[4 * b + 3]; }
    const bool ok = bad == 0.0L;
    out_host[0] = ok ? (double)(s0 - 0.5L * (long double)n * LOG_2PI) : NAN;
    out_host[1] = ok ? (double)s1 : NAN;
    out_host[2] = ok ? (double)s2 : NAN;
    out_host[3] = (double)bad;
    if (grad_host) {
        for (int i = 0; i < ntheta; ++i) grad_host[i] = 0.0;
        // the trace pass sums w_jk (M_jk - (alpha_j u_k + u_j alpha_k) / 2) dK_jk over the lower triangle = MINUS the gradient
        for (int i = 0; i < nk; ++i) {
            long double s = 0.0L;
            for (int bb = 0; bb < nblocks; ++bb) s += part[(size_t)bb * nk + i];
            grad_host[i] = ok ? -(double)s : NAN;
        }
    }
    return 0;
}

}  // extern "C"
