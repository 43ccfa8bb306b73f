// The m x m linear algebra of the nearest-neighbour (Vecchia) path (include/fvgp_hip_nn.h): n independent m x m problems,
// m <= 64, instead of one n x n.  The neighbour lists come from nn_search.hip or nn_grid.hip; only dispatch_pad is shared with them.
// fvgp_hip_nn_conditionals  one wavefront per (row, b), NN_WAVES of them per workgroup and nothing shared between them: lane l owns
//     neighbour l.  Assembly: for column j the lanes read x_j from lane j's registers (v_readlane, j is uniform) and lanes l >= j store
//     K(x_l, x_j) into the packed lower triangle held COLUMN-major in LDS (column j: rows j .. M - 1, consecutive lanes on consecutive
//     addresses).  Factorisation: left-looking, column by column, lane l accumulating its entry of the column over the earlier columns
//     (own entries conflict-free, row j's entries broadcast); the pivot leaves lane j by v_readlane, and both right-hand sides (k and
//     r_c, a register each) are substituted in the same step.  Padded lanes are identity rows.
// fvgp_hip_nn_loglik, _loglik_grad, _loglik_fisher   one host path (nn_loglik, one workspace layout: nn_layout) at the levels NN_VALUE,
//     NN_GRAD, NN_FISHER: the conditionals on the data itself in the level's mode of the kernel, then the sums.
//     NN_GRAD: the kernel goes on from the factor in LDS (a backward pass for A^-1 k and A^-1 r_c, one more sweep over the
//     block's entries with their derivatives) and writes every row's score.  NN_FISHER: it goes on after the score (a full-row
//     sweep of derivatives, a forward pass with every right-hand side, the pairwise products) and writes every row's packed term.
//     The sums (nn_sum_columns: the likelihood's two terms, the scores' columns, the packed entries): slices of 256 rows by a halving tree in
//     LDS, the slices to 0 in ascending order by one thread per (b, column).  No atomics anywhere.  The triangle is mirrored on the host.
#include "radial.h"
#include "kernel_family.h"
#include "reduce.h"
#include "nn_geometry.h"
#include "../../include/fvgp_hip_nn.h"
#include <math.h>
#include <vector>

namespace {

constexpr int NN_WAVES = 4;                       // conditionals: waves (problems) per workgroup
constexpr int NN_TAB = 1 + FVGP_MAX_DIM;          // theta table row: sigma^2, then 1 / l per dimension
constexpr int NN_SUM_ROWS = 256;                 // rows per slice of the likelihood's sums

// LDS traffic between the lanes of ONE wave: the wave's DS operations execute in order, the fences keep the compiler from moving them
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane j's v in every lane (j wave-uniform)
__device__ __forceinline__ double lane_value(const double v, const int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

// the level of a likelihood call, and what nn_cond_kernel computes beside mu and var: nothing, every row's score, or the score and the
// row's Fisher information.  NN_FACTOR is no likelihood level: the kernel stops behind the backward pass and writes the row of the sparse
// inverse Cholesky factor (fvgp_hip_nn_factor)
constexpr int NN_VALUE = 0, NN_GRAD = 1, NN_FISHER = 2, NN_FACTOR = 3;

// f(std::integral_constant<int, MODE>) for the level
template <class F>
inline void dispatch_mode(int level, F &&f) {
    if (level == NN_FACTOR) f(std::integral_constant<int, NN_FACTOR>{});
    else if (level == NN_FISHER) f(std::integral_constant<int, NN_FISHER>{});
    else if (level == NN_GRAD) f(std::integral_constant<int, NN_GRAD>{});
    else f(std::integral_constant<int, NN_VALUE>{});
}

// ------------------------------------------------------------------------------------------------------------ conditionals
struct NcArgs {
    const double *xq, *xr, *r, *v, *s, *tab;       // tab (B, NN_TAB)
    const int *idx;
    double *mu, *var;
    long nq, nr, ld;
    int d, m;
    double *score;                                 // GRAD: (B, nq, nth), the row's d log p(y_i | y_c) / d theta
    int nth, iso;                                  // GRAD: columns of score; one length scale for every dimension
    double *fisher;                                // NN_FISHER: (B, nq, nth (nth + 1) / 2), the row's term of the Fisher information, packed lower
    double *coef, *dinv; long ldc;                 // NN_FACTOR: (nq, ldc) and (nq), the row of W; r and mu are NULL there and var is d
};

// GRAD: the likelihood's conditionals (xq == xr, s == v) and each row's score.  Everything up to mu and var is the value kernel's code,
// the same operations in the same order; the factor is still in LDS when they are done, and the score needs no second factorisation:
// a = L^-T w = A^-1 k and beta = L^-T z = A^-1 r_c by one backward pass, then one more sweep over the kernel entries of the block of
// (c, i) with their derivatives, each weighted by b_p q_q' + b_q' q_p (include/fvgp_hip_nn.h has the formula).
//
// NN_FISHER: the row's term F_i of the Fisher information of the product of conditionals, E[-d^2 log p(y_i | y_c)], after the
// score and from the same factor.  With dS = dSigma / d theta_h:  t_h = (dS b) on the neighbours (one full-row sweep over the block's
// entries: the lanes the score's sweep masks take part), delta_h = b^T dS b = d var / d theta_h, u_h = L^-1 t_h (every right-hand side in
// one forward pass), F_i[h][k] = u_h^T u_k / var + 1/2 delta_h delta_k / var^2.  It reads x, v, theta and the lists, never r.
//
// NN_FACTOR: the value path (xq == xr, s == v) and the backward pass for a = A^-1 k, then the row of the sparse inverse
// Cholesky factor, dinv = 1 / sqrt(var) and coef = -(a dinv); it stops there, never reads r and writes no mu (var goes to the workspace).
template <int KIND, int D, int M, int MODE>    // D == 0: runtime dimension; M: the padded block, m <= M
__global__ __launch_bounds__(64 * NN_WAVES) void nn_cond_kernel(NcArgs a) {
    constexpr bool GRAD = MODE >= NN_GRAD;
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    constexpr int TRI = M * (M + 1) / 2;
    __shared__ double sm_all[NN_WAVES * TRI];
    const int d = D ? D : a.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * NN_WAVES + wave;
    if (row >= a.nq) return;                       // (no workgroup barrier below: the waves share nothing)
    const long b = blockIdx.y;
    double *sm = sm_all + wave * TRI;
    const double *tab = a.tab + b * NN_TAB;
    const double sig = tab[0];
    double il[DD], u[DD], xi[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) { il[k] = k < d ? tab[1 + k] : 0.0; xi[k] = k < d ? a.xq[row * d + k] : 0.0; }
    // lane l's neighbour; a lane without one (past m, or an index outside the reference rows) is an identity row
    long c = -1;
    if (lane < a.m) c = a.idx[row * a.ld + lane];
    const bool valid = c >= 0 && c < a.nr;
    const long cc = valid ? c : 0;
#pragma unroll
    for (int k = 0; k < DD; ++k) u[k] = k < d ? a.xr[cc * d + k] : 0.0;
    const double vc = valid ? a.v[cc] : 0.0;
    double tz = (MODE != NN_FACTOR && valid) ? a.r[cc] : 0.0;      // becomes z_l
    double tw = 0.0;                               // k_l = k(x_c, x_i), becomes w_l
    {
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < d) { const double e = (u[k] - xi[k]) * il[k]; r2 = fma(e, e, r2); }
        const double kv = radial<KIND>(r2, sig);
        if (valid) tw = kv;
    }
    const unsigned long long vmask = __ballot(valid);

    // assembly: column j of the lower triangle at sm[col + l], col = off(j) - j, off(j) = j M - j (j - 1) / 2
    for (int j = 0, col = 0; j < M; col += M - j - 1, ++j) {
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < d) { const double e = (u[k] - lane_value(u[k], j)) * il[k]; r2 = fma(e, e, r2); }
        double kv = radial<KIND>(r2, sig);
        const bool vj = (vmask >> j) & 1ull;
        if (lane == j) kv = valid ? kv + vc : 1.0;
        else if (!(valid && vj)) kv = 0.0;
        if (lane >= j && lane < M) sm[col + lane] = kv;
    }
    wave_sync();

    // factorisation and both substitutions
    bool fail = false;
    double linv = 1.0;                             // GRAD: 1 / L_ll (the diagonal slots of sm keep A's diagonal)
    for (int j = 0, col = 0; j < M; col += M - j - 1, ++j) {
        const int lr = lane < j ? j : (lane < M ? lane : M - 1);       // (lanes outside the column repeat a row of it: every read stays inside the triangle)
        double sacc = sm[col + lr];
        for (int k = 0, ck = 0; k < j; ck += M - k - 1, ++k) sacc = fma(-sm[ck + lr], sm[ck + j], sacc);
        double p = lane_value(sacc, j);
        if (!(p > 0.0)) { fail = true; p = 1.0; }
        const double ljj = sqrt(p), inv = 1.0 / ljj;
        const double lc = sacc * inv;
        if (lane > j && lane < M) sm[col + lane] = lc;
        if (GRAD && lane == j) linv = inv;
        const double wj = lane_value(tw, j) * inv, zj = lane_value(tz, j) * inv;
        if (lane == j) { tw = wj; tz = zj; }
        else if (lane > j) { tw = fma(-lc, wj, tw); tz = fma(-lc, zj, tz); }
        wave_sync();
    }
    if (lane >= M) { tw = 0.0; tz = 0.0; }
    const double mu = wave_sum(tw * tz), ww = wave_sum(tw * tw);
    if (lane == 0) {
        double kxx = radial<KIND>(0.0, sig);
        if (a.s) kxx += a.s[row];
        if (MODE != NN_FACTOR) a.mu[b * a.nq + row] = fail ? NAN : mu;
        a.var[b * a.nq + row] = fail ? NAN : kxx - ww;
    }
    if constexpr (GRAD) {
        // L^T a = w and L^T beta = z in one pass, outer-product form: step j takes a_j, beta_j from lane j and the lanes l < j subtract
        // L[j][l] times them (row j of the factor: lane l reads its own column at row j).  No reduction, the order is j = M - 1 .. 0.
        const int mycol = lane * M - lane * (lane + 1) / 2;      // (only lanes < j <= M - 1 read)
        double ta = tw, tb = tz;
        for (int j = M - 1; j >= 0; --j) {
            const double aj = lane_value(ta * linv, j), bj = lane_value(tb * linv, j);
            if (lane == j) { ta = aj; tb = bj; }
            else if (lane < j) { const double l = sm[mycol + j]; ta = fma(-l, aj, ta); tb = fma(-l, bj, tb); }
        }
        double kxx = radial<KIND>(0.0, sig);
        if (a.s) kxx += a.s[row];
        if constexpr (MODE == NN_FACTOR) {
            const double di = 1.0 / sqrt(kxx - lane_value(ww, 0));
            if (lane < a.m) a.coef[row * a.ldc + lane] = fail ? NAN : valid ? -(ta * di) : 0.0;
            if (lane == 0) a.dinv[row] = fail ? NAN : di;
            return;
        }
        const double dv = kxx - lane_value(ww, 0), e = a.r[row] - lane_value(mu, 0);
        const double ed = e / dv, c2 = 0.5 * (ed * ed - 1.0 / dv);
        // b = (-a, 1), q = (e / d) (beta, 0) + c2 b: this lane's entries; the entry of x_i itself is (1, c2)
        const double bl = -ta, ql = fma(ed, tb, c2 * bl);
        double acc[1 + DD];
#pragma unroll
        for (int k = 0; k <= DD; ++k) acc[k] = 0.0;
        const bool iso = a.iso != 0;
        // column j < M: the entries (l, j), l > j, of the neighbours' block; column M: those of (l, i).  Lanes without a neighbour and
        // columns without one take no part.
        for (int j = 0; j <= M; ++j) {
            const bool self = j == M;
            const int jl = self ? 0 : j;           // (a lane to read that exists; its values are not used for x_i's column)
            if (!self && !((vmask >> j) & 1ull)) continue;
            const double wgt = self ? fma(bl, c2, ql) : fma(bl, lane_value(ql, jl), lane_value(bl, jl) * ql);
            double ek[DD], r2 = 0.0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                ek[k] = 0.0;
                if (k < d) { ek[k] = (u[k] - (self ? xi[k] : lane_value(u[k], jl))) * il[k]; r2 = fma(ek[k], ek[k], r2); }
            }
            double phi, cf;
            radial_grad<KIND>(r2, sig, phi, cf);
            if (valid && (self || lane > j)) {
                acc[0] = fma(wgt, phi, acc[0]);
                const double wc = wgt * cf;
                if (iso) acc[1] = fma(wc, r2 * il[0], acc[1]);
                else {
#pragma unroll
                    for (int k = 0; k < DD; ++k)
                        if (k < d) acc[1 + k] = fma(wc, ek[k] * ek[k] * il[k], acc[1 + k]);
                }
            }
        }
        if (valid) acc[0] = fma(bl, ql, acc[0]);   // the diagonal: d Sigma[p][p] = 1 for sigma^2, 0 for the length scales
        const int np = iso ? 2 : d + 1;
        double *out = a.score + (b * a.nq + row) * a.nth;
#pragma unroll
        for (int h = 0; h <= DD; ++h)
            if (h < np) {
                double s = wave_sum(acc[h]);
                if (h == 0) s += c2;               // the diagonal entry of x_i itself
                if (lane == 0) out[h] = fail ? NAN : s;
            }
        if (lane == 0)
            for (int h = np; h < a.nth; ++h) out[h] = 0.0;

        if constexpr (MODE == NN_FISHER) {
            double t[1 + DD], dlt[1 + DD];         // t_h: this lane's entry of dS_h b, then of L^-1 of it; delta_h (lane 0's is the sum)
#pragma unroll
            for (int h = 0; h <= DD; ++h) { t[h] = 0.0; dlt[h] = 0.0; }
            // the neighbours' block, every entry (l, j), l != j, times b_j: the row of a symmetric matrix needs both triangles
            for (int j = 0; j < M; ++j) {
                if (!((vmask >> j) & 1ull)) continue;
                const double bj = lane_value(bl, j);
                double ek[DD], r2 = 0.0;
#pragma unroll
                for (int k = 0; k < DD; ++k) {
                    ek[k] = 0.0;
                    if (k < d) { ek[k] = (u[k] - lane_value(u[k], j)) * il[k]; r2 = fma(ek[k], ek[k], r2); }
                }
                double phi, cf;
                radial_grad<KIND>(r2, sig, phi, cf);
                if (valid && lane != j) {
                    t[0] = fma(bj, phi, t[0]);
                    const double wc = bj * cf;
                    if (iso) t[1] = fma(wc, r2 * il[0], t[1]);
                    else {
#pragma unroll
                        for (int k = 0; k < DD; ++k)
                            if (k < d) t[1 + k] = fma(wc, ek[k] * ek[k] * il[k], t[1 + k]);
                    }
                }
            }
            if (valid) t[0] += bl;                 // the diagonal of the block: d Sigma[p][p] = 1 for sigma^2, 0 for the length scales
            // the column of x_i (b = 1 there) closes t, and delta_h = sum_l b_l (t_h[l] + dk_h[l]) + d Sigma[i][i]
            {
                double ek[DD], r2 = 0.0;
#pragma unroll
                for (int k = 0; k < DD; ++k) {
                    ek[k] = 0.0;
                    if (k < d) { ek[k] = (u[k] - xi[k]) * il[k]; r2 = fma(ek[k], ek[k], r2); }
                }
                double phi, cf;
                radial_grad<KIND>(r2, sig, phi, cf);
#pragma unroll
                for (int h = 0; h <= DD; ++h)
                    if (h < np) {
                        double dk = phi;           // d k(x_l, x_i) / d theta_h
                        if (h > 0) dk = iso ? cf * (r2 * il[0]) : cf * (ek[h ? h - 1 : 0] * ek[h ? h - 1 : 0] * il[h ? h - 1 : 0]);
                        double s = 0.0;
                        if (valid) { t[h] += dk; s = bl * (t[h] + dk); }
                        s = wave_sum(s);
                        dlt[h] = h == 0 ? s + 1.0 : s;
                    }
            }
            // L u_h = t_h for every h at once: step j takes u_h[j] from lane j, the lanes l > j subtract L[l][j] times it (the column the
            // factorisation wrote); lanes without a neighbour carry 0 and are identity rows
            for (int j = 0, col = 0; j < M; col += M - j - 1, ++j) {
                double l = 0.0;
                if (lane > j && lane < M) l = sm[col + lane];
#pragma unroll
                for (int h = 0; h <= DD; ++h)
                    if (h < np) {
                        const double uj = lane_value(t[h] * linv, j);
                        if (lane == j) t[h] = uj;
                        else if (lane > j && lane < M) t[h] = fma(-l, uj, t[h]);
                    }
            }
            // F_i[h][k] = u_h^T u_k / var + 1/2 delta_h delta_k / var^2, (h, k <= h) at h (h + 1) / 2 + k
            double *fo = a.fisher + (b * a.nq + row) * ((long)a.nth * (a.nth + 1) / 2);
#pragma unroll
            for (int h = 0; h <= DD; ++h)
                if (h < np) {
#pragma unroll
                    for (int k = 0; k <= h; ++k) {
                        const double s = wave_sum(t[h] * t[k]);
                        if (lane == 0) fo[h * (h + 1) / 2 + k] = fail ? NAN : s / dv + 0.5 * (dlt[h] / dv) * (dlt[k] / dv);
                    }
                }
            if (lane == 0)
                for (int e = np * (np + 1) / 2; e < a.nth * (a.nth + 1) / 2; ++e) fo[e] = 0.0;
        }
    }
}

// info <- 0 or 1 + the first e in [0, total) with var[e] not positive: one workgroup, each thread the smallest of its stride, then a
// halving tree of minima
__global__ __launch_bounds__(256) void nn_info_kernel(const double *var, long total, long long *info) {
    __shared__ long long sm[256];
    const int tid = threadIdx.x;
    long long first = 0x7fffffffffffffffLL;
    for (long e = tid; e < total; e += 256)
        if (!(var[e] > 0.0)) { first = e; break; }
    sm[tid] = first;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off && sm[tid + off] < sm[tid]) sm[tid] = sm[tid + off];
        __syncthreads();
    }
    if (tid == 0) *info = sm[0] == 0x7fffffffffffffffLL ? 0 : sm[0] + 1;
}

// --------------------------------------------------------------------------------------------------- the sums over the rows
// where the W columns c .. c + W - 1 of row (b, i) come from: a (B, n, ncol) array (the scores, the Fisher rows), a column at a time ...
struct NnColumns {
    static constexpr int W = 1;
    const double *src;
    __device__ void operator()(long b, long i, int c, long n, int ncol, double *t) const { t[0] = src[(b * n + i) * ncol + c]; }
};
// ... or the likelihood's pair, formed here and summed together: column 0 (r - mu)^2 / var, column 1 log var
struct NnLikTerms {
    static constexpr int W = 2;
    const double *r, *mu, *var;
    __device__ void operator()(long b, long i, int, long n, int, double *t) const {
        const double dv = var[b * n + i], e = r[i] - mu[b * n + i];
        t[0] = e * e / dv;
        t[1] = log(dv);
    }
};

// part[(b * nslices + slice) * ncol + c] = the slice's sum of column c: a halving tree over 256 rows, W columns at a time (W divides ncol) ...
template <class S>
__global__ __launch_bounds__(NN_SUM_ROWS) void nn_slice_sum_kernel(S src, long n, int ncol, double *part) {
    constexpr int W = S::W;
    __shared__ double sf[W][NN_SUM_ROWS];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * NN_SUM_ROWS + tid, b = blockIdx.y;
    for (int c = 0; c < ncol; c += W) {
        double t[W] = {};
        if (i < n) src(b, i, c, n, ncol, t);
#pragma unroll
        for (int w = 0; w < W; ++w) sf[w][tid] = t[w];
        __syncthreads();
        for (int off = NN_SUM_ROWS / 2; off > 0; off >>= 1) {
            if (tid < off) {
#pragma unroll
                for (int w = 0; w < W; ++w) sf[w][tid] += sf[w][tid + off];
            }
            __syncthreads();
        }
        if (tid == 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) part[(b * gridDim.x + blockIdx.x) * ncol + c + w] = sf[w][0];
        }
        __syncthreads();                           // (sf[.][0] has been read before the next columns overwrite it)
    }
}

// ... and out[b][c] = the slices added to 0 in ascending order, one thread per (b, c).  LIK (ncol == 2, the likelihood's pair):
// out[b] = {log p, fit, logdet} instead, log p by the thread of fit, which takes logdet from the lane beside it
template <bool LIK>
__global__ __launch_bounds__(64) void nn_total_kernel(const double *part, long nslices, int ncol, long count, long n, double *out) {
    const long e = (long)blockIdx.x * 64 + threadIdx.x;
    const long b = e / ncol, c = e - b * ncol;
    double s = 0.0;
    if (e < count)
        for (long sl = 0; sl < nslices; ++sl) s += part[(b * nslices + sl) * ncol + c];
    if (!LIK) {
        if (e < count) out[e] = s;
        return;
    }
    const double f = s, l = __shfl_down(s, 1, 64);
    if (e < count) out[b * 3 + 1 + c] = s;
    if (e < count && c == 0) out[b * 3] = -0.5 * (f + l + (double)n * 1.8378770664093454836);      // log 2 pi
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline int64_t nn_slices(int64_t n) { return (n + NN_SUM_ROWS - 1) / NN_SUM_ROWS; }
inline int64_t nn_packed(int ntheta) { return (int64_t)ntheta * (ntheta + 1) / 2; }

// all a conditionals call takes, and the head of every other workspace of this unit: the info word in the first 16 bytes (where the
// caller's buffer begins), `tab` the theta table
struct NnCondWs { long long *info; double *tab; };
NnCondWs nn_cond_layout(Carve &c, int B) {
    return {c.take<long long>(1), c.take<double>((int64_t)B * NN_TAB)};
}

// the likelihood's, every result piece 16-byte aligned and the sums behind it packed: `out` the three results per b, `part` the pair's
// sums per (b, slice); from NN_GRAD: `grad` (B, ntheta), `gpart` the scores' sums per (b, slice, column); at NN_FISHER: `fis` (B, P)
// packed, `fpart` the rows' sums per (b, slice, entry).  A level's layout is the one below it and its own two pieces behind.
struct NnWs { NnCondWs cond; double *out, *part, *grad, *gpart, *fis, *fpart; };
NnWs nn_layout(Carve &c, int level, int64_t n, int B, int ntheta) {
    const int64_t sums = (int64_t)B * nn_slices(n);
    NnWs l{};
    l.cond = nn_cond_layout(c, B);
    l.out = c.take<double>((int64_t)B * 3); l.part = c.take<double>(2 * sums, sizeof(double));
    if (level >= NN_GRAD) { l.grad = c.take<double>((int64_t)B * ntheta); l.gpart = c.take<double>(sums * ntheta, sizeof(double)); }
    if (level >= NN_FISHER) { l.fis = c.take<double>((int64_t)B * nn_packed(ntheta)); l.fpart = c.take<double>(sums * nn_packed(ntheta), sizeof(double)); }
    return l;
}

// the factor's: the conditionals' of one vector, then the n conditional variances
struct NnFactorWs { NnCondWs cond; double *dvar; };
NnFactorWs nn_factor_layout(Carve &c, int64_t n) {
    return {nn_cond_layout(c, 1), c.take<double>(n, sizeof(double))};
}

// the theta table of B hyperparameter vectors into work, the conditionals over it at `level` and the info word; nothing is read back.
// score (B, nq, ntheta) from NN_GRAD and fisher (B, nq, P) at NN_FISHER, else NULL (the likelihood's structure only: xq == xr, s == v)
int nn_run_conditionals(fvgp_handle *h, int level, int kernel_id, const double *xq, int64_t nq, const double *xr, int64_t nr, int d,
                        const double *thetas, int ntheta, int B, const int *idx, int64_t ld, int m, const double *r, const double *v,
                        const double *s, double *mu, double *var, const NnCondWs &w, double *score, double *fisher,
                        double *coef = nullptr, int64_t ldc = 0, double *dinv = nullptr) {
    std::vector<double> tab((size_t)B * NN_TAB);
    KmatDesc k{};
    for (int b = 0; b < B; ++b) {
        const int rc = kmat_desc_from_theta(kernel_id, d, thetas + (size_t)b * ntheta, ntheta, &k);
        if (rc) return rc;
        tab[(size_t)b * NN_TAB] = k.sig;
        for (int i = 0; i < FVGP_MAX_DIM; ++i) tab[(size_t)b * NN_TAB + 1 + i] = k.invl[i];
    }
    double *tab_dev = w.tab;
    HIPCHK(hipMemcpyAsync(tab_dev, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));       // (the table leaves this frame)
    NcArgs a;
    a.xq = xq; a.xr = xr; a.r = r; a.v = v; a.s = s; a.tab = tab_dev; a.idx = idx; a.mu = mu; a.var = var;
    a.nq = nq; a.nr = nr; a.ld = ld; a.d = d; a.m = m;
    a.score = score; a.nth = ntheta; a.iso = KERNEL_FAMILY[kernel_id].iso ? 1 : 0;
    a.fisher = fisher;
    a.coef = coef; a.ldc = ldc; a.dinv = dinv;
    const dim3 grid((unsigned)((nq + NN_WAVES - 1) / NN_WAVES), (unsigned)B), block(64 * NN_WAVES);
    dispatch_kind_dim(k.kind, d, [&](auto KIND, auto D) {
        dispatch_pad(m, [&](auto M) {
            dispatch_mode(level, [&](auto MODE) {
                hipLaunchKernelGGL((nn_cond_kernel<decltype(KIND)::value, decltype(D)::value, decltype(M)::value, decltype(MODE)::value>), grid, block, 0,
                                   h->stream, a);
            });
        });
    });
    HIPCHK(hipGetLastError());
    HIPLAUNCH(nn_info_kernel, dim3(1), dim3(256), h->stream, (const double *)var, (long)(nq * B), w.info);
    return 0;
}

// the slices' sums of `source`'s ncol columns over n rows into part (B, slices, ncol), and their totals into `total`
template <class S>
int nn_sum_columns(hipStream_t stream, S source, int64_t n, int ncol, int B, double *part, double *total) {
    const int64_t ns = nn_slices(n);
    const long count = (long)B * ncol;
    HIPLAUNCH(nn_slice_sum_kernel<S>, dim3((unsigned)ns, (unsigned)B), dim3(NN_SUM_ROWS), stream, source, (long)n, ncol, part);
    constexpr bool LIK = std::is_same<S, NnLikTerms>::value;
    HIPLAUNCH(nn_total_kernel<LIK>, dim3((unsigned)((count + 63) / 64)), dim3(64), stream, (const double *)part,
              (long)ns, ncol, count, (long)n, total);
    return 0;
}

// The three likelihood entries (include/fvgp_hip_nn.h): `level` says how far the call goes, `who` is the entry's name in its error texts.
// An error is minus the argument's position in THAT entry: score and grad_host exist from NN_GRAD, fisher_rows and fisher_host at
// NN_FISHER, and the positions behind them shift with the level.  Nothing is launched or written before the last check has passed.
int nn_loglik(int level, const std::string &who, fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *thetas_host,
              int ntheta, int B, const int *idx, int64_t ld, int m, const double *r, const double *v, double *mu, double *var, double *score,
              double *fisher_rows, double *work, int64_t work_bytes, double *out_host, double *grad_host, double *fisher_host,
              int64_t *info_host) {
    static const char *const sizing[] = {"fvgp_hip_nn_workspace_bytes(FVGP_NN_LOGLIK, n, B)", "fvgp_hip_nn_grad_workspace_bytes(n, B, ntheta)",
                                         "fvgp_hip_nn_fisher_workspace_bytes(n, B, ntheta)"};
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!x) return -3;
    if (n < 1 || n > 0x7fffffffLL) return -4;
    int rc = check_kernel_args(kernel_id, d, thetas_host, ntheta, 5, 6, 7); if (rc) return rc;
    if (B < 1 || B > 65535) { fvgp_set_error(who + ": 1 .. 65535 hyperparameter vectors per call"); return -8; }
    if (!idx) return -9;
    if (m < 1 || m > FVGP_NN_MAX_NEIGHBORS) { fvgp_set_error(who + ": 1 .. FVGP_NN_MAX_NEIGHBORS neighbours"); return -11; }
    if (ld < m) return -10;
    if (!r) return -12;
    if (!v) return -13;
    if (!mu) return -14;
    if (!var) return -15;
    if (level >= NN_GRAD && !score) return -16;
    if (level == NN_FISHER && !fisher_rows) return -17;
    const int at = 15 + level;                     // the last device array's position: var, score or fisher_rows
    if (!work || ((uintptr_t)work & 7)) return -(at + 1);
    Carve c(work); const NnWs l = nn_layout(c, level, n, B, ntheta);
    if (work_bytes < c.bytes()) { fvgp_set_error(who + ": work smaller than " + sizing[level]); return -(at + 2); }
    if (!out_host) return -(at + 3);
    if (level >= NN_GRAD && !grad_host) return -(at + 4);
    if (level == NN_FISHER && !fisher_host) return -(at + 5);
    if (!info_host) return -(at + 4 + level);
    HIPCHK(hipSetDevice(h->device));
    rc = nn_run_conditionals(h, level, kernel_id, x, n, x, n, d, thetas_host, ntheta, B, idx, ld, m, r, v, v, mu, var, l.cond, score, fisher_rows);
    if (rc) return rc;
    const int P = (int)nn_packed(ntheta);
    rc = nn_sum_columns(h->stream, NnLikTerms{r, mu, var}, n, 2, B, l.part, l.out); if (rc) return rc;
    if (level >= NN_GRAD) { rc = nn_sum_columns(h->stream, NnColumns{score}, n, ntheta, B, l.gpart, l.grad); if (rc) return rc; }
    if (level == NN_FISHER) { rc = nn_sum_columns(h->stream, NnColumns{fisher_rows}, n, P, B, l.fpart, l.fis); if (rc) return rc; }
    long long info = 0;
    std::vector<double> packed(level == NN_FISHER ? (size_t)B * P : 0);
    HIPCHK(hipMemcpyAsync(&info, l.cond.info, sizeof(info), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(out_host, l.out, (size_t)B * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (level >= NN_GRAD) HIPCHK(hipMemcpyAsync(grad_host, l.grad, (size_t)B * ntheta * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (level == NN_FISHER) HIPCHK(hipMemcpyAsync(packed.data(), l.fis, packed.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *info_host = info;
    // the packed lower triangles into full symmetric matrices
    for (int b = 0; level == NN_FISHER && b < B; ++b)
        for (int hh = 0; hh < ntheta; ++hh)
            for (int kk = 0; kk <= hh; ++kk) {
                const double f = packed[(size_t)b * P + (size_t)hh * (hh + 1) / 2 + kk];
                fisher_host[((size_t)b * ntheta + hh) * ntheta + kk] = f;
                fisher_host[((size_t)b * ntheta + kk) * ntheta + hh] = f;
            }
    return 0;
}

}  // namespace

extern "C" {

int64_t fvgp_hip_nn_workspace_bytes(int what, int64_t nq, int B) {
    if (what < FVGP_NN_SEARCH || what > FVGP_NN_LOGLIK || nq < 1 || B < 1) return -1;
    return what == FVGP_NN_CONDITIONALS ? carve_bytes(nn_cond_layout, B) : what == FVGP_NN_LOGLIK ? carve_bytes(nn_layout, NN_VALUE, nq, B, 0) : 0;
}

int64_t fvgp_hip_nn_grad_workspace_bytes(int64_t n, int B, int ntheta) {
    if (n < 1 || B < 1 || ntheta < 1) return -1;
    return carve_bytes(nn_layout, NN_GRAD, n, B, ntheta);
}

int64_t fvgp_hip_nn_fisher_workspace_bytes(int64_t n, int B, int ntheta) {
    if (n < 1 || B < 1 || ntheta < 1) return -1;
    return carve_bytes(nn_layout, NN_FISHER, n, B, ntheta);
}

int fvgp_hip_nn_conditionals(fvgp_handle *h, int kernel_id, const double *xq, int64_t nq, const double *xr, int64_t nr, int d,
                             const double *thetas_host, int ntheta, int B, const int *idx, int64_t ld, int m,
                             const double *r, const double *v, const double *s_or_null, double *mu, double *var,
                             double *work, int64_t work_bytes, int64_t *info_host) {
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!xq) return -3;
    if (nq < 1 || (nq + NN_WAVES - 1) / NN_WAVES > 0x7fffffffLL) return -4;
    if (!xr) return -5;
    if (nr < 1 || nr > 0x7fffffffLL) return -6;
    int rc = check_kernel_args(kernel_id, d, thetas_host, ntheta, 7, 8, 9); if (rc) return rc;
    if (B < 1 || B > 65535) { fvgp_set_error("nn_conditionals: 1 .. 65535 hyperparameter vectors per call"); return -10; }
    if (!idx) return -11;
    if (m < 1 || m > FVGP_NN_MAX_NEIGHBORS) { fvgp_set_error("nn_conditionals: 1 .. FVGP_NN_MAX_NEIGHBORS neighbours"); return -13; }
    if (ld < m) return -12;
    if (!r) return -14;
    if (!v) return -15;
    if (!mu) return -17;
    if (!var) return -18;
    if (!work || ((uintptr_t)work & 7)) return -19;
    Carve c(work); const NnCondWs l = nn_cond_layout(c, B);
    if (work_bytes < c.bytes()) {
        fvgp_set_error("nn_conditionals: work smaller than fvgp_hip_nn_workspace_bytes(FVGP_NN_CONDITIONALS, nq, B)"); return -20;
    }
    if (!info_host) return -21;
    HIPCHK(hipSetDevice(h->device));
    rc = nn_run_conditionals(h, NN_VALUE, kernel_id, xq, nq, xr, nr, d, thetas_host, ntheta, B, idx, ld, m, r, v, s_or_null, mu, var, l, nullptr, nullptr);
    if (rc) return rc;
    long long info = 0;
    HIPCHK(hipMemcpyAsync(&info, l.info, sizeof(info), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *info_host = info;
    return 0;
}

int64_t fvgp_hip_nn_factor_workspace_bytes(int64_t n) {
    if (n < 1) return -1;
    return carve_bytes(nn_factor_layout, n);
}

int fvgp_hip_nn_factor(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta_host, int ntheta,
                       const int *idx, int64_t ld, int m, const double *v, double *coef, int64_t ldc, double *dinv,
                       double *work, int64_t work_bytes, int64_t *info_host) {
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!x) return -3;
    if (n < 1 || n > 0x7fffffffLL) return -4;
    int rc = check_kernel_args(kernel_id, d, theta_host, ntheta, 5, 6, 7); if (rc) return rc;
    if (!idx) return -8;
    if (m < 1 || m > FVGP_NN_MAX_NEIGHBORS) { fvgp_set_error("nn_factor: 1 .. FVGP_NN_MAX_NEIGHBORS neighbours"); return -10; }
    if (ld < m) return -9;
    if (!v) return -11;
    if (!coef) return -12;
    if (ldc < m) return -13;
    if (!dinv) return -14;
    if (!work || ((uintptr_t)work & 7)) return -15;
    Carve c(work); const NnFactorWs l = nn_factor_layout(c, n);
    if (work_bytes < c.bytes()) { fvgp_set_error("nn_factor: work smaller than fvgp_hip_nn_factor_workspace_bytes(n)"); return -16; }
    if (!info_host) return -17;
    HIPCHK(hipSetDevice(h->device));
    rc = nn_run_conditionals(h, NN_FACTOR, kernel_id, x, n, x, n, d, theta_host, ntheta, 1, idx, ld, m, nullptr, v, v, nullptr, l.dvar, l.cond,
                             nullptr, nullptr, coef, ldc, dinv);
    if (rc) return rc;
    long long info = 0;
    HIPCHK(hipMemcpyAsync(&info, l.cond.info, sizeof(info), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *info_host = info;
    return 0;
}

int fvgp_hip_nn_loglik(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *thetas_host, int ntheta, int B,
                       const int *idx, int64_t ld, int m, const double *r, const double *v, double *mu, double *var,
                       double *work, int64_t work_bytes, double *out_host, int64_t *info_host) {
    return nn_loglik(NN_VALUE, "nn_loglik", h, kernel_id, x, n, d, thetas_host, ntheta, B, idx, ld, m, r, v, mu, var, nullptr, nullptr, work,
                     work_bytes, out_host, nullptr, nullptr, info_host);
}

int fvgp_hip_nn_loglik_grad(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *thetas_host, int ntheta, int B,
                            const int *idx, int64_t ld, int m, const double *r, const double *v, double *mu, double *var, double *score,
                            double *work, int64_t work_bytes, double *out_host, double *grad_host, int64_t *info_host) {
    return nn_loglik(NN_GRAD, "nn_loglik_grad", h, kernel_id, x, n, d, thetas_host, ntheta, B, idx, ld, m, r, v, mu, var, score, nullptr, work,
                     work_bytes, out_host, grad_host, nullptr, info_host);
}

int fvgp_hip_nn_loglik_fisher(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *thetas_host, int ntheta, int B,
                              const int *idx, int64_t ld, int m, const double *r, const double *v, double *mu, double *var, double *score,
                              double *fisher_rows, double *work, int64_t work_bytes, double *out_host, double *grad_host,
                              double *fisher_host, int64_t *info_host) {
    return nn_loglik(NN_FISHER, "nn_loglik_fisher", h, kernel_id, x, n, d, thetas_host, ntheta, B, idx, ld, m, r, v, mu, var, score, fisher_rows,
                     work, work_bytes, out_host, grad_host, fisher_host, info_host);
}

}  // extern "C"
