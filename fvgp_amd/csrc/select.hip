// Greedy batch selection of measurement points (fvgp_hip_select_batch): the pivoted Cholesky of the posterior covariance of
// P candidates, q steps, without the P x P matrix.  With d the candidates' conditional latent variances, s their noise variances and
// j the candidate picked at step t (largest d_i, or largest d_i / s_i; ties to the lowest index),
//     r_i = k(x_i, x_j) - sum_n k(x_i, X_n) w_n,      w = KV^-1 k(X, x_j)                 (column j of the posterior covariance)
//     c_i = (r_i - sum_{s<t} G[s,i] G[s,j]) / sqrt(d_j + s_j),     G[t,i] = c_i,     d_i <- max(d_i - c_i^2, 0).
// Per step, all in stream order on the handle's stream, no host round trip:
//     select_pick_kernel      one workgroup: the 64-candidate partials {score, index} -> j_t, d_j, p_t = d_j + s_j, x_j into a slot;
//                             or `done` once the best d_j <= tol max_i d_i(initial) / nothing is left
//     launch_kmat, potrs_vec  k(X, x_slot) into a padded n-vector and the one-right-hand-side solve in place (the existing assembly and
//                             sweeps, unchanged: they do not read `done` and after exhaustion solve for the last slot once more)
//     select_cross_kernel     the slice partials of sum_n k(x_i, X_n) w_n, lanes along candidates (slice_sum.h)
//     select_downdate_kernel  one thread per candidate: slices added in ascending order, the direct term, c_i, G, d, the next partials
// the last two once per block of at most `select_block` candidates.  The row split is a function of n alone and every sum has a fixed
// order: r_i, and with it row t of G at candidate i, has the same bits whatever P is, whichever candidates share the call and wherever
// the blocks are cut.  Cross pass per entry: one exp (plus the rsq of the Matern kinds), d subtractions, d + 1 fused multiply-adds.
#include "radial.h"
#include "kernel_family.h"
#include "slice_sum.h"
#include "argmax.h"
#include <math.h>

namespace {

constexpr int SEL_PART = 64;                 // candidates per argmax partial (one wave)
constexpr int64_t SEL_BLOCK_MAX = 65536;     // largest (and default) `select_block`

// the call's small state: [0] p_t = d_j + s_j, [1] max_i d_i(initial); then j_t and `done` as 64-bit words
struct SelState { double p, dmax; long long j, done; };

struct SelArgs {
    const double *x, *xc, *noise;            // data (n, d), candidates (P, d), noise (P) or nullptr
    double *var;                             // (P) the conditional variances d
    double *G; long ldg_in;                  // (q, P) in the workspace
    double *Gout; long ldg;                  // the caller's copy or nullptr
    const double *w;                         // (np) KV^-1 k(X, x_slot)
    double *slot;                            // (FVGP_MAX_DIM)
    double *part;                            // (slices, pcap)
    double *best;                            // (nparts, 3): score, index (as a double: P < 2^53), max d (first pass only)
    SelState *st;
    unsigned char *taken;                    // (P) 1 once the candidate has been picked
    long long *idx; double *pickv;           // (q) the caller's outputs (written only)
    long n, P, pcap, c0, cn;                 // the launch covers candidates [c0, c0 + cn)
    int d, q, t, crit, repeats;
    double sig, tol;
    double il[FVGP_MAX_DIM];
};

// what candidate i offers the next pick: d, or d / s; nothing if it is taken (and repeats are off) or its score is no number
__device__ __forceinline__ Best candidate(const SelArgs &a, long i, double dv, bool taken) {
    Best b;
    b.score = a.crit == 0 ? dv : dv / a.noise[i];
    b.idx = (taken && !a.repeats) || !(b.score >= 0.0) ? -1 : i;
    return b;
}

// before step 0: variances below 0 taken as 0, the first partials, the largest initial variance; the state reset
__global__ __launch_bounds__(256) void select_init_kernel(SelArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (i == 0) {
        a.st->done = 0; a.st->j = -1; a.st->p = 1.0; a.st->dmax = 0.0;
        for (int k = 0; k < FVGP_MAX_DIM; ++k) a.slot[k] = k < a.d ? a.xc[k] : 0.0;
    }
    Best b{0.0, -1};
    double dm = 0.0;
    if (i < a.P) {
        double v = a.var[i];
        if (v < 0.0) { v = 0.0; a.var[i] = v; }
        a.taken[i] = 0;
        b = candidate(a, i, v, false);
        dm = v;
    }
    b = wave_best(b);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(dm, off, 64); if (o > dm) dm = o; }
    if (lane == 0 && i < a.P) {
        double *o = a.best + 3 * (i / SEL_PART);
        o[0] = b.score; o[1] = (double)b.idx; o[2] = dm;
    }
}

// step t: the partials -> j_t (one workgroup)
__global__ __launch_bounds__(256) void select_pick_kernel(SelArgs a) {
    __shared__ double ss[256], sd[256];
    __shared__ long si[256];
    const int tid = threadIdx.x;
    if (a.st->done) return;                                   // (uniform: written by an earlier launch)
    const long nparts = (a.P + SEL_PART - 1) / SEL_PART;
    Best b{0.0, -1};
    double dm = 0.0;
    for (long k = tid; k < nparts; k += 256) {
        const Best o{a.best[3 * k], (long)a.best[3 * k + 1]};
        if (better(o, b)) b = o;
        if (a.t == 0) { const double v = a.best[3 * k + 2]; if (v > dm) dm = v; }
    }
    ss[tid] = b.score; si[tid] = b.idx; sd[tid] = dm;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            const Best m{ss[tid], si[tid]}, o{ss[tid + off], si[tid + off]};
            if (better(o, m)) { ss[tid] = o.score; si[tid] = o.idx; }
            if (sd[tid + off] > sd[tid]) sd[tid] = sd[tid + off];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    if (a.t == 0) a.st->dmax = sd[0];
    const long j = si[0];
    const double dj = j >= 0 ? a.var[j] : 0.0;
    if (j < 0 || dj <= a.tol * a.st->dmax) {                  // exhausted: this slot and every later one
        a.st->done = 1;
        for (int s = a.t; s < a.q; ++s) { a.idx[s] = -1; a.pickv[s] = 0.0; }
        return;
    }
    a.idx[a.t] = j; a.pickv[a.t] = dj;
    a.taken[j] = 1;
    a.st->j = j; a.st->p = dj + (a.noise ? a.noise[j] : 0.0);
    for (int k = 0; k < a.d; ++k) a.slot[k] = a.xc[j * a.d + k];
}

// the slice partials of sum_n k(x_i, X_n) w_n for the candidates [c0, c0 + cn): grid (ceil(cn / 64), slices)
template <int KIND, int D>   // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(256) void select_cross_kernel(SelArgs a) {
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
    double u[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) u[k] = k < d ? a.xc[i * d + k] : 0.0;
    __syncthreads();

    const int r0 = wave * SLICE_WAVE_ROWS, rows = slice_wave_rows(a.n, row0, wave);
    double s0 = 0.0, s1 = 0.0;                                // even and odd rows: two exp chains in flight, added once at the end
    int r = 0;
    for (; r + 1 < rows; r += 2) {
        const double *xa = sx + (r0 + r) * DD, *xb = xa + DD;
        double ra = 0.0, rb = 0.0;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < d) {
                const double ea = (u[k] - xa[k]) * a.il[k], eb = (u[k] - xb[k]) * a.il[k];
                ra = fma(ea, ea, ra); rb = fma(eb, eb, rb);
            }
        s0 = fma(radial<KIND>(ra, a.sig), sw[r0 + r], s0);
        s1 = fma(radial<KIND>(rb, a.sig), sw[r0 + r + 1], s1);
    }
    if (r < rows) {
        const double *xa = sx + (r0 + r) * DD;
        double ra = 0.0;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < d) { const double ea = (u[k] - xa[k]) * a.il[k]; ra = fma(ea, ea, ra); }
        s0 = fma(radial<KIND>(ra, a.sig), sw[r0 + r], s0);
    }
    double s = s0 + s1;

    __syncthreads();                                          // every wave is done with the staged rows
    if (wave > 0) *slice_parked(sm, 1, wave, lane) = s;
    __syncthreads();
    if (wave != 0 || loc >= a.cn) return;
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) s += *slice_parked(sm, 1, ww, lane);      // ((wave 0 + wave 1) + wave 2) + wave 3
    a.part[(long)blockIdx.y * a.pcap + loc] = s;
}

// one thread per candidate of [c0, c0 + cn): r_i, c_i, G[t, i], d_i and the partial of its 64 candidates for the next pick
template <int KIND>
__global__ __launch_bounds__(256) void select_downdate_kernel(SelArgs a, long slices) {
    if (a.st->done) return;
    const long loc = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long i = a.c0 + loc;
    const long j = a.st->j;
    Best b{0.0, -1};
    if (loc < a.cn) {
        double sum = 0.0;
        for (long s = 0; s < slices; ++s) sum += a.part[s * a.pcap + loc];
        double r2 = 0.0;
        for (int k = 0; k < a.d; ++k) { const double e = (a.xc[i * a.d + k] - a.slot[k]) * a.il[k]; r2 = fma(e, e, r2); }
        const double r = radial<KIND>(r2, a.sig) - sum;
        double acc = 0.0;
        for (int s = 0; s < a.t; ++s) acc = fma(a.G[s * a.ldg_in + i], a.G[s * a.ldg_in + j], acc);
        const double c = (r - acc) / sqrt(a.st->p);
        a.G[(long)a.t * a.ldg_in + i] = c;
        if (a.Gout) a.Gout[(long)a.t * a.ldg + i] = c;
        double dv = fma(-c, c, a.var[i]);
        if (dv < 0.0) dv = 0.0;
        a.var[i] = dv;
        b = candidate(a, i, dv, a.taken[i] != 0);
    }
    b = wave_best(b);
    if (lane == 0 && loc < a.cn) {
        double *o = a.best + 3 * (i / SEL_PART);
        o[0] = b.score; o[1] = (double)b.idx;
    }
}

struct SelLayout { int64_t kvec, slot, state, best, taken, G, part, total; };      // offsets in doubles (each a multiple of 2)
SelLayout sel_layout(int64_t n, int64_t P, int q) {
    SelLayout l;
    const int64_t np = pad128(n), nparts = (P + SEL_PART - 1) / SEL_PART, pcap = P < SEL_BLOCK_MAX ? P : SEL_BLOCK_MAX;
    auto even = [](int64_t v) { return (v + 1) & ~(int64_t)1; };
    int64_t o = 0;
    l.kvec = o; o += np;
    l.slot = o; o += even(FVGP_MAX_DIM);
    l.state = o; o += even((int64_t)(sizeof(SelState) / sizeof(double)));
    l.best = o; o += even(3 * nparts);
    l.taken = o; o += even((P + 7) / 8);
    l.G = o; o += even((int64_t)q * P);
    l.part = o; o += slice_count(n) * pcap;
    l.total = o;
    return l;
}

}  // namespace

extern "C" {

int64_t fvgp_hip_select_workspace_bytes(int64_t n, int64_t P, int q) {
    if (n < 1 || P < 1 || q < 1) return -1;
    return sel_layout(n, P, q).total * (int64_t)sizeof(double);
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
    if (d < 1 || d > FVGP_MAX_DIM) { fvgp_set_error("input dimension out of range"); return -5; }
    if (!theta) return -6;
    if (ntheta < kernel_param_count(kernel_id, d)) { fvgp_set_error("too few hyperparameters for this kernel"); return -7; }
    int rc = check_square(L, n, ldl, 8, 4, 9);
    if (rc) return rc;
    if (!xcand) return -10;
    if (P <= 0) return -11;
    if (criterion == 1 && !noise) { fvgp_set_error("select_batch: criterion 1 needs the candidates' noise variances (all > 0)"); return -12; }
    if (!var) return -13;
    if (q < 1) return -14;
    if (criterion != 0 && criterion != 1) return -15;
    if (!(tol >= 0.0)) return -17;
    if (!work || ((uintptr_t)work & 15)) { fvgp_set_error("select_batch: work must be 16-byte aligned"); return -18; }
    if (work_bytes < fvgp_hip_select_workspace_bytes(n, P, q)) {
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
    const SelLayout lay = sel_layout(n, P, q);
    const int64_t block = h->select_block < SEL_BLOCK_MAX ? h->select_block : SEL_BLOCK_MAX;
    // the handle's own buffers (block inverses of the factor, the sweeps' vector): allocated on the first call that needs them
    rc = ensure_linv(h, L, n, ldl); if (rc) return rc;
    rc = ensure_scratch(h, np); if (rc) return rc;

    SelArgs a;
    a.x = x; a.xc = xcand; a.noise = noise; a.var = var;
    a.G = work + lay.G; a.ldg_in = P; a.Gout = G_out; a.ldg = ldg;
    a.w = work + lay.kvec; a.slot = work + lay.slot; a.part = work + lay.part; a.best = work + lay.best;
    a.st = reinterpret_cast<SelState *>(work + lay.state);
    a.taken = reinterpret_cast<unsigned char *>(work + lay.taken);
    a.idx = reinterpret_cast<long long *>(idx_out); a.pickv = pick_var_out;
    a.n = n; a.P = P; a.pcap = P < SEL_BLOCK_MAX ? P : SEL_BLOCK_MAX; a.c0 = 0; a.cn = 0;
    a.d = d; a.q = q; a.t = 0; a.crit = criterion; a.repeats = allow_repeats ? 1 : 0;
    a.sig = k.sig; a.tol = tol;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.il[i] = k.invl[i];

    double *kvec = work + lay.kvec;
    HIPCHK(hipMemsetAsync(kvec, 0, (size_t)np * sizeof(double), h->stream));          // the padding rows stay 0 through every step
    hipLaunchKernelGGL(select_init_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    for (int t = 0; t < q; ++t) {
        a.t = t;
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(256), 0, h->stream, a);
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
                hipLaunchKernelGGL((select_downdate_kernel<decltype(KIND)::value>), dim3((unsigned)((a.cn + 255) / 256)), dim3(256), 0,
                                   h->stream, a, (long)S);
            });
            HIPCHK(hipGetLastError());
        }
    }
    return 0;
}

}  // extern "C"
