// The greedy pivot core of fvgp_hip_select_batch (select.hip) and fvgp_hip_pchol (matrix_free.hip): q steps of a pivoted Cholesky over P
// candidates without the P x P matrix.  With d the candidates' remaining variances and j the pick of step t,
//     c_i = (r_i - sum_{s<t} G[s,i] G[s,j]) / sqrt(p_t),     G[t,i] = c_i,     d_i <- max(d_i - c_i^2, 0),     p_t = d_j (+ the noise of j)
// where r_i = k(x_i, x_j), less the caller's slice partials when CROSS.  Three kernels, all in stream order:
//     pivot_init_kernel        before step 0: d (given, or sigma^2 everywhere) clipped at 0, the first 64-candidate partials, the state reset
//     pivot_pick_kernel        one workgroup: the partials {score, index} (argmax.h, ties to the lowest index) -> j_t, p_t, x_j into the
//                              slot; or `done` once the best d_j <= tol max_i d_i(initial) / nothing is left
//     pivot_downdate_kernel    one thread per candidate: r_i, c_i, G, d and the partial of its 64 candidates for the next pick
// What the two callers do differently is a few nullable pointers of PivotArgs and CROSS.  Each unit that includes this header compiles
// the kernels for itself: the library holds pivot_init_kernel and pivot_pick_kernel twice, and a profile shows either under one name.
#pragma once
#include "radial.h"
#include "argmax.h"

namespace {

constexpr int PIVOT_PART = 64;               // candidates per argmax partial (one wave)

// the run's small state: p_t, max_i d_i(initial), j_t and `done` (0, or 1 + the step that found the run exhausted) as 64-bit words
struct PivotState { double p, dmax; long long j, done; };

struct PivotArgs {
    const double *x, *xc, *noise;            // data (n, d), candidates (P, d), noise (P) or nullptr
    double *var;                             // (P) the variances d
    double *G; long ldg_in;                  // (q, P) the factor the downdate reads back
    double *Gout; long ldg;                  // a second copy of every row or nullptr
    const double *w;                         // (np) KV^-1 k(X, x_slot)                                 (the cross pass only)
    double *slot;                            // (FVGP_MAX_DIM)
    double *part;                            // (slices, pcap)                                          (the cross pass only)
    double *best;                            // (nparts, 2): score, index (as a double: P < 2^53)
    double *dmaxp;                           // (nparts) max d of the first pass; nullptr: d starts as sigma^2 everywhere
    PivotState *st;
    unsigned char *taken;                    // (P) 1 once the candidate has been picked
    long long *idx; double *pickv;           // (q) the picks (-1 from the exhausted step on) and their d_j or nullptr (written only)
    long n, P, pcap, c0, cn;                 // the launch covers candidates [c0, c0 + cn)
    int d, q, t, crit, repeats;
    double sig, tol;
    double il[FVGP_MAX_DIM];
};

// what candidate i offers the next pick: d, or d / s; nothing if it is taken (and repeats are off) or its score is no number
__device__ __forceinline__ Best candidate(const PivotArgs &a, long i, double dv, bool taken) {
    Best b;
    b.score = a.crit == 0 ? dv : dv / a.noise[i];
    b.idx = (taken && !a.repeats) || !(b.score >= 0.0) ? -1 : i;
    return b;
}

__global__ __launch_bounds__(256) void pivot_init_kernel(PivotArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (i == 0) {
        a.st->done = 0; a.st->j = -1; a.st->p = 1.0; a.st->dmax = a.sig;      // (with partial maxima, step 0 replaces dmax)
        for (int k = 0; k < FVGP_MAX_DIM; ++k) a.slot[k] = k < a.d ? a.xc[k] : 0.0;
    }
    Best b{0.0, -1};
    double dm = 0.0;
    if (i < a.P) {
        double v = a.dmaxp ? a.var[i] : a.sig;
        if (v < 0.0) v = 0.0;
        a.var[i] = v;
        a.taken[i] = 0;
        b = candidate(a, i, v, false);
        dm = v;
    }
    b = wave_best(b);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(dm, off, 64); if (o > dm) dm = o; }
    if (lane == 0 && i < a.P) {
        double *o = a.best + 2 * (i / PIVOT_PART);
        o[0] = b.score; o[1] = (double)b.idx;
        if (a.dmaxp) a.dmaxp[i / PIVOT_PART] = dm;
    }
}

// step t: the partials -> j_t (one workgroup)
__global__ __launch_bounds__(256) void pivot_pick_kernel(PivotArgs a) {
    __shared__ double ss[256], sd[256];
    __shared__ long si[256];
    const int tid = threadIdx.x;
    if (a.st->done) return;                                   // (uniform: written by an earlier launch)
    const long nparts = (a.P + PIVOT_PART - 1) / PIVOT_PART;
    const bool measure = a.t == 0 && a.dmaxp;
    Best b{0.0, -1};
    double dm = 0.0;
    for (long k = tid; k < nparts; k += 256) {
        const Best o{a.best[2 * k], (long)a.best[2 * k + 1]};
        if (better(o, b)) b = o;
        if (measure) { const double v = a.dmaxp[k]; if (v > dm) dm = v; }
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
    if (measure) a.st->dmax = sd[0];
    const long j = si[0];
    const double dj = j >= 0 ? a.var[j] : 0.0;
    if (j < 0 || dj <= a.tol * a.st->dmax) {                  // exhausted: this slot and every later one
        a.st->done = a.t + 1;
        for (int s = a.t; s < a.q; ++s) { a.idx[s] = -1; if (a.pickv) a.pickv[s] = 0.0; }
        return;
    }
    a.idx[a.t] = j; if (a.pickv) a.pickv[a.t] = dj;
    a.taken[j] = 1;
    a.st->j = j; a.st->p = dj + (a.noise ? a.noise[j] : 0.0);
    for (int k = 0; k < a.d; ++k) a.slot[k] = a.xc[j * a.d + k];
}

// CROSS: r_i = k(x_i, x_j) less the `slices` partials of sum_n k(x_i, X_n) w_n, added in ascending order.  A template parameter, not
// slices == 0: without the subtraction k - acc contracts into radial's last multiply, and a zero subtracted at run time would round
// in between
template <int KIND, bool CROSS>
__global__ __launch_bounds__(256) void pivot_downdate_kernel(PivotArgs a, long slices) {
    if (a.st->done) return;
    const long loc = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long i = a.c0 + loc;
    const long j = a.st->j;
    Best b{0.0, -1};
    if (loc < a.cn) {
        double sum = 0.0;
        if (CROSS)
            for (long s = 0; s < slices; ++s) sum += a.part[s * a.pcap + loc];
        double r2 = 0.0;
        for (int k = 0; k < a.d; ++k) { const double e = (a.xc[i * a.d + k] - a.slot[k]) * a.il[k]; r2 = fma(e, e, r2); }
        const double r = CROSS ? radial<KIND>(r2, a.sig) - sum : radial<KIND>(r2, a.sig);
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
        double *o = a.best + 2 * (i / PIVOT_PART);
        o[0] = b.score; o[1] = (double)b.idx;
    }
}

// the workspace every run needs, each piece a multiple of 16 bytes; `words` per partial: 3 with the maxima, which then lie behind the
// (score, index) pairs inside `best` as dmaxp.  The pointers go into the run's arguments
inline void pivot_layout(Carve &c, int64_t P, int words, PivotArgs &a) {
    const int64_t parts = (P + PIVOT_PART - 1) / PIVOT_PART;
    a.slot = c.take<double>(FVGP_MAX_DIM);
    a.st = c.take<PivotState>(1);
    a.best = c.take<double>(words * parts);
    a.dmaxp = words > 2 ? c.view<double>(a.best, 2 * parts) : nullptr;
    a.taken = c.take<unsigned char>(P);
}

}  // namespace
