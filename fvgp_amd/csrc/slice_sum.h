// Sums over the data rows with LANES ALONG POINTS (posterior_grad.hip, select.hip, matvec.hip): the rows are cut into slices of SLICE_ROWS, one
// workgroup of four waves per (64 points, slice).  The slice's x rows and one vector entry per row are staged in LDS once (every lane
// reads the same row: broadcast reads), each wave takes SLICE_WAVE_ROWS of them, and the sums of waves 1 .. 3 are parked in LDS for
// wave 0 to add in wave order.  The split is a function of n alone: a point's sums have the same bits whatever else rides in the launch.
// slice_rows is the row loop of the two kernels whose summand is k(u, x_r) times S staged entries (select_cross_kernel, S = 1, and
// kmatvec_kernel); posterior_grad.hip has its own.
#pragma once
#include "common.h"
#include "radial.h"

namespace {

constexpr int SLICE_ROWS = 256;      // data rows per workgroup (slice)
constexpr int SLICE_WAVE_ROWS = 64;  // ... per wave

inline int64_t slice_count(int64_t n) { return (n + SLICE_ROWS - 1) / SLICE_ROWS; }

// sx[r][DD] <- x[row0 + r][d] (rows past n read the last row and are never summed), sa[r] <- v[(row0 + r) * vstride] (0 past n);
// 256 threads, the caller synchronises
template <int DD>
__device__ __forceinline__ void slice_stage(double *sx, double *sa, const double *x, const double *v, long vstride, long n, int d,
                                            long row0, int tid) {
    for (int e = tid; e < SLICE_ROWS * d; e += 256) {
        const int rr = e / d, kk = e - rr * d;
        long gr = row0 + rr; if (gr >= n) gr = n - 1;
        sx[rr * DD + kk] = x[gr * d + kk];
    }
    {
        const long gr = row0 + tid;
        sa[tid] = gr < n ? v[gr * vstride] : 0.0;
    }
}

// slice_stage with S entries per row (matvec.hip): sb[r][S] <- B[row0 + r][c0 .. c0 + sc) (0 past n and from column sc on)
template <int DD, int S>
__device__ __forceinline__ void slice_stage_cols(double *sx, double *sb, const double *x, const double *B, long ldb, int c0, int sc,
                                                 long n, int d, long row0, int tid) {
    for (int e = tid; e < SLICE_ROWS * d; e += 256) {
        const int rr = e / d, kk = e - rr * d;
        long gr = row0 + rr; if (gr >= n) gr = n - 1;
        sx[rr * DD + kk] = x[gr * d + kk];
    }
    for (int e = tid; e < SLICE_ROWS * S; e += 256) {
        const int rr = e / S, cc = e - rr * S;
        const long gr = row0 + rr;
        sb[e] = gr < n && cc < sc ? B[gr * ldb + c0 + cc] : 0.0;
    }
}

// rows of the slice at row0 that wave `wave` sums (0: none exist)
__device__ __forceinline__ int slice_wave_rows(long n, long row0, int wave) {
    const long left = n - row0 - (long)wave * SLICE_WAVE_ROWS;
    return left >= SLICE_WAVE_ROWS ? SLICE_WAVE_ROWS : (left > 0 ? (int)left : 0);
}

// this wave's rows [r0, r0 + rows) of the staged slice against the lane's point u: s0[c] += k(u, x_r) sb[r][c] over the even rows,
// s1[c] over the odd ones (two exp chains in flight; the caller adds the pair once, at the end), then an odd last row into s0
template <int KIND, int DD, int S>
__device__ __forceinline__ void slice_rows(const double *sx, const double *sb, int r0, int rows, int d, const double (&u)[DD],
                                           const double (&il)[DD], double sig, double (&s0)[S], double (&s1)[S]) {
    int r = 0;
    for (; r + 1 < rows; r += 2) {
        const double *xa = sx + (r0 + r) * DD, *xb = xa + DD;
        double ra = 0.0, rb = 0.0;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < d) {
                const double ea = (u[k] - xa[k]) * il[k], eb = (u[k] - xb[k]) * il[k];
                ra = fma(ea, ea, ra); rb = fma(eb, eb, rb);
            }
        const double ka = radial<KIND>(ra, sig), kb = radial<KIND>(rb, sig);
        const double *ba = sb + (r0 + r) * S, *bb = ba + S;
#pragma unroll
        for (int c = 0; c < S; ++c) { s0[c] = fma(ka, ba[c], s0[c]); s1[c] = fma(kb, bb[c], s1[c]); }
    }
    if (r < rows) {
        const double *xa = sx + (r0 + r) * DD;
        double ra = 0.0;
#pragma unroll
        for (int k = 0; k < DD; ++k)
            if (k < d) { const double ea = (u[k] - xa[k]) * il[k]; ra = fma(ea, ea, ra); }
        const double ka = radial<KIND>(ra, sig);
        const double *ba = sb + (r0 + r) * S;
#pragma unroll
        for (int c = 0; c < S; ++c) s0[c] = fma(ka, ba[c], s0[c]);
    }
}

// where wave w (1 .. 3) parks its nacc sums for this lane: sum s at [s * 64]
__device__ __forceinline__ double *slice_parked(double *sm, int nacc, int w, int lane) { return sm + (w - 1) * nacc * 64 + lane; }

}  // namespace
