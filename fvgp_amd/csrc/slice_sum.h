// Sums over the data rows with LANES ALONG POINTS (posterior_grad.hip, select.hip, matrix_free.hip): the rows are cut into slices of SLICE_ROWS, one
// workgroup of four waves per (64 points, slice).  The slice's x rows and one vector entry per row are staged in LDS once (every lane
// reads the same row: broadcast reads), each wave takes SLICE_WAVE_ROWS of them, and the sums of waves 1 .. 3 are parked in LDS for
// wave 0 to add in wave order.  The split is a function of n alone: a point's sums have the same bits whatever else rides in the launch.
#pragma once
#include "common.h"

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

// slice_stage with S entries per row (matrix_free.hip): sb[r][S] <- B[row0 + r][c0 .. c0 + sc) (0 past n and from column sc on)
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

// where wave w (1 .. 3) parks its nacc sums for this lane: sum s at [s * 64]
__device__ __forceinline__ double *slice_parked(double *sm, int nacc, int w, int lane) { return sm + (w - 1) * nacc * 64 + lane; }

}  // namespace
