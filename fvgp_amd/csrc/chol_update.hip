// Rank-k update of a resident Cholesky factor and removal of data points.
//
//   fvgp_hip_chol_update : L <- chol(L L^T + W W^T) in place, by Givens rotations of the columns of [L | W]
//   fvgp_hip_chol_delete : the factor of K+V without the rows / columns R, from the factor L of all of it:
//                          KV[S,S] = L[S,S] L[S,S]^T + L[S,R] L[S,R]^T  (S the kept indices), so the new factor is the
//                          positive rank-|R| update of the compacted triangle L[S,S] by W = L[S,R]
//
// One pass takes up to 16 columns of W.  Column j of L is rotated against column p of W, p = 0 .. kp-1 in turn:
//     q_p = L_jj^2 + sum_{u <= p} W_ju^2,  r_p = sqrt(q_p),  c_p = r_{p-1} / r_p,  s_p = W_jp / r_p   (r_{-1} = L_jj)
//     every row i >= j:  (L_ij, W_ip) <- (c_p L_ij + s_p W_ip,  c_p W_ip - s_p L_ij)
// The coefficients of column j are a function of row j alone (as the columns before j left it), and given the coefficients of a
// 128-column block every row below it is independent of every other row.  So per block column J there are two plain launches in
// stream order: ONE workgroup rotates the 128 x 128 diagonal block (in LDS, a thread per row, W's rows in registers) and leaves the
// 128 x kp coefficient pairs in a table; then a workgroup per 64 rows (a lane of its first wave per row) applies the table to
// (L_IJ, W_I) for every row below, the tile
// staged through LDS so that global memory is read and written in whole rows of the tile.  No workgroup waits for another through
// memory, nothing is accumulated atomically, every sum has a fixed order: the same call gives the same bits, and row i of the result
// depends on rows <= i of L and W only (the leading m rows of an update of n rows ARE the update of the leading m x m problem).
#include "common.h"
#include <type_traits>

namespace {

constexpr int CU_RANK = FVGP_CHOL_UPDATE_MAX_RANK;      // columns of W per pass
constexpr int CU_TAB_DOUBLES = TILE * CU_RANK * 2;      // (c, s) per column of the block and column of W
constexpr int DLD = TILE + 1;                           // LDS row stride of the staged tiles: a thread per row reads without conflicts
constexpr int PANEL_ROWS = 64;                          // rows per workgroup of the panel step: a lane of its first wave each
constexpr int PANEL_THREADS = 256, DIAG_THREADS = 256;  // (the other waves only move the tiles between memory and LDS)
constexpr int64_t STRIP_ROWS = 1024;                    // most rows of the compaction's strip scratch
constexpr int64_t STRIP_DOUBLES = (int64_t)1 << 25;     // ... and most doubles of it (256 MiB): fewer rows per strip past n = 32768

struct CuArgs {
    double *L; long ldl;
    double *W; long ldw;       // W already offset to the pass's first column
    long n, j0;                // rows of the problem, first column of the block column
    int kp, jfirst;            // columns of W in this pass; first column of the block with a non-zero row of W
    double *tab;
};

// ---- the diagonal step: one workgroup, thread t owns row j0 + t ---------------------------------------------------
template <int KP>
__global__ __launch_bounds__(DIAG_THREADS) void chol_update_diag_kernel(CuArgs a) {
    __shared__ double sD[TILE * DLD];
    __shared__ double srow[KP + 2];
    __shared__ double2_t scs[KP];
    const int t = threadIdx.x;
    const long left = a.n - a.j0;
    const int nv = left < TILE ? (int)left : TILE;
    double *Lb = a.L + a.j0 * a.ldl + a.j0;
    // the block through LDS, two rows per instruction and 16 loads in flight per thread (a load per row and iteration would serialise
    // 128 round trips to memory); the lower triangle only: the strict upper is never read
    const int c = t & (TILE - 1), rh = t >> 7;
    for (int base = 0; base < TILE; base += 32) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = base + 2 * u + rh;
            v[u] = (r < nv && c <= r) ? Lb[(long)r * a.ldl + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = base + 2 * u + rh;
            if (r < nv && c <= r) sD[r * DLD + c] = v[u];
        }
    }
    // KP >= kp is a compile-time count (no branch between two rotations, their LDS reads issued together); the columns kp .. KP - 1
    // are zero, their rotations c = x / x = 1, s = 0: every value keeps its bits
    double w[KP];
#pragma unroll
    for (int p = 0; p < KP; ++p) w[p] = (t < nv && p < a.kp) ? a.W[(a.j0 + t) * a.ldw + p] : 0.0;
    __syncthreads();
    for (int j = a.jfirst; j < nv; ++j) {
        if (t == j) {
            srow[0] = sD[j * DLD + j];
#pragma unroll
            for (int p = 0; p < KP; ++p) srow[1 + p] = w[p];
        }
        __syncthreads();
        if (t < KP) {
            const double l = srow[0];
            double q = l * l, qp = q;
#pragma unroll
            for (int u = 0; u < KP; ++u)
                if (u <= t) { qp = q; q = fma(srow[1 + u], srow[1 + u], q); }
            const double r = sqrt(q), rp = t == 0 ? l : sqrt(qp);
            double2_t cs;
            cs.x = rp / r; cs.y = srow[1 + t] / r;
            scs[t] = cs;
            a.tab[(j * KP + t) * 2] = cs.x;
            a.tab[(j * KP + t) * 2 + 1] = cs.y;
            if (t == KP - 1) sD[j * DLD + j] = r;
        }
        __syncthreads();
        if (t > j && t < nv) {
            double l = sD[t * DLD + j];
#pragma unroll
            for (int p = 0; p < KP; ++p) {
                const double2_t cs = scs[p];
                const double sw = cs.y * w[p];
                w[p] = fma(cs.x, w[p], -(cs.y * l));
                l = fma(cs.x, l, sw);
            }
            sD[t * DLD + j] = l;
        }
    }
    __syncthreads();
    for (int base = 0; base < TILE; base += 32) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = base + 2 * u + rh;
            if (r < nv && c <= r) Lb[(long)r * a.ldl + c] = sD[r * DLD + c];
        }
    }
}

// ---- the panel step: a workgroup per 64 rows below the block, lane t of its first wave owns row r0 + t ----------------------------------------
template <int KP>
__global__ __launch_bounds__(PANEL_THREADS) void chol_update_panel_kernel(CuArgs a) {
    __shared__ double sT[PANEL_ROWS * DLD];
    __shared__ double2_t scs[TILE * KP];
    const int t = threadIdx.x;
    const long r0 = a.j0 + TILE + (long)blockIdx.x * PANEL_ROWS;
    const long left = a.n - r0;
    const int nr = left < PANEL_ROWS ? (int)left : PANEL_ROWS;
    const double2_t *tab2 = reinterpret_cast<const double2_t *>(a.tab);
    for (int e = t; e < TILE * KP; e += PANEL_THREADS) scs[e] = tab2[e];
    double *Lb = a.L + r0 * a.ldl + a.j0;
    // four waves move the tile, a row of it (1 KiB contiguous) per wave instruction and 16 of them in flight per wave; wave 0 rotates
    const int lane = t & 63, rq = t >> 6;
    {
        double2_t v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = 4 * u + rq;
            if (r < nr) v[u] = *reinterpret_cast<const double2_t *>(Lb + (long)r * a.ldl + 2 * lane);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = 4 * u + rq;
            if (r < nr) { sT[r * DLD + 2 * lane] = v[u].x; sT[r * DLD + 2 * lane + 1] = v[u].y; }
        }
    }
    double w[KP];
#pragma unroll
    for (int p = 0; p < KP; ++p) w[p] = (t < nr && p < a.kp) ? a.W[(r0 + t) * a.ldw + p] : 0.0;
    __syncthreads();
    if (t < nr) {                                                          // (nr <= 64: wave 0, lane t owns row r0 + t)
        for (int j = a.jfirst; j < TILE; ++j) {
            double l = sT[t * DLD + j];
#pragma unroll
            for (int p = 0; p < KP; ++p) {
                const double2_t cs = scs[j * KP + p];
                const double sw = cs.y * w[p];
                w[p] = fma(cs.x, w[p], -(cs.y * l));
                l = fma(cs.x, l, sw);
            }
            sT[t * DLD + j] = l;
        }
#pragma unroll
        for (int p = 0; p < KP; ++p)
            if (p < a.kp) a.W[(r0 + t) * a.ldw + p] = w[p];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int r = 4 * u + rq;
        if (r < nr) {
            double2_t v;
            v.x = sT[r * DLD + 2 * lane]; v.y = sT[r * DLD + 2 * lane + 1];
            *reinterpret_cast<double2_t *>(Lb + (long)r * a.ldl + 2 * lane) = v;
        }
    }
}

// ---- removal: the kept indices, W = L[S,R], and L[S,S] moved up-left through a strip --------------------------------------
// S[i - #(R < i)] = i for every i not in R (R strictly increasing)
__global__ void kept_index_kernel(const long *R, int k, long n, long *S) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = k;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (R[mid] < i) lo = mid + 1; else hi = mid; }
    if (lo < k && R[lo] == i) return;
    S[i - lo] = i;
}

// W[i][p] = L[S[i]][R[p]] where that lies below the diagonal, else 0
__global__ void gather_w_kernel(const double *L, long ldl, const long *S, const long *R, long m, int k, double *W, long ldw) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * k) return;
    const long i = e / k; const int p = (int)(e % k);
    const long s = S[i], r = R[p];
    W[i * ldw + p] = r < s ? L[s * ldl + r] : 0.0;
}

// strip[i - a][j] = L[S[i]][S[j]], j <= i, for the rows i = a + blockIdx.x: reads rows >= a of L only
__global__ __launch_bounds__(256) void strip_gather_kernel(const double *L, long ldl, const long *S, long a, double *strip, long lds) {
    const long i = a + blockIdx.x;
    const double *src = L + S[i] * ldl;
    double *dst = strip + (long)blockIdx.x * lds;
    for (long j = threadIdx.x; j <= i; j += 256) dst[j] = src[S[j]];
}

// L[i][j] = strip[i - a][j], j <= i: writes rows a .. a + gridDim.x - 1 of L, which no later strip reads
__global__ __launch_bounds__(256) void strip_scatter_kernel(double *L, long ldl, long a, const double *strip, long lds) {
    const long i = a + blockIdx.x;
    const double *src = strip + (long)blockIdx.x * lds;
    double *dst = L + i * ldl;
    for (long j = threadIdx.x; j <= i; j += 256) dst[j] = src[j];
}

int64_t strip_rows(int64_t n) {
    int64_t r = STRIP_DOUBLES / even_up(n);
    if (r > STRIP_ROWS) r = STRIP_ROWS;
    if (r > n) r = n;
    return r < 1 ? 1 : r;
}

// the passes of an update whose arguments have been checked; row0[g]: the first row of W with a non-zero in pass g's columns
int update_passes(fvgp_handle *h, double *L, int64_t n, int64_t ldl, double *W, int k, int64_t ldw, const int64_t *row0, int64_t row0_all,
                  double *tab) {
    for (int p0 = 0, g = 0; p0 < k; p0 += CU_RANK, ++g) {
        const int64_t first = row0 ? row0[g] : row0_all;
        if (first >= n) continue;
        CuArgs a;
        a.L = L; a.ldl = (long)ldl; a.W = W + p0; a.ldw = (long)ldw; a.n = (long)n; a.tab = tab;
        a.kp = k - p0 < CU_RANK ? k - p0 : CU_RANK;
        for (int64_t j0 = first / TILE * TILE; j0 < n; j0 += TILE) {
            a.j0 = (long)j0;
            a.jfirst = first > j0 ? (int)(first - j0) : 0;
            const int64_t below = n - j0 - TILE;
            const dim3 grid((unsigned)((below + PANEL_ROWS - 1) / PANEL_ROWS));
            auto go = [&](auto KP) {
                hipLaunchKernelGGL(chol_update_diag_kernel<decltype(KP)::value>, dim3(1), dim3(DIAG_THREADS), 0, h->stream, a);
                if (below > 0) hipLaunchKernelGGL(chol_update_panel_kernel<decltype(KP)::value>, grid, dim3(PANEL_THREADS), 0, h->stream, a);
            };
            if (a.kp == 1) go(std::integral_constant<int, 1>{});
            else if (a.kp == 2) go(std::integral_constant<int, 2>{});
            else if (a.kp <= 4) go(std::integral_constant<int, 4>{});
            else if (a.kp <= 8) go(std::integral_constant<int, 8>{});
            else go(std::integral_constant<int, CU_RANK>{});
            HIPCHK(hipGetLastError());
        }
    }
    return 0;
}

// the coefficient table, all an update uses of its workspace (FVGP_CHOL_UPDATE_TABLE_BYTES) and the first piece of a removal's
static_assert(CU_TAB_DOUBLES * sizeof(double) == FVGP_CHOL_UPDATE_TABLE_BYTES, "the table's size is part of the ABI");
double *cu_table(Carve &c) { return c.take<double>(CU_TAB_DOUBLES); }

// a removal's workspace: the table, the removed and the kept indices, W = L[S, R] (n rows of ldw), the strip (srows rows of lds)
struct DeleteWs { double *tab; long *R, *S; double *W, *strip; int64_t ldw, lds, srows; };
DeleteWs delete_layout(Carve &c, int64_t n, int64_t k) {
    const int64_t ldw = even_up(k), lds = even_up(n), srows = strip_rows(n);
    return {cu_table(c), c.take<long>(k), c.take<long>(n), c.take<double>(n * ldw), c.take<double>(srows * lds), ldw, lds, srows};
}

}  // namespace

extern "C" {

int64_t fvgp_hip_chol_update_workspace_bytes(int64_t n, int64_t k) {
    if (n < 1 || k < 1) return -1;
    return carve_bytes(delete_layout, n, k);
}

int fvgp_hip_chol_update(fvgp_handle *h, double *L, int64_t n, int64_t ldl, double *W, int64_t k, int64_t ldw, int64_t row0,
                         double *ws, int64_t ws_bytes) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    if (!W) return -5;
    if (k < 1 || k > INT32_MAX) return -6;
    if (ldw < k) { fvgp_set_error("chol_update: ldw below k"); return -7; }
    if (row0 < 0 || row0 > n) { fvgp_set_error("chol_update: row0 outside 0 .. n"); return -8; }
    if (!ws || ((uintptr_t)ws & 15)) { fvgp_set_error("chol_update: ws must be 16-byte aligned"); return -9; }
    Carve c(ws); double *tab = cu_table(c);
    if (ws_bytes < c.bytes()) { fvgp_set_error("chol_update: ws smaller than FVGP_CHOL_UPDATE_TABLE_BYTES"); return -10; }
    HIPCHK(hipSetDevice(h->device));
    return update_passes(h, L, n, ldl, W, (int)k, ldw, nullptr, row0, tab);
}

int fvgp_hip_chol_delete(fvgp_handle *h, double *L, int64_t n, int64_t ldl, const int64_t *idx_host, int64_t k, double *ws, int64_t ws_bytes) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    if (!idx_host) return -5;
    if (k < 1 || k >= n || k > INT32_MAX) { fvgp_set_error("chol_delete: k outside 1 .. n - 1"); return -6; }
    for (int64_t p = 0; p < k; ++p)
        if (idx_host[p] < 0 || idx_host[p] >= n || (p && idx_host[p] <= idx_host[p - 1])) {
            fvgp_set_error("chol_delete: indices must be strictly increasing and inside 0 .. n - 1"); return -5;
        }
    if (!ws || ((uintptr_t)ws & 15)) { fvgp_set_error("chol_delete: ws must be 16-byte aligned"); return -7; }
    Carve c(ws); const DeleteWs l = delete_layout(c, n, k);
    if (ws_bytes < c.bytes()) {
        fvgp_set_error("chol_delete: ws smaller than fvgp_hip_chol_update_workspace_bytes(n, k)"); return -8;
    }
    HIPCHK(hipSetDevice(h->device));
    const int64_t m = n - k, ldw = l.ldw, np = pad128(n), first = idx_host[0], lds = l.lds, srows = l.srows;
    double *tab = l.tab, *W = l.W, *strip = l.strip;
    long *R = l.R, *S = l.S;
    static_assert(sizeof(long) == sizeof(int64_t), "index words");
    HIPCHK(hipMemcpyAsync(R, idx_host, (size_t)k * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(kept_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, R, (int)k, (long)n, S);
    HIPCHK(hipGetLastError());
    if (first < m) {        // (else only trailing rows leave: W is zero and the kept triangle stays where it is)
        hipLaunchKernelGGL(gather_w_kernel, dim3((unsigned)((m * k + 255) / 256)), dim3(256), 0, h->stream, L, (long)ldl, S, R, (long)m, (int)k,
                           W, (long)ldw);
        HIPCHK(hipGetLastError());
        for (int64_t a = first; a < m; a += srows) {
            const unsigned rows = (unsigned)(m - a < srows ? m - a : srows);
            hipLaunchKernelGGL(strip_gather_kernel, dim3(rows), dim3(256), 0, h->stream, L, (long)ldl, S, (long)a, strip, (long)lds);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(strip_scatter_kernel, dim3(rows), dim3(256), 0, h->stream, L, (long)ldl, (long)a, strip, (long)lds);
            HIPCHK(hipGetLastError());
        }
    }
    rc = launch_pad_identity(h, L, m, np, ldl);
    if (rc) return rc;
    if (first >= m) return 0;
    // column p of W is zero above the first kept row behind R[p]: row R[p] - p of the compacted order
    std::vector<int64_t> row0;
    for (int64_t p0 = 0; p0 < k; p0 += CU_RANK) row0.push_back(idx_host[p0] - p0);
    return update_passes(h, L, m, ldl, W, (int)k, ldw, row0.data(), 0, tab);
}

}  // extern "C"
