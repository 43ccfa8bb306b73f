// The exact cell-grid neighbour search of the nearest-neighbour path (include/fvgp_hip_nn.h), d <= 3: the lists of
// fvgp_hip_nn_search, element for element, in near-linear time.
// fvgp_hip_nn_grid_build    a uniform grid of cubic cells over the reference rows in the search's scaled coordinates.  Four steps: the
//     bounding box (per-workgroup minima and maxima, read back and joined on the host: the one synchronisation); the cells per dimension
//     on the host; every row's cell, and its rank inside the cell from an integer atomic on the cell's counter (the counts do not depend
//     on the order, the ranks do: they only decide where inside its cell's bucket a row lands); an exclusive scan of the counts (three
//     launches: blocks of NG_SCAN_BLOCK entries, their sums by one workgroup, the offsets added); the rows' indices and coordinates
//     written to start[cell] + rank.  Linear in nr whatever the fullest cell holds.
// fvgp_hip_nn_grid_search   a lane per query as in nn_search_kernel, its distance and its list (nn_geometry.h: nn_dist2, nn_top_insert),
//     the list ordered by the pair (distance, index) explicitly, since rows no longer arrive in ascending index.  Cells are visited in growing Chebyshev shells around
//     the query's cell; cells that follow each other along the last dimension are one contiguous range of the bucketed rows, so a run of
//     them costs two reads of `start`.  The walk stops when the list is full and its worst distance lies STRICTLY below a lower bound on
//     the computed distance of every row in a cell not visited yet (ng_stop_bound; the margin is derived in DESIGN 28).  Causal calls: the
//     queries with fewer than ng_early(nr) candidates go to the brute entry (fvgp_hip_nn_search), whose cost there is small, while a grid
//     walk would cover most of the grid to find them.  Every loop is bounded by the grid's shape or a cell's occupancy, never by a
//     coordinate.
#include "nn_geometry.h"
#include "../../include/fvgp_hip_nn.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int NG_MAX_DIM = FVGP_NN_GRID_MAX_DIM;  // 3
constexpr int NG_OCCUPANCY = 2;                   // target mean rows per cell
constexpr int64_t NG_MAX_CELLS = (int64_t)1 << 24;
// causal queries with fewer candidates than ng_early(nr) go to the brute entry: walking E rows costs it about E microseconds, a grid walk
// at i candidates of nr rows about nr / i cells -- measured at both values on both sides of the switch
constexpr int64_t NG_EARLY_SMALL = 1024, NG_EARLY_LARGE = 4096, NG_EARLY_SWITCH = 65536;
inline int64_t ng_early(int64_t nr) { return nr < NG_EARLY_SWITCH ? NG_EARLY_SMALL : NG_EARLY_LARGE; }
constexpr int NG_THREADS = 256;
constexpr int NG_BOX_WGS = 256;                   // workgroups, and partials, of the box reduction
constexpr int NG_BOX_WORDS = 8;                   // doubles per partial: lo[3], hi[3], a flag for a coordinate that is not finite, unused
constexpr int NG_SCAN_ITEMS = 8;                  // entries per thread of the scan
constexpr int NG_SCAN_BLOCK = NG_THREADS * NG_SCAN_ITEMS;
constexpr int64_t NG_SCAN_MAX_BLOCKS = (NG_MAX_CELLS + 1 + NG_SCAN_BLOCK - 1) / NG_SCAN_BLOCK;
constexpr double NG_MAGIC = 1852729202.0;         // info[0]: 'nngr'
constexpr double NG_SLACK = 0x1p-40;              // absolute slack of a cell-coordinate gap, times (|t| + cells + 2)  
constexpr double NG_SHRINK = 1.0 - 0x1p-20;       // relative margin on the squared bound
constexpr double NG_BOUND_FLOOR = 1e-270;         // a bound below this stops nothing (the relative analysis needs normal numbers)

// info_host, FVGP_NN_GRID_INFO doubles
enum { NI_MAGIC = 0, NI_NR = 1, NI_D = 2, NI_SCALE = 3, NI_IS = 6, NI_LO = 9, NI_H = 12, NI_INVH = 13, NI_NC = 14, NI_CELLS = 17, NI_EARLY = 18 };

inline int64_t ng_cell_cap(int64_t nr) { return nr < NG_MAX_CELLS ? nr : NG_MAX_CELLS; }

// the grid buffer, every piece a multiple of 8 bytes: bucketed coordinates (nr, d) | start (cells + 1, at most cap + 1) | bucketed indices (nr)
struct NgGridBuf { double *bx; int *start, *bidx; };
inline NgGridBuf ng_grid_layout(Carve &c, int64_t nr, int d) {
    NgGridBuf l;
    l.bx = c.take<double>(nr * d, 8);
    l.start = c.take<int>(ng_cell_cap(nr) + 1, 8);
    l.bidx = c.take<int>(nr, 8);
    return l;
}

// what both the build and the search need of the grid.  Dimension k of the data sits in slot 3 - d + k: the last dimension is always slot
// 2, the one cells are contiguous along, and slots in front of the data's have one cell
struct NgGrid {
    int d, nc[3];
    double is[NG_MAX_DIM], lo[NG_MAX_DIM], h, invh;
};

// the cell coordinate of x[k] before flooring, and its cell: the SAME operations in the build and in the search, each monotone in x
__device__ __forceinline__ double ng_t(const NgGrid &g, const int k, const double x) { return ((x - g.lo[k]) * g.is[k]) * g.invh; }
__device__ __forceinline__ int ng_cell(const double t, const int nc) {
    return (int)fmin(fmax(t, 0.0), (double)(nc - 1));      // (fmax drops a NaN: cell 0)
}

// ------------------------------------------------------------------------------------------------------------------ build
struct NbArgs {
    const double *x;
    double *box;
    int *cid, *rank, *start, *bidx, *bsum;
    double *bx;
    long nr, len;                                  // len: entries of `start` (cells + 1)
    int nwg;
    NgGrid g;
};
// the build's workspace, every piece a multiple of 8 bytes: box partials | cell of every row | rank of every row in its cell | block
// sums of the scan; the pointers go into the build's arguments
inline void ng_work_layout(Carve &c, int64_t nr, NbArgs &a) {
    a.box = c.take<double>((int64_t)NG_BOX_WGS * NG_BOX_WORDS, 8);
    a.cid = c.take<int>(nr, 8);
    a.rank = c.take<int>(nr, 8);
    a.bsum = c.take<int>(NG_SCAN_MAX_BLOCKS, 8);
}

template <int D>
__global__ __launch_bounds__(NG_THREADS) void ng_box_kernel(NbArgs a) {
    __shared__ double s[NG_THREADS / 64][NG_BOX_WORDS];
    const int tid = threadIdx.x;
    double lo[D], hi[D], bad = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (long i = (long)blockIdx.x * NG_THREADS + tid; i < a.nr; i += (long)gridDim.x * NG_THREADS)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double v = a.x[i * D + k];
            if (!isfinite(v)) bad = 1.0;
            lo[k] = fmin(lo[k], v); hi[k] = fmax(hi[k], v);
        }
    // minima and maxima are exact: any order of joining them gives the same box
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < D; ++k) { lo[k] = fmin(lo[k], __shfl_down(lo[k], off, 64)); hi[k] = fmax(hi[k], __shfl_down(hi[k], off, 64)); }
        bad = fmax(bad, __shfl_down(bad, off, 64));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) { s[tid >> 6][k] = lo[k]; s[tid >> 6][3 + k] = hi[k]; }
        s[tid >> 6][6] = bad;
    }
    __syncthreads();
    if (tid == 0) {
        double *out = a.box + (long)blockIdx.x * NG_BOX_WORDS;
        for (int k = 0; k < 3; ++k) { out[k] = INFINITY; out[3 + k] = -INFINITY; }
        out[6] = 0.0; out[7] = 0.0;
        for (int w = 0; w < NG_THREADS / 64; ++w) {
            for (int k = 0; k < D; ++k) { out[k] = fmin(out[k], s[w][k]); out[3 + k] = fmax(out[3 + k], s[w][3 + k]); }
            out[6] = fmax(out[6], s[w][6]);
        }
    }
}

template <int D>
__device__ __forceinline__ int ng_cell_id(const NgGrid &g, const double *x) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) c = c * g.nc[3 - D + k] + ng_cell(ng_t(g, k, x[k]), g.nc[3 - D + k]);
    return c;
}

// every row's cell and its rank among the rows of that cell (the order of arrival); start[cell] counts
template <int D>
__global__ __launch_bounds__(NG_THREADS) void ng_count_kernel(NbArgs a) {
    const long i = (long)blockIdx.x * NG_THREADS + threadIdx.x;
    if (i >= a.nr) return;
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = a.x[i * D + k];
    const int c = ng_cell_id<D>(a.g, x);
    a.cid[i] = c;
    a.rank[i] = atomicAdd(a.start + c, 1);
}

// exclusive scan of start[0 .. len) in place: blocks of NG_SCAN_BLOCK entries scanned by themselves, bsum[block] <- the block's sum
__global__ __launch_bounds__(NG_THREADS) void ng_scan_blocks_kernel(NbArgs a) {
    __shared__ int s[NG_THREADS];
    const int tid = threadIdx.x;
    const long e0 = (long)blockIdx.x * NG_SCAN_BLOCK + (long)tid * NG_SCAN_ITEMS;
    int v[NG_SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int t = 0; t < NG_SCAN_ITEMS; ++t) { v[t] = e0 + t < a.len ? a.start[e0 + t] : 0; sum += v[t]; }
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < NG_THREADS; off <<= 1) {
        const int add = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    int run = s[tid] - sum;                        // the entries of the threads in front
#pragma unroll
    for (int t = 0; t < NG_SCAN_ITEMS; ++t) {
        if (e0 + t < a.len) a.start[e0 + t] = run;
        run += v[t];
    }
    if (tid == NG_THREADS - 1) a.bsum[blockIdx.x] = s[tid];
}

// bsum[0 .. nb) <- its exclusive scan, one workgroup: a run of consecutive entries per thread
__global__ __launch_bounds__(NG_THREADS) void ng_scan_sums_kernel(NbArgs a, int nb) {
    __shared__ int s[NG_THREADS];
    const int tid = threadIdx.x;
    const int per = (nb + NG_THREADS - 1) / NG_THREADS;
    const int b0 = tid * per, b1 = b0 + per < nb ? b0 + per : nb;
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += a.bsum[b];
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < NG_THREADS; off <<= 1) {
        const int add = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    int run = s[tid] - sum;
    for (int b = b0; b < b1; ++b) { const int v = a.bsum[b]; a.bsum[b] = run; run += v; }
}

__global__ __launch_bounds__(NG_THREADS) void ng_scan_add_kernel(NbArgs a) {
    const int add = a.bsum[blockIdx.x];
    const long e0 = (long)blockIdx.x * NG_SCAN_BLOCK;
    for (int t = threadIdx.x; t < NG_SCAN_BLOCK; t += NG_THREADS)
        if (e0 + t < a.len) a.start[e0 + t] += add;
}

// row i goes to start[its cell] + its rank: its index and a copy of its coordinates, so that a cell's rows are read together
template <int D>
__global__ __launch_bounds__(NG_THREADS) void ng_fill_kernel(NbArgs a) {
    const long i = (long)blockIdx.x * NG_THREADS + threadIdx.x;
    if (i >= a.nr) return;
    const long p = (long)a.start[a.cid[i]] + a.rank[i];
    if (p < 0 || p >= a.nr) return;                // (never taken: the ranks of a cell are 0 .. its count - 1)
    a.bidx[p] = (int)i;
#pragma unroll
    for (int k = 0; k < D; ++k) a.bx[p * D + k] = a.x[i * D + k];
}

// ------------------------------------------------------------------------------------------------------------------ search
struct NgArgs {
    const double *xq, *bx;
    const int *start, *bidx;
    int *out;
    long nq, nr, ld, c0;
    int m, shells;                                 // shells: the most cells of one dimension
    NgGrid g;
};

template <int D, int M>      // M: list capacity, m <= M
__global__ __launch_bounds__(64) void nn_grid_search_kernel(NgArgs a) {
    __shared__ double sd[M * 64];                  // [slot][lane]
    __shared__ int si[M * 64];
    const int lane = threadIdx.x, m = a.m;
    const long q = (long)blockIdx.x * 64 + lane;
    if (q >= a.nq) return;                         // (no barrier below: a lane touches its own column of the lists alone)
    const long lim = a.c0 >= 0 ? (a.c0 + q < a.nr ? a.c0 + q : a.nr) : a.nr;
    double u[D], is[D];
    // slot s of the grid: the query's cell cq, the gaps from the query to its cell's lower and upper face in cells (negative or past 1
    // where the query was clamped into the grid from outside), and the slack of a gap
    int cq[3] = {0, 0, 0}, nc[3];
    double glo[3] = {0.0, 0.0, 0.0}, ghi[3] = {0.0, 0.0, 0.0}, slack[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 3; ++s) nc[s] = a.g.nc[s];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        u[k] = a.xq[q * D + k]; is[k] = a.g.is[k];
        const int s = 3 - D + k;
        const double t = ng_t(a.g, k, u[k]);
        cq[s] = ng_cell(t, nc[s]);
        glo[s] = t - (double)cq[s];
        ghi[s] = (double)(cq[s] + 1) - t;
        slack[s] = NG_SLACK * (fabs(t) + (double)(nc[s] + 2));
    }
    NnTop t;

    // the bucketed rows p0 .. p1 - 1 into the list, sorted by (distance, index)
    auto visit = [&](const int p0, const int p1) {
        for (int p = p0; p < p1; ++p) {
            const int j = a.bidx[p];
            if (j >= lim) continue;
            nn_top_insert<true>(t, sd, si, lane, m, nn_dist2<D>(u, a.bx + (long)p * D, is, D), j);
        }
    };
    // the cells (c0, c1, l2 .. h2), contiguous in the buckets
    auto run = [&](const int c0, const int c1, const int l2, const int h2) {
        if (l2 > h2) return;
        const long base = ((long)c0 * nc[1] + c1) * nc[2];
        visit(a.start[base + l2], a.start[base + h2 + 1]);
    };
    int last = 0;                                  // the farthest shell that holds a cell
#pragma unroll
    for (int s = 0; s < 3; ++s) { last = max(last, cq[s]); last = max(last, nc[s] - 1 - cq[s]); }

    for (int R = 0; R < a.shells; ++R) {
        if (R > last) break;
        // shell R: the cells at Chebyshev distance exactly R from cq, clipped to the grid
        const int l0 = max(cq[0] - R, 0), h0 = min(cq[0] + R, nc[0] - 1);
        const int l1 = max(cq[1] - R, 0), h1 = min(cq[1] + R, nc[1] - 1);
        const int l2 = max(cq[2] - R, 0), h2 = min(cq[2] + R, nc[2] - 1);
        for (int c0 = l0; c0 <= h0; ++c0) {
            const bool b0 = c0 - cq[0] == R || cq[0] - c0 == R;
            for (int c1 = l1; c1 <= h1; ++c1) {
                if (b0 || c1 - cq[1] == R || cq[1] - c1 == R) run(c0, c1, l2, h2);
                else {
                    if (cq[2] - R >= 0) run(c0, c1, cq[2] - R, cq[2] - R);
                    if (R > 0 && cq[2] + R <= nc[2] - 1) run(c0, c1, cq[2] + R, cq[2] + R);
                }
            }
        }
        if (t.cnt < m) continue;
        // ng_stop_bound: a row in a cell outside shells 0 .. R lies, in some slot s, at least R + 1 cells above or below cq[s]; its
        // computed cell coordinate then differs from the query's by at least the gap to that face plus R
        double bound = INFINITY;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (cq[s] + R + 1 <= nc[s] - 1) { const double g = fmax(ghi[s] + (double)R - slack[s], 0.0) * a.g.h; bound = fmin(bound, g * g); }
            if (cq[s] - R - 1 >= 0) { const double g = fmax(glo[s] + (double)R - slack[s], 0.0) * a.g.h; bound = fmin(bound, g * g); }
        }
        bound *= NG_SHRINK;
        if (bound >= NG_BOUND_FLOOR && t.worst < bound) break;
    }
    for (int p = 0; p < m; ++p) a.out[q * a.ld + p] = p < t.cnt ? si[p * 64 + lane] : -1;
}

inline bool pos_finite(double v) { return v > 0.0 && std::isfinite(v); }
inline bool whole(double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); }

// the grid of an info record that fits (nr, d); false where it does not
inline bool ng_from_info(const double *info, int64_t nr, int d, NgGrid *g, int64_t *cells) {
    if (info[NI_MAGIC] != NG_MAGIC || info[NI_NR] != (double)nr || info[NI_D] != (double)d) return false;
    g->d = d;
    for (int s = 0; s < 3; ++s) g->nc[s] = 1;
    int64_t prod = 1;
    for (int k = 0; k < NG_MAX_DIM; ++k) {
        g->is[k] = 1.0; g->lo[k] = 0.0;
        if (k >= d) continue;
        if (!pos_finite(info[NI_SCALE + k]) || !pos_finite(info[NI_IS + k]) || !std::isfinite(info[NI_LO + k])) return false;
        if (!whole(info[NI_NC + k], 1.0, (double)NG_MAX_CELLS)) return false;
        g->is[k] = info[NI_IS + k]; g->lo[k] = info[NI_LO + k];
        g->nc[3 - d + k] = (int)info[NI_NC + k];
        prod *= (int64_t)info[NI_NC + k];
        if (prod > NG_MAX_CELLS) return false;
    }
    if (!pos_finite(info[NI_H]) || !pos_finite(info[NI_INVH])) return false;
    if (info[NI_CELLS] != (double)prod || prod > ng_cell_cap(nr)) return false;
    g->h = info[NI_H]; g->invh = info[NI_INVH];
    *cells = prod;
    return true;
}

// cells per dimension for extents ext[k] >= 0 (scaled): cubic cells of edge h, about NG_OCCUPANCY rows each, at most cap cells; a
// dimension of no extent, or thinner than a cell, has one cell.  Returns h; nc[k] >= every row's (x - lo) is invh there.
inline double ng_choose(const double *ext, int d, int64_t nr, int64_t cap, int64_t *nc) {
    for (int k = 0; k < d; ++k) nc[k] = 1;
    const double target = (double)std::max<int64_t>(1, std::min(cap, (nr + NG_OCCUPANCY - 1) / NG_OCCUPANCY));
    bool on[NG_MAX_DIM];
    int na = 0;
    for (int k = 0; k < d; ++k) { on[k] = ext[k] > 0.0; na += on[k]; }
    double h = 0.0;
    for (int pass = 0; pass < NG_MAX_DIM && na > 0; ++pass) {      // dimensions thinner than a cell leave, the others share the cells
        double logvol = 0.0;
        for (int k = 0; k < d; ++k) if (on[k]) logvol += std::log(ext[k]);
        h = std::exp((logvol - std::log(target)) / na);
        bool dropped = false;
        for (int k = 0; k < d; ++k) if (on[k] && ext[k] < h) { on[k] = false; --na; dropped = true; }
        if (!dropped) break;
    }
    if (na == 0 || !pos_finite(h) || !pos_finite(1.0 / h)) return 1.0;      // one cell
    for (int grow = 0; grow < 400; ++grow, h *= 1.25) {
        const double invh = 1.0 / h;
        if (!pos_finite(h) || !pos_finite(invh)) break;
        int64_t prod = 1;
        bool fits = true;
        for (int k = 0; k < d && fits; ++k) {
            const double t = ext[k] * invh;        // the device's cell coordinate of a row on the upper face
            if (!(t < (double)NG_MAX_CELLS)) { fits = false; break; }
            nc[k] = std::max<int64_t>(1, (int64_t)std::ceil(t));
            prod *= nc[k];
            if (prod > cap) fits = false;
        }
        if (fits) return h;
    }
    for (int k = 0; k < d; ++k) nc[k] = 1;
    return 1.0;
}

}  // namespace

extern "C" {

int64_t fvgp_hip_nn_grid_bytes(int64_t nr, int d) {
    if (nr < 1 || nr > 0x7fffffffLL || d < 1 || d > NG_MAX_DIM) return -1;
    return carve_bytes(ng_grid_layout, nr, d);
}

int64_t fvgp_hip_nn_grid_workspace_bytes(int64_t nr, int d) {
    if (nr < 1 || nr > 0x7fffffffLL || d < 1 || d > NG_MAX_DIM) return -1;
    return carve_bytes_for<NbArgs>(ng_work_layout, nr);
}

int fvgp_hip_nn_grid_build(fvgp_handle *h, const double *xr, int64_t nr, int d, const double *scales_host, void *grid_dev,
                           int64_t grid_bytes, void *work, int64_t work_bytes, double *info_host) {
    static_assert(FVGP_NN_GRID_INFO > NI_EARLY, "the info record");
    if (!h) return -1;
    if (!xr) return -2;
    if (nr < 1 || nr > 0x7fffffffLL) return -3;
    if (d < 1 || d > NG_MAX_DIM) { fvgp_set_error("nn_grid_build: the cell grid takes 1 .. 3 dimensions; fvgp_hip_nn_search has no such limit"); return -4; }
    double scale[NG_MAX_DIM], is[NG_MAX_DIM];
    if (!nn_scales("nn_grid_build", scales_host, d, NG_MAX_DIM, is, scale)) return -5;
    if (!grid_dev || ((uintptr_t)grid_dev & 7)) return -6;
    Carve gc(grid_dev), wc(work); const NgGridBuf gl = ng_grid_layout(gc, nr, d);
    NbArgs a;
    ng_work_layout(wc, nr, a);
    if (grid_bytes < gc.bytes()) { fvgp_set_error("nn_grid_build: grid buffer smaller than fvgp_hip_nn_grid_bytes(nr, d)"); return -7; }
    if (!work || ((uintptr_t)work & 7)) return -8;
    if (work_bytes < wc.bytes()) {
        fvgp_set_error("nn_grid_build: work smaller than fvgp_hip_nn_grid_workspace_bytes(nr, d)"); return -9;
    }
    if (!info_host) return -10;
    HIPCHK(hipSetDevice(h->device));
    a.x = xr; a.nr = nr;
    a.bx = gl.bx; a.start = gl.start; a.bidx = gl.bidx;
    a.nwg = (int)std::min<int64_t>(NG_BOX_WGS, (nr + NG_THREADS - 1) / NG_THREADS);
    a.len = 0; a.g = NgGrid{};
    // 1. the box
    dispatch_dim3(d, [&](auto D) { hipLaunchKernelGGL((ng_box_kernel<decltype(D)::value>), dim3((unsigned)a.nwg), dim3(NG_THREADS), 0, h->stream, a); });
    HIPCHK(hipGetLastError());
    std::vector<double> part((size_t)a.nwg * NG_BOX_WORDS);
    HIPCHK(hipMemcpyAsync(part.data(), a.box, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    double lo[NG_MAX_DIM], hi[NG_MAX_DIM], ext[NG_MAX_DIM], bad = 0.0;
    for (int k = 0; k < NG_MAX_DIM; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (int w = 0; w < a.nwg; ++w) {
        const double *p = part.data() + (size_t)w * NG_BOX_WORDS;
        for (int k = 0; k < d; ++k) { lo[k] = std::fmin(lo[k], p[k]); hi[k] = std::fmax(hi[k], p[3 + k]); }
        bad = std::fmax(bad, p[6]);
    }
    for (int k = 0; k < d; ++k) {
        ext[k] = (hi[k] - lo[k]) * is[k];
        if (bad != 0.0 || !std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !std::isfinite(ext[k])) {
            fvgp_set_error("nn_grid_build: the reference rows' bounding box is not finite"); return -11;
        }
    }
    // 2. the cells
    int64_t nc[NG_MAX_DIM] = {1, 1, 1}, cells = 1;
    const double edge = ng_choose(ext, d, nr, ng_cell_cap(nr), nc);
    a.g.d = d; a.g.h = edge; a.g.invh = 1.0 / edge;
    for (int s = 0; s < 3; ++s) a.g.nc[s] = 1;
    for (int k = 0; k < NG_MAX_DIM; ++k) { a.g.is[k] = is[k]; a.g.lo[k] = k < d ? lo[k] : 0.0; }
    for (int k = 0; k < d; ++k) { a.g.nc[3 - d + k] = (int)nc[k]; cells *= nc[k]; }
    a.len = cells + 1;
    // 3. cells of the rows, counts, scan, buckets
    const dim3 rows((unsigned)((nr + NG_THREADS - 1) / NG_THREADS)), threads(NG_THREADS);
    const int nb = (int)((a.len + NG_SCAN_BLOCK - 1) / NG_SCAN_BLOCK);
    HIPCHK(hipMemsetAsync(a.start, 0, (size_t)a.len * sizeof(int), h->stream));
    dispatch_dim3(d, [&](auto D) { hipLaunchKernelGGL((ng_count_kernel<decltype(D)::value>), rows, threads, 0, h->stream, a); });
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ng_scan_blocks_kernel, dim3((unsigned)nb), threads, 0, h->stream, a);
    hipLaunchKernelGGL(ng_scan_sums_kernel, dim3(1), threads, 0, h->stream, a, nb);
    hipLaunchKernelGGL(ng_scan_add_kernel, dim3((unsigned)nb), threads, 0, h->stream, a);
    HIPCHK(hipGetLastError());
    dispatch_dim3(d, [&](auto D) { hipLaunchKernelGGL((ng_fill_kernel<decltype(D)::value>), rows, threads, 0, h->stream, a); });
    HIPCHK(hipGetLastError());
    for (int k = 0; k < FVGP_NN_GRID_INFO; ++k) info_host[k] = 0.0;
    info_host[NI_MAGIC] = NG_MAGIC; info_host[NI_NR] = (double)nr; info_host[NI_D] = (double)d;
    for (int k = 0; k < NG_MAX_DIM; ++k) {
        info_host[NI_SCALE + k] = scale[k]; info_host[NI_IS + k] = is[k];
        info_host[NI_LO + k] = k < d ? lo[k] : 0.0; info_host[NI_NC + k] = (double)nc[k];
    }
    info_host[NI_H] = a.g.h; info_host[NI_INVH] = a.g.invh; info_host[NI_CELLS] = (double)cells; info_host[NI_EARLY] = (double)ng_early(nr);
    return 0;
}

int fvgp_hip_nn_grid_search(fvgp_handle *h, const double *xq, int64_t nq, const double *xr, int64_t nr, int d, int m, int64_t c0,
                            const double *info_host, const void *grid_dev, int *idx_out, int64_t ld) {
    if (!h) return -1;
    if (!xq) return -2;
    if (nq < 1 || (nq + 63) / 64 > 0x7fffffffLL) return -3;
    if (!xr) return -4;
    if (nr < 1 || nr > 0x7fffffffLL) return -5;
    if (d < 1 || d > NG_MAX_DIM) { fvgp_set_error("nn_grid_search: the cell grid takes 1 .. 3 dimensions"); return -6; }
    if (m < 1 || m > FVGP_NN_MAX_NEIGHBORS) { fvgp_set_error("nn_grid_search: 1 .. FVGP_NN_MAX_NEIGHBORS neighbours"); return -8; }
    NgArgs a;
    int64_t cells = 0;
    if (!info_host || !ng_from_info(info_host, nr, d, &a.g, &cells)) {
        fvgp_set_error("nn_grid_search: info_host is not what fvgp_hip_nn_grid_build left for these (nr, d)"); return -9;
    }
    if (!idx_out) return -10;
    if (ld < m) return -11;
    if (!grid_dev || ((uintptr_t)grid_dev & 7)) return -12;
    HIPCHK(hipSetDevice(h->device));
    // the early rows of a causal call: the brute entry, under the scales the grid was built with (1 / scale gives the same bits there)
    int64_t early = 0;
    if (c0 >= 0 && c0 < ng_early(nr)) {
        early = std::min<int64_t>(nq, ng_early(nr) - c0);
        const int rc = fvgp_hip_nn_search(h, xq, early, xr, nr, d, info_host + NI_SCALE, m, c0, idx_out, ld);
        if (rc) return rc;
        if (early == nq) return 0;
    }
    Carve gc(const_cast<void *>(grid_dev));                       // (the search only reads the grid)
    const NgGridBuf gl = ng_grid_layout(gc, nr, d);
    a.bx = gl.bx; a.start = gl.start; a.bidx = gl.bidx;
    a.xq = xq + early * d; a.out = idx_out + early * ld;
    a.nq = nq - early; a.nr = nr; a.ld = ld; a.c0 = c0 < 0 ? -1 : c0 + early; a.m = m;
    a.shells = std::max(a.g.nc[0], std::max(a.g.nc[1], a.g.nc[2]));
    const dim3 grid((unsigned)((a.nq + 63) / 64)), block(64);
    dispatch_dim3(d, [&](auto D) {
        dispatch_pad(m, [&](auto M) {
            hipLaunchKernelGGL((nn_grid_search_kernel<decltype(D)::value, decltype(M)::value>), grid, block, 0, h->stream, a);
        });
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
