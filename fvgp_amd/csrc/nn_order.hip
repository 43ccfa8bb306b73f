// The maxmin (farthest-point, coarse-to-fine) ordering of the nearest-neighbour path (include/fvgp_hip_nn.h): perm[0] = first,
// perm[t] = the point not picked yet that lies farthest from the t points picked before it, ties to the lowest index.
// fvgp_hip_nn_maxmin_order   q launches of ONE kernel in stream order, nothing else synchronises.  Every workgroup owns a fixed strip of
//     points, a few per thread, and keeps their distance to the nearest pick in the workspace (-1: picked).  The launch of step t
//       1. reduces the partials {score, index} that step t - 1 left, one per workgroup, to the pick j -- every workgroup for itself, all
//          to the same j, since the order of argmax.h (ties to the lowest index) makes the argmax associative; workgroup 0 records it;
//       2. lowers its own points' distances by the one to x_j (nn_geometry.h: nn_dist2) and leaves its best point as its partial in the
//          OTHER of two partial arrays (t & 1): a workgroup may still read step t - 1's while another writes step t's.
//     Step 0 takes j = first and sets the distances instead of lowering them.  No atomics, no communication inside a launch, every loop
//     bounded by launch arguments.  O(q n d) flops; a step reads 8 (d + 1) bytes per point not picked yet and writes the distances that fell.
#include "argmax.h"
#include "nn_geometry.h"
#include "../../include/fvgp_hip_nn.h"

namespace {

constexpr int NO_THREADS = 256;                   // threads per workgroup
constexpr int NO_MAX_WGS = 512;                   // most workgroups, and with them partials, of a step

struct NoArgs {
    const double *x;
    double *mind;                                  // (n) squared scaled distance to the nearest pick; -1 once picked
    Best *part;                                    // (2, NO_MAX_WGS) the workgroups' best points: step t writes row t & 1
    long long *perm;
    double *dist;                                  // or nullptr
    long n, first, strip;                          // strip: points per workgroup (a multiple of NO_THREADS)
    int d, t, nwg;
    double is[FVGP_MAX_DIM];                       // 1 / scale per dimension (1: unscaled)
};

// the workgroup's best of the threads' b, in every thread
__device__ __forceinline__ Best block_best(Best b, Best *sb) {
    const int tid = threadIdx.x;
    b = wave_best(b);
    __syncthreads();                               // (sb's last use has been read)
    if ((tid & 63) == 0) sb[tid >> 6] = b;
    __syncthreads();
    b = sb[0];
#pragma unroll
    for (int w = 1; w < NO_THREADS / 64; ++w)
        if (better(sb[w], b)) b = sb[w];
    return b;
}

template <int D>      // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(NO_THREADS) void nn_maxmin_step_kernel(NoArgs a) {
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    __shared__ Best sb[NO_THREADS / 64];
    const int d = D ? D : a.d;
    const int tid = threadIdx.x;
    long j = a.first;
    if (a.t > 0) {
        const Best *prev = a.part + (long)((a.t & 1) ^ 1) * NO_MAX_WGS;
        Best b{0.0, -1};
        for (int k = tid; k < a.nwg; k += NO_THREADS) {
            const Best o = prev[k];
            if (better(o, b)) b = o;
        }
        b = block_best(b, sb);
        j = b.idx;
        if (j < 0 || j >= a.n) return;             // (uniform, and never taken: q <= n leaves a point to pick at every step)
        if (blockIdx.x == 0 && tid == 0) { a.perm[a.t] = j; if (a.dist) a.dist[a.t] = b.score; }
    } else if (blockIdx.x == 0 && tid == 0) {
        a.perm[0] = j; if (a.dist) a.dist[0] = INFINITY;
    }
    double xj[DD], is[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) { xj[k] = k < d ? a.x[j * d + k] : 0.0; is[k] = a.is[k]; }
    const long s0 = (long)blockIdx.x * a.strip;
    const long s1 = s0 + a.strip < a.n ? s0 + a.strip : a.n;
    Best b{0.0, -1};
    for (long i = s0 + tid; i < s1; i += NO_THREADS) {
        const double m0 = a.t > 0 ? a.mind[i] : INFINITY;
        double m = m0;
        if (i == j) m = -1.0;
        else if (m >= 0.0) {
            double dist = nn_dist2<DD>(a.x + i * d, xj, is, d);
            if (!(dist >= 0.0)) dist = 0.0;        // a distance that is no number counts as 0: the order stays total
            if (dist < m) m = dist;
        }
        if (a.t == 0 || m != m0) a.mind[i] = m;
        const Best o{m, m >= 0.0 ? i : -1};
        if (better(o, b)) b = o;                   // (ascending i per thread: the strict order keeps the lowest index)
    }
    b = block_best(b, sb);
    if (tid == 0) a.part[(long)(a.t & 1) * NO_MAX_WGS + blockIdx.x] = b;
}

// the workspace: the n distances, then the two rows of partials; the pointers go into the steps' arguments
inline void no_layout(Carve &c, int64_t n, NoArgs &a) {
    a.mind = c.take<double>(n);
    a.part = c.take<Best>(2 * NO_MAX_WGS);
}

}  // namespace

extern "C" {

int64_t fvgp_hip_nn_maxmin_workspace_bytes(int64_t n) {
    if (n < 1) return -1;
    return carve_bytes_for<NoArgs>(no_layout, n);
}

int fvgp_hip_nn_maxmin_order(fvgp_handle *h, const double *x, int64_t n, int d, const double *scales_host, int64_t first, int64_t q,
                             int64_t *perm_out, double *dist_out, double *work, int64_t work_bytes) {
    static_assert(sizeof(Best) == 2 * sizeof(double) && sizeof(long long) == sizeof(int64_t), "the workspace layout, the picks' type");
    if (!h) return -1;
    if (!x) return -2;
    if (n < 1 || n > 0x7fffffffLL) return -3;
    if (d < 1 || d > FVGP_MAX_DIM) { fvgp_set_error("input dimension out of range"); return -4; }
    NoArgs a;
    if (!nn_scales("nn_maxmin_order", scales_host, d, FVGP_MAX_DIM, a.is)) return -5;
    if (first < 0 || first >= n) { fvgp_set_error("nn_maxmin_order: first must be one of the n points"); return -6; }
    if (q < 1 || q > n) { fvgp_set_error("nn_maxmin_order: 1 .. n points to order"); return -7; }
    if (!perm_out) return -8;
    if (!work || ((uintptr_t)work & 7)) return -10;
    Carve c(work); no_layout(c, n, a);
    if (work_bytes < c.bytes()) {
        fvgp_set_error("nn_maxmin_order: work smaller than fvgp_hip_nn_maxmin_workspace_bytes(n)"); return -11;
    }
    HIPCHK(hipSetDevice(h->device));
    // strips of whole workgroup widths, as few per workgroup as NO_MAX_WGS workgroups allow; no workgroup without a point
    const int64_t per = (n + NO_MAX_WGS - 1) / NO_MAX_WGS;
    a.strip = (per + NO_THREADS - 1) / NO_THREADS * NO_THREADS;
    a.nwg = (int)((n + a.strip - 1) / a.strip);
    a.x = x;
    a.perm = reinterpret_cast<long long *>(perm_out); a.dist = dist_out;
    a.n = n; a.first = first; a.d = d;
    for (int64_t t = 0; t < q; ++t) {
        a.t = (int)t;
        dispatch_dim(d, [&](auto D) {
            hipLaunchKernelGGL((nn_maxmin_step_kernel<decltype(D)::value>), dim3((unsigned)a.nwg), dim3(NO_THREADS), 0, h->stream, a);
        });
        HIPCHK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
