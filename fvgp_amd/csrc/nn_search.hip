// The brute-force neighbour search of the nearest-neighbour path (include/fvgp_hip_nn.h).
// fvgp_hip_nn_search        the m nearest candidates of every query: a wavefront per 64 queries, a lane per query, the reference rows
//     staged through LDS in slices (every lane reads the same row: broadcast reads), each lane's running top-m in LDS (nn_geometry.h:
//     nn_top_insert by distance alone).  Rows are walked in ascending index, so ties stay with the lower index.
#include "nn_geometry.h"
#include "../../include/fvgp_hip_nn.h"

namespace {

constexpr int NN_SEARCH_ROWS = 128;               // reference rows per staged slice of the search
constexpr int NN_SEARCH_QUERIES = 65536;          // queries per launch of the search

struct NsArgs {
    const double *xq, *xr;
    int *out;
    long nq, nr, ld, c0;
    int d, m;
    double is[FVGP_MAX_DIM];                       // 1 / scale per dimension (1: unscaled)
};

template <int D, int M>      // D == 0: runtime dimension (<= FVGP_MAX_DIM); M: list capacity, m <= M
__global__ __launch_bounds__(64) void nn_search_kernel(NsArgs a) {
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    __shared__ double sx[NN_SEARCH_ROWS * DD];
    __shared__ double sd[M * 64];                  // [slot][lane]
    __shared__ int si[M * 64];
    const int d = D ? D : a.d, m = a.m;
    const int lane = threadIdx.x;
    const long q0 = (long)blockIdx.x * 64, q = q0 + lane;
    const long qi = q < a.nq ? q : a.nq - 1;
    double u[DD], is[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) { u[k] = k < d ? a.xq[qi * d + k] : 0.0; is[k] = a.is[k]; }
    // candidates of this lane [0, lim) and of the block [0, top)
    long lim = a.nr, top = a.nr;
    if (a.c0 >= 0) {
        lim = a.c0 + q < a.nr ? a.c0 + q : a.nr;
        const long ql = q0 + 63 < a.nq ? q0 + 63 : a.nq - 1;
        top = a.c0 + ql < a.nr ? a.c0 + ql : a.nr;
    }
    if (q >= a.nq) lim = 0;
    NnTop t;

    for (long row0 = 0; row0 < top; row0 += NN_SEARCH_ROWS) {
        __syncthreads();                           // the last slice has been read
        const int rows = top - row0 < NN_SEARCH_ROWS ? (int)(top - row0) : NN_SEARCH_ROWS;
        for (int e = lane; e < rows * d; e += 64) {
            const int rr = e / d, kk = e - rr * d;
            sx[rr * DD + kk] = a.xr[(row0 + rr) * d + kk];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const double dist = nn_dist2<DD>(u, sx + r * DD, is, d);
            const long j = row0 + r;
            if (j < lim) nn_top_insert<false>(t, sd, si, lane, m, dist, (int)j);
        }
    }
    if (q >= a.nq) return;
    for (int p = 0; p < m; ++p) a.out[q * a.ld + p] = p < t.cnt ? si[p * 64 + lane] : -1;
}

}  // namespace

extern "C" int fvgp_hip_nn_search(fvgp_handle *h, const double *xq, int64_t nq, const double *xr, int64_t nr, int d,
                                  const double *scales_host, int m, int64_t c0, int *idx_out, int64_t ld) {
    if (!h) return -1;
    if (!xq) return -2;
    if (nq < 1 || (nq + 63) / 64 > 0x7fffffffLL) return -3;
    if (!xr) return -4;
    if (nr < 1 || nr > 0x7fffffffLL) return -5;
    if (d < 1 || d > FVGP_MAX_DIM) { fvgp_set_error("input dimension out of range"); return -6; }
    NsArgs a;
    if (!nn_scales("nn_search", scales_host, d, FVGP_MAX_DIM, a.is)) return -7;
    if (m < 1 || m > FVGP_NN_MAX_NEIGHBORS) { fvgp_set_error("nn_search: 1 .. FVGP_NN_MAX_NEIGHBORS neighbours"); return -8; }
    if (!idx_out) return -10;
    if (ld < m) return -11;
    HIPCHK(hipSetDevice(h->device));
    a.xr = xr; a.nr = nr; a.ld = ld; a.d = d; a.m = m;
    // a launch per NN_SEARCH_QUERIES queries (a row's result does not depend on the cut): no single launch walks 10^6 x 10^6 pairs
    for (int64_t q0 = 0; q0 < nq; q0 += NN_SEARCH_QUERIES) {
        a.xq = xq + q0 * d; a.out = idx_out + q0 * ld;
        a.nq = nq - q0 < NN_SEARCH_QUERIES ? nq - q0 : NN_SEARCH_QUERIES;
        a.c0 = c0 < 0 ? -1 : c0 + q0;
        const dim3 grid((unsigned)((a.nq + 63) / 64)), block(64);
        dispatch_dim(d, [&](auto D) {
            dispatch_pad(m, [&](auto M) {
                hipLaunchKernelGGL((nn_search_kernel<decltype(D)::value, decltype(M)::value>), grid, block, 0, h->stream, a);
            });
        });
        HIPCHK(hipGetLastError());
    }
    return 0;
}
