// The neighbour geometry of the nearest-neighbour path, written once for the brute search (nn_search.hip), the maxmin ordering
// (nn_order.hip) and the cell-grid search (nn_grid.hip): the scaled squared distance, the sorted top-m list of a lane, the dimension and
// list-size dispatch, and the host's check of the scales.  What the path promises -- the grid returns the brute lists element
// for element, the ordering's distances are the search's -- holds because all three call nn_dist2 and take 1 / scale from nn_scales.
#pragma once
#include "common.h"
#include <cmath>
#include <type_traits>

namespace {

// sum_k ((a_k - b_k) * is_k)^2 over k < d, ascending k, every square fused into the sum.  DD: the compile-time bound of d (the arrays'
// length where they are registers); DD == FVGP_MAX_DIM with a runtime d is the generic case.  The result's bits do not depend on which of
// a and b is the point held in registers: the difference is squared.
template <int DD>
__device__ __forceinline__ double nn_dist2(const double *a, const double *b, const double *is, const int d) {
    double dist = 0.0;
#pragma unroll
    for (int k = 0; k < DD; ++k)
        if (k < d) { const double e = (a[k] - b[k]) * is[k]; dist = fma(e, e, dist); }
    return dist;
}

// A lane's running top-m list in LDS, sorted ascending, slot-major (sd / si [slot][lane]: lanes touching the same slot never meet on a
// bank); `worst` (and `worst_i`) cache the last entry once the list is full, so most candidates are turned away without an LDS read.
struct NnTop { int cnt = 0, worst_i = 0; double worst = INFINITY; };

// the entry (pd, pi) comes behind the candidate (dist, j)
template <bool BY_INDEX>
__device__ __forceinline__ bool nn_behind(const double pd, const int pi, const double dist, const int j) {
    if constexpr (BY_INDEX) return pd > dist || (pd == dist && pi > j);
    else return pd > dist;
}

// candidate (dist, j) into the list of capacity m, by insertion from the end.  BY_INDEX false: the order is the distance alone and an
// entry moves only for a strictly smaller one -- candidates that arrive in ascending index keep ties with the lower index, and no index
// is compared.  BY_INDEX true: the order is the pair (distance, index), for candidates in any order.
template <bool BY_INDEX>
__device__ __forceinline__ void nn_top_insert(NnTop &t, double *sd, int *si, const int lane, const int m, const double dist, const int j) {
    bool in = t.cnt < m || dist < t.worst;
    if constexpr (BY_INDEX) in = in || (dist == t.worst && j < t.worst_i);
    if (!in) return;
    int p = t.cnt < m ? t.cnt : m - 1;             // the slot that opens: behind the list, or its last entry drops out
    while (p > 0 && nn_behind<BY_INDEX>(sd[(p - 1) * 64 + lane], si[(p - 1) * 64 + lane], dist, j)) {
        sd[p * 64 + lane] = sd[(p - 1) * 64 + lane];
        si[p * 64 + lane] = si[(p - 1) * 64 + lane];
        --p;
    }
    sd[p * 64 + lane] = dist;
    si[p * 64 + lane] = j;
    if (t.cnt < m) ++t.cnt;
    if (t.cnt == m) { t.worst = sd[(m - 1) * 64 + lane]; if constexpr (BY_INDEX) t.worst_i = si[(m - 1) * 64 + lane]; }
}

// f(std::integral_constant<int, D>) with the dimensions that have an instantiation of their own (those of dispatch_kind_dim); D = 0 is
// the runtime dimension (<= FVGP_MAX_DIM)
template <class F>
inline void dispatch_dim(int d, F &&f) {
    switch (d) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 0>{}); break;
    }
}

// ... and for the cell grid, whose dimensions (1 .. 3, checked by the caller) all have one
template <class F>
inline void dispatch_dim3(int d, F &&f) {
    switch (d) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        default: f(std::integral_constant<int, 3>{}); break;
    }
}

// f(std::integral_constant<int, M>) for the padded size of m neighbours
template <class F>
inline void dispatch_pad(int m, F &&f) {
    if (m <= 16) f(std::integral_constant<int, 16>{});
    else if (m <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

// is[0 .. len) <- 1 / scale per dimension, 1 where there is none (scales_host NULL: everywhere); scale[0 .. len), where the caller keeps
// the scales themselves, likewise.  False, with the error text set under the entry's name `who`, for a scale that is not positive and
// finite; the entry returns its own code.
inline bool nn_scales(const char *who, const double *scales_host, int d, int len, double *is, double *scale = nullptr) {
    for (int k = 0; k < len; ++k) { is[k] = 1.0; if (scale) scale[k] = 1.0; }
    if (scales_host)
        for (int k = 0; k < d; ++k) {
            if (!(scales_host[k] > 0.0) || !std::isfinite(scales_host[k])) { fvgp_set_error(std::string(who) + ": scales must be positive and finite"); return false; }
            is[k] = 1.0 / scales_host[k]; if (scale) scale[k] = scales_host[k];
        }
    return true;
}

}  // namespace
