// The running best {score, index} of an argmax with ties to the lowest index: one definition of the order and of the wave's reduction,
// for the pick and the 64-candidate partials of the greedy pivot core (pivot.h).
#pragma once
#include "common.h"

namespace {

struct Best { double score; long idx; };     // idx < 0: none
__device__ __forceinline__ bool better(const Best a, const Best b) {
    return a.idx >= 0 && (b.idx < 0 || a.score > b.score || (a.score == b.score && a.idx < b.idx));
}
__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Best o;
        o.score = __shfl_down(b.score, off, 64);
        o.idx = __shfl_down(b.idx, off, 64);
        if (better(o, b)) b = o;
    }
    return b;
}

}  // namespace
