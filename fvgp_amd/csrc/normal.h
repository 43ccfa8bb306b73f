// z(seed, stream, i, j), the stateless normal generator of fvgp_hip_normal_fill (sample.hip: the fill and the joint draws; matrix_free.hip:
// the probes of the stochastic log-likelihood).  One definition, so that every caller evaluates an element with the same operations.
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr double TWO_PI = 6.283185307179586476925286766559;
constexpr double TWO_M53 = 1.0 / 9007199254740992.0;

__device__ __forceinline__ double normal_at(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, uint32_t i, uint32_t j) {
    uint32_t c0 = i, c1 = j, c2 = s0, c3 = s1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    const uint64_t a = ((uint64_t)c0 | ((uint64_t)c1 << 32)) >> 11, b = ((uint64_t)c2 | ((uint64_t)c3 << 32)) >> 11;
    const double u1 = ((double)a + 0.5) * TWO_M53, u2 = ((double)b + 0.5) * TWO_M53;
    return sqrt(-2.0 * log(u1)) * cos(TWO_PI * u2);
}

}  // namespace
