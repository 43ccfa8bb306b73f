// Radial functions of the stationary kernels (kmat.hip: the covariance assembly and its gradient; batch.hip: the batched
// assembly).  One definition, so that every assembly computes an entry with the same operations.
#pragma once
#include "common.h"

namespace {

constexpr double SQRT3 = 1.7320508075688772935;
constexpr double SQRT5 = 2.2360679774997896964;

// exp(-a) for a >= 0, a streaming kernel's version: Cody-Waite reduction a = n ln2 + r, |r| <= ln2 / 2, a degree-12 polynomial for
// exp(-r) (max. relative error 2e-17 of the polynomial, below 1 ulp with the rounding of the Horner steps), the scaling by one
// v_ldexp_f64 (which flushes through the subnormals to 0 by itself: no range checks).  17 fp64 operations, no comparison, no
// select (the library call carries four of each for arguments that cannot occur here).
__device__ __forceinline__ double exp_neg(const double a0) {
    // beyond 800 the result is 0 whatever the argument (+inf included: the reduction below would make inf - inf of it); a NaN
    // fails the comparison and stays a NaN, as numpy's exp leaves it (kernels.py:16-33)
    const double a = a0 > 800.0 ? 800.0 : a0;
    const double n = __builtin_rint(a * 1.4426950408889634074);          // a / ln 2
    double r = fma(n, -6.93147180369123816490e-01, a);                    // ln2 in two pieces: r = a - n ln2, exact product
    r = fma(n, -1.90821492927058770002e-10, r);
    const double x = -r;
    double p = 2.08767569878680989792e-09;                                // 1 / 12!
    p = fma(p, x, 2.50521083854417187751e-08);
    p = fma(p, x, 2.75573192239858906526e-07);
    p = fma(p, x, 2.75573192239858906526e-06);
    p = fma(p, x, 2.48015873015873015873e-05);
    p = fma(p, x, 1.98412698412698412698e-04);
    p = fma(p, x, 1.38888888888888888889e-03);
    p = fma(p, x, 8.33333333333333333333e-03);
    p = fma(p, x, 4.16666666666666666667e-02);
    p = fma(p, x, 1.66666666666666666667e-01);
    p = fma(p, x, 0.5);
    p = fma(p, x, 1.0);
    p = fma(p, x, 1.0);
    return __builtin_ldexp(p, -(int)n);
}

// sqrt(x) for x >= 0 from the hardware reciprocal square root: one coupled Newton (Goldschmidt) step on g ~ sqrt(x), h ~ 1 / (2 sqrt(x))
// and one correction of g (the library's sqrt rescales for subnormal arguments, classifies its input and corrects twice: squared
// scaled distances need none of it).  x is first raised to 1e-300, so the diagonal (x = 0) gives 1e-150, which every radial function
// here maps to the same bits as 0.
__device__ __forceinline__ double sqrt_pos(const double x0) {
    const double x = x0 < 1e-300 ? 1e-300 : x0;          // (not fmax: a NaN distance stays a NaN, kernels.py:461-481)
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    const double d = fma(-g, g, x);
    return fma(d, h, g);
}

template <int KIND>
__device__ __forceinline__ double radial(double r2, double sig) {
    if (KIND == 0) return sig * exp_neg(0.5 * r2);
    const double r = sqrt_pos(r2);
    if (KIND == 1) { const double a = SQRT3 * r; return sig * (1.0 + a) * exp_neg(a); }
    const double a = SQRT5 * r;
    return sig * fma(5.0 / 3.0, r2, 1.0 + a) * exp_neg(a);
}

// phi and the common factor cf such that dK/dl_k = cf * e2[k] * invl[k]  (e2 = D^2 / l^2), one exp and one square root per entry
// (kmat.hip: the gradient trace; grad_batch.hip: its batched twin)
template <int KIND>
__device__ __forceinline__ void radial_grad(const double r2, const double sig, double &phi, double &cf) {
    if (KIND == 0) { phi = exp_neg(0.5 * r2); cf = sig * phi; return; }
    const double r = sqrt_pos(r2);
    if (KIND == 1) { const double ea = exp_neg(SQRT3 * r); phi = fma(SQRT3, r, 1.0) * ea; cf = 3.0 * sig * ea; return; }
    const double ea = exp_neg(SQRT5 * r), t = fma(SQRT5, r, 1.0);
    phi = fma(5.0 / 3.0, r2, t) * ea; cf = (5.0 / 3.0) * sig * t * ea;
}

// radial_grad's phi and cf, and c2 = -(1 / r) dcf/dr such that d2K/dl_k dl_m = c2 e2[k] e2[m] invl[k] invl[m] - 3 delta_km cf e2[k] invl[k]^2
// (hessian.hip: the second-derivative trace), still one exp and one reciprocal square root per entry.  Matern 3/2's c2 carries 1 / r:
// at r2 = 0 it is 3 sqrt3 sig 1e150, finite, and every product it enters has an e2 factor that is exactly 0 there.
template <int KIND>
__device__ __forceinline__ void radial_hess(const double r2, const double sig, double &phi, double &cf, double &c2) {
    if (KIND == 0) { phi = exp_neg(0.5 * r2); cf = sig * phi; c2 = cf; return; }
    const double r = sqrt_pos(r2);
    if (KIND == 1) {
        // 1 / r from the reciprocal square root sqrt_pos starts from (the same instruction on the same argument), two Newton steps
        // against the corrected r
        double y = __builtin_amdgcn_rsq(r2 < 1e-300 ? 1e-300 : r2);
        y = fma(y, fma(-r, y, 1.0), y);
        y = fma(y, fma(-r, y, 1.0), y);
        const double ea = exp_neg(SQRT3 * r);
        phi = fma(SQRT3, r, 1.0) * ea; cf = 3.0 * sig * ea; c2 = SQRT3 * cf * y; return;
    }
    const double ea = exp_neg(SQRT5 * r), t = fma(SQRT5, r, 1.0);
    phi = fma(5.0 / 3.0, r2, t) * ea; cf = (5.0 / 3.0) * sig * t * ea; c2 = (25.0 / 3.0) * sig * ea;
}

}  // namespace
