"""Generate tests/golden/G12_posterior_grad_richardson.npz: ground truth for GP.posterior_gradients that does not depend on this
package.  Build-time only (needs the reference checkout, imported through the recipe of oracle/make_golden.py).

For RBF and Matern-5/2 (ARD) at the inputs of fixture G9 (N = 256, d = 2, the ten G9 prediction points) the REFERENCE's
posterior_mean and posterior_covariance(variance_only=True) are recorded at the points shifted by -2h, -h, +h, +2h along each input
direction.  The test forms the 4-point Richardson derivative
    f'(x) ~ [f(x - 2h) - 8 f(x - h) + 8 f(x + h) - f(x + 2h)] / (12 h)
whose error is  h^4 |f^(5)| / 30  (truncation)  +  (1 + 8 + 8 + 1) delta / (12 h) = 1.5 delta / h  (round-off, delta = the noise of one
recorded value).  Both terms are estimated here from the reference alone:
    F5     max |f^(5)| over points and directions, from a 6-point central fifth difference at the coarse step l_min / 8 (its own
           round-off, 16 delta / hc^5, is orders below F5);
    delta  three times the largest residual of a straight-line fit through f at eight points spaced 1e-9 apart (over that span the
           curvature contributes 1e-18 f'': what is left is the evaluation's rounding noise), not less than 7e-12 of the value's scale
           (the survey's figure for the reference's noise in m);
and h is where their sum is least, h^5 = 45 delta / (4 F5), rounded to two digits.  The
resulting bound  err = h^4 F5 / 30 + 1.5 delta / h  is stored beside the values (err_m, err_v: absolute).
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
SHIFTS = (-2.0, -1.0, 1.0, 2.0)


def main():
    warnings.simplefilter("ignore")
    from oracle.make_golden import import_reference
    fvgp = import_reference()
    from fvgp import kernels as rk

    def ref_rbf(x1, x2, h):
        return h[0] * rk.squared_exponential_kernel(rk.get_anisotropic_distance_matrix(x1, x2, h[1:]), 1.)

    def ref_m52(x1, x2, h):
        return h[0] * rk.matern_kernel_diff2(rk.get_anisotropic_distance_matrix(x1, x2, h[1:]), 1.)

    with np.load(os.path.join(OUT, "G9_derivatives_rbf_n256_d2.npz")) as z:
        x, y, nv, theta, xp = z["x"], z["y"], z["noise_variances"], z["theta"], z["x_pred"]
    D = x.shape[1]
    fx = {"x": x, "y": y, "noise_variances": nv, "theta": theta, "x_pred": xp, "shifts": np.array(SHIFTS),
          "kernels": np.array(["rbf_ard", "matern52_ard"])}
    for name, kern in (("rbf_ard", ref_rbf), ("matern52_ard", ref_m52)):
        gp = fvgp.GP(x, y, init_hyperparameters=theta, noise_variances=nv, kernel_function=kern)

        def f_m(q):
            return np.asarray(gp.posterior_mean(q)["m(x)"], dtype=np.float64).reshape(-1)

        def f_v(q):
            return np.asarray(gp.posterior_covariance(q, variance_only=True)["v(x)"], dtype=np.float64).reshape(-1)

        def shifted(k, s):
            q = np.array(xp)
            q[:, k] += s
            return q

        for tag, f, scale in (("m", f_m, float(np.max(np.abs(f_m(xp))))), ("v", f_v, float(theta[0]))):
            hc = float(np.min(theta[1:])) / 8.0
            F5 = 0.0
            delta = 7e-12 * scale
            t = np.arange(8.0)
            for k in range(D):
                c = {j: f(shifted(k, j * hc)) for j in (-3, -2, -1, 1, 2, 3)}
                F5 = max(F5, float(np.max(np.abs(c[3] - 4 * c[2] + 5 * c[1] - 5 * c[-1] + 4 * c[-2] - c[-3]) / (2.0 * hc ** 5))))
                line = np.stack([f(shifted(k, j * 1e-9)) for j in t])              # (8, P)
                coef = np.polyfit(t, line, 1)                                       # (2, P)
                res = line - (coef[0][None, :] * t[:, None] + coef[1][None, :])
                delta = max(delta, 3.0 * float(np.max(np.abs(res))))
            h = float(f"{(45.0 * delta / (4.0 * F5)) ** 0.2:.1e}")
            err = h ** 4 * F5 / 30.0 + 1.5 * delta / h
            vals = np.stack([np.stack([f(shifted(k, s * h)) for s in SHIFTS]) for k in range(D)])     # (D, 4, P)
            fx[f"{name}_{tag}_h"] = np.array(h)
            fx[f"{name}_{tag}_F5"] = np.array(F5)
            fx[f"{name}_{tag}_delta"] = np.array(delta)
            fx[f"{name}_{tag}_err"] = np.array(err)
            fx[f"{name}_{tag}_vals"] = vals
            fx[f"{name}_{tag}_0"] = f(xp)
            print(f"{name} {tag}: scale {scale:.3g} F5 {F5:.3e} delta {delta:.3e} h {h:.2e} err {err:.3e}")
    np.savez_compressed(os.path.join(OUT, "G12_posterior_grad_richardson.npz"), **fx)


if __name__ == "__main__":
    main()
