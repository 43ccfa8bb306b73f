"""Leave-one-out cross-validation on the training data, in closed form (Rasmussen & Williams 5.4.2).

The validation scores of gp_validation.py need held-out points; an autonomous experiment has none to spare.  For a GP all n
leave-one-out predictions follow from KV^-1 (POTRI) and KVinvY, which the gradient path computes anyway:

    y_i - mu_i = alpha_i / q_i,   sigma^2_i = 1 / q_i,   L_LOO = sum_i log p(y_i | y_-i),      q = diag(KV^-1), alpha = KV^-1 (y - m)

and L_LOO -- the training objective of choice when the kernel family is misspecified -- has an exact gradient that costs one
symmetric N^3 product for all hyperparameters together (fvgp_hip_loo, csrc/loo.hip).  One factorisation per call, on the scratch
buffers: the GP's state is never touched.  The reference has no counterpart; `GP(..., args={"training_objective": "loo"})` makes
`train` optimise it.
"""
import numpy as np

from . import _lib


def assemble_loo_gradient(g_kernel, u, alpha, mdiag, dV=None, dm=None):
    """dL_LOO/dtheta from the device's pieces: g_kernel (H,) the kernel term (0 where the kernel owns nothing), u = Q w,
    alpha = KVinvY[:, component] and mdiag = diag(Q diag(c) Q), n-vectors; dV (H, n) the derivative of the noise variances or None;
    dm (H, n) the derivative of the prior mean or None:

        dL/dtheta_j = g_kernel_j + sum_k dV_jk (u_k alpha_k - M_kk) + u^T dm_j

    Every term counts (the marginal likelihood's rule of dropping the kernel term beside a mean term is the reference's and belongs
    to its objective only)."""
    g = np.array(g_kernel, dtype=np.float64)
    if dV is not None:
        dV = np.asarray(dV, dtype=np.float64)
        if dV.ndim != 2:
            raise NotImplementedError("the LOO gradient takes a diagonal noise derivative (H, n); for a matrix-valued noise model use "
                                      "a gradient-free method ('mcmc', 'global') on loo_log_predictive")
        g = g + dV @ (np.asarray(u) * np.asarray(alpha) - np.asarray(mdiag))
    if dm is not None:
        g = g + np.asarray(dm, dtype=np.float64) @ np.asarray(u)
    return g


class LOOMixin:
    """Mixed into fvgp_amd.GP: needs _evaluate, _scratch, _H, _native, _hps, y_data, _noise_grad, _mean_grad."""

    def _loo_device(self, hyperparameters, component, want_grad):
        if self._sharded:
            raise NotImplementedError("leave-one-out cross-validation needs KV^-1 on one device; the row-sharded mode has no LOO path "
                                      "(build the GP without args['process_group'], or score it with held-out data: rmse, nlpd, crps)")
        if want_grad and self._native is None:
            raise NotImplementedError("the LOO gradient re-evaluates dK/dtheta on the device: use one of the named kernels, or a "
                                      "gradient-free method ('mcmc', 'global') on loo_log_predictive with a kernel callable")
        H, n = self._H, self.point_number
        hps = self._hps if hyperparameters is None else np.asarray(hyperparameters, dtype=np.float64)
        KV, aw = self._scratch()
        if self._work2 is None:
            self._work2 = H.empty(self._np, self._np)
        try:
            _, _, m, V = self._evaluate(hps, KV, aw, use_callables=False)
        except Exception as e:
            raise Exception(f"Linear algebra failed for hyperparameters {hps}: {e}") from e
        ws = H.empty(max(1, _lib.loo_workspace_bytes(n) // 8))
        resid, var = H.empty(n), H.empty(n)
        u = H.empty(n) if want_grad else None
        mdiag = H.empty(n) if want_grad else None
        ncol = self.y_data.shape[1]
        out, g = H.loo(self._native.kernel_id if want_grad else None, self._x_dev if want_grad else None, hps if want_grad else None,
                       aw, ncol, component, KV, self._work2, ws, resid, var, u, mdiag, n=n)
        if out[3] != 0:
            raise Exception(f"Linear algebra failed for hyperparameters {hps}: {int(out[3])} diagonal entries of KV^-1 are not "
                            "positive and finite")
        return out, g, resid, var, u, mdiag, aw, V, hps

    def loo_predictions(self, hyperparameters=None, component=0):
        """All n leave-one-out predictions at `hyperparameters` (None: the current ones) from one factorisation:
        "m_loo" / "v_loo" the predictive mean and variance of the noisy observation y_i given every other point, "v_loo_latent" the
        variance without point i's own noise (vector noise models; None otherwise), "log_predictive" the n terms log p(y_i | y_-i),
        "loo_log_predictive" their sum, "rmse" and "nlpd" (= -loo_log_predictive / n) over the n held-out points."""
        out, _, resid, var, _, _, _, V, _ = self._loo_device(hyperparameters, component, False)
        n = self.point_number
        r, v = resid.cpu().numpy(), var.cpu().numpy()
        return {"m_loo": self.y_data[:, component] - r, "v_loo": v,
                "v_loo_latent": v - np.asarray(V) if np.ndim(V) == 1 else None,
                "log_predictive": -0.5 * np.log(2.0 * np.pi * v) - 0.5 * r * r / v,
                "loo_log_predictive": float(out[0]), "rmse": float(np.sqrt(out[1] / n)), "nlpd": float(-out[0] / n)}

    def loo_log_predictive(self, hyperparameters=None, component=0):
        """sum_i log p(y_i | y_-i, theta): the leave-one-out log predictive probability (to be maximised)"""
        return float(self._loo_device(hyperparameters, component, False)[0][0])

    def neg_loo_log_predictive(self, hyperparameters=None, component=0):
        return -self.loo_log_predictive(hyperparameters, component)

    def neg_loo_log_predictive_and_gradient(self, hyperparameters=None, component=0):
        """(-L_LOO, -dL_LOO/dtheta) from ONE factorisation; kernel, diagonal-noise and mean hyperparameters all carry their exact term"""
        out, g, _, _, u, mdiag, aw, _, hps = self._loo_device(hyperparameters, component, True)
        n = self.point_number
        dV = self._noise_grad(hps) if self._noise_callable is not None else None
        dm = self._mean_grad(hps) if self._mean_callable is not None else None
        if dV is not None or dm is not None:
            g = assemble_loo_gradient(g, u.cpu().numpy(), aw[:n, component].cpu().numpy(), mdiag.cpu().numpy(), dV, dm)
        return -float(out[0]), -np.asarray(g, dtype=np.float64)

    def neg_loo_log_predictive_gradient(self, hyperparameters=None, component=0):
        return self.neg_loo_log_predictive_and_gradient(hyperparameters, component)[1]
