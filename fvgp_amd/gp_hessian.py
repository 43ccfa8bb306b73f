"""The exact Hessian of the negative log marginal likelihood, and what it is for at a trained theta.

`GP.neg_log_likelihood_hessian` is the reference's forward difference of the gradient: H + 1 factorisations for four to six digits.
`GP.neg_log_likelihood_exact_hessian` evaluates the closed form on the device in one call (fvgp_hip_loglik_hess, csrc/hessian.hip):

    H_ij = 1/2 sum_ab (W - b b^T)_ab (d2K/dtheta_i dtheta_j)_ab - [ 1/2 tr(G_i K_j) - b^T K_j w_i ],   W = KV^-1, b = W (y - m),
                                                                                                        G_i = W K_i W, w_i = W K_i b

for the hyperparameters the named kernel owns.  On top of it: the Laplace approximation N(theta, H^-1) of the hyperparameter posterior
with its evidence (`GP.hyperparameter_laplace`, samples ready for `posterior_mixture`), and Newton-type local training
(`GP(..., args={"exact_hessian": True})` hands the Hessian to scipy).  One factorisation per call, on the scratch buffers: the GP's
state is never touched.
"""
import numpy as np

from . import _lib


def laplace_from_hessian(theta, neg_log_likelihood, hessian, n_samples=0, seed=0, bounds=None, max_tries=64):
    """The Laplace approximation of the hyperparameter posterior under a flat prior from (theta, f = -log p(y|theta), H = f''): a
    dictionary with "mean" (theta), "hessian", "covariance" (H^-1), "log_evidence" = -f + (H/2) log 2 pi - 1/2 log|H| and "samples",
    (n_samples, H) draws from N(theta, H^-1).  A draw outside `bounds` ((H, 2), default every component > 0) is drawn again, at most
    `max_tries` times.  Raises ValueError where H is not positive definite: theta is then no minimum."""
    theta = np.asarray(theta, dtype=np.float64)
    H = np.asarray(hessian, dtype=np.float64)
    nh = len(theta)
    if H.shape != (nh, nh):
        raise ValueError(f"the Hessian must be ({nh}, {nh}), got {H.shape}")
    H = 0.5 * (H + H.T)
    lam = np.linalg.eigvalsh(H)
    if not np.all(np.isfinite(lam)) or lam[0] <= 0.0:
        raise ValueError(f"the Hessian is not positive definite (smallest eigenvalue {lam[0]:.6g}): "
                         "θ is not at a minimum of the negative log-likelihood")
    L = np.linalg.cholesky(H)                                  # H = L L^T
    Linv = np.linalg.solve(L, np.eye(nh))
    cov = Linv.T @ Linv
    cov = 0.5 * (cov + cov.T)
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
    log_evidence = -float(neg_log_likelihood) + 0.5 * nh * np.log(2.0 * np.pi) - 0.5 * logdet
    n_samples = int(n_samples)
    if bounds is None:
        lo, hi, lo_open = np.zeros(nh), np.full(nh, np.inf), True
    else:
        b = np.asarray(bounds, dtype=np.float64)
        if b.shape != (nh, 2):
            raise ValueError(f"bounds must be ({nh}, 2), got {b.shape}")
        lo, hi, lo_open = b[:, 0], b[:, 1], False
    rng = np.random.default_rng(seed)
    samples = np.empty((n_samples, nh))
    todo = np.arange(n_samples)
    for _ in range(int(max_tries)):
        if len(todo) == 0:
            break
        z = rng.standard_normal((len(todo), nh))
        samples[todo] = theta + z @ Linv                       # x = theta + L^-T z: covariance L^-T L^-1 = H^-1
        s = samples[todo]
        ok = np.all((s > lo) if lo_open else (s >= lo), axis=1) & np.all(s <= hi, axis=1)
        todo = todo[~ok]
    if len(todo):
        raise RuntimeError(f"{len(todo)} of {n_samples} Laplace samples were still outside the bounds after {max_tries} draws each: "
                           "the approximation puts most of its mass outside (pass wider bounds, or check theta)")
    return {"mean": theta.copy(), "hessian": H, "covariance": cov, "log_evidence": float(log_evidence), "samples": samples}


class HessianMixin:
    """Mixed into fvgp_amd.GP: needs _evaluate, _scratch, _H, _native, _hps, y_data, _work2, neg_log_likelihood."""

    _FD_ROUTE = "use neg_log_likelihood_hessian (the finite-difference route)"

    def _check_exact_hessian(self, hps):
        if self._sharded:
            raise NotImplementedError("the exact Hessian needs KV^-1 and two more N x N buffers on one device; for a row-sharded GP "
                                      + self._FD_ROUTE)
        if self._native is None:
            raise NotImplementedError("the exact Hessian re-evaluates the kernel's second derivatives on the device; with a kernel "
                                      "callable " + self._FD_ROUTE)
        if self._linalg_callables is not None:
            raise NotImplementedError("the exact Hessian runs on the device's own factorisation; with linalg_mode callables "
                                      + self._FD_ROUTE)
        nk = self._native.n_hyperparameters(self.index_set_dim)
        if len(hps) != nk:
            raise NotImplementedError(f"the exact Hessian covers the {nk} hyperparameters the kernel owns, this GP has {len(hps)} (noise "
                                      "or mean callables own the rest: their second derivatives are not available); " + self._FD_ROUTE)

    def neg_log_likelihood_exact_hessian(self, hyperparameters=None, component=0, return_gradient=False):
        """The exact (H, H) Hessian of neg_log_likelihood at `hyperparameters` (None: the current ones) from one factorisation and
        one device call: the average of the device's raw block and its transpose (H_ij and H_ji are computed independently there), so
        symmetric to the bit.  return_gradient: (hessian, gradient), the gradient of neg_log_likelihood_gradient from the same call.
        Named kernels without noise- or mean-owned hyperparameters, one device; otherwise NotImplementedError."""
        hps = self._hps if hyperparameters is None else np.asarray(hyperparameters, dtype=np.float64)
        self._check_exact_hessian(hps)
        H, n = self._H, self.point_number
        KV, aw = self._scratch()
        if self._work2 is None:
            self._work2 = H.empty(self._np, self._np)
        if self._work3 is None:
            self._work3 = H.empty(self._np, self._np)
        try:
            self._evaluate(hps, KV, aw, use_callables=False)
        except Exception as e:
            raise Exception(f"Linear algebra failed for hyperparameters {hps}: {e}") from e
        ws = H.empty(max(1, _lib.loglik_hess_workspace_bytes(n, self.index_set_dim) // 8))
        g, raw = H.loglik_hess(self._native.kernel_id, self._x_dev, hps, aw, self.y_data.shape[1], component, KV, self._work2,
                               self._work3, ws)
        hess = 0.5 * (raw + raw.T)
        return (hess, g) if return_gradient else hess

    def hyperparameter_laplace(self, hyperparameters=None, n_samples=0, seed=0, bounds=None):
        """The Laplace approximation N(theta, H^-1) of the hyperparameter posterior at `hyperparameters` (None: the current, trained
        ones) under a flat prior: "mean", "hessian" (exact), "covariance", "log_evidence" = log p(y|theta) + (H/2) log 2 pi -
        1/2 log|H| (for comparing kernels) and "samples" (n_samples, H), inside `bounds` (default: every component > 0) and ready for
        posterior_mixture(x_pred, samples).  Raises ValueError where the Hessian is not positive definite."""
        hps = self._hps if hyperparameters is None else np.asarray(hyperparameters, dtype=np.float64)
        hess = self.neg_log_likelihood_exact_hessian(hps)
        f = self.neg_log_likelihood(hps)
        return laplace_from_hessian(hps, f, hess, n_samples=n_samples, seed=seed, bounds=bounds)
