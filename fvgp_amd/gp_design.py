"""Greedy batch selection of measurement points: given P candidate positions, which q to measure next.

The rule picks the candidate with the largest conditional variance (or the largest information gain), conditions every other
candidate on it, and repeats -- the pivoted Cholesky factorisation of the candidates' posterior covariance, the greedy maximiser of the
joint entropy of the batch and of its mutual information with f (Nemhauser, Wolsey & Fisher 1978: within 1 - 1/e of the best batch).
With j the pick, d the conditional latent variances and s the candidates' noise variances,

    r_i = k(x_i, x_j) - sum_n k(x_i, X_n) w_n,   w = KV^-1 k(X, x_j)                        (column j of the posterior covariance)
    c_i = (r_i - sum_{s<t} G[s,i] G[s,j]) / sqrt(d_j + s_j),      d_i <- max(d_i - c_i^2, 0)

costs two vector sweeps over the factor the GP already holds and one matrix-free pass over the candidates (fvgp_hip_select_batch,
csrc/select.hip): O(P q) memory, no P x P array on the device or the host for any P, nothing that depends on y.  The reference has no
counterpart; its route is posterior_covariance(x)["S_flat"] and a pivoted Cholesky on the host, which forms P x P.
"""
import warnings

import numpy as np

from . import _lib

CRITERIA = {"variance": 0, "information": 1}
_HOST_ROUTE = "the host route is posterior_covariance(x_candidates)['S_flat'] and a pivoted Cholesky of it"


class DesignMixin:
    """Mixed into fvgp_amd.GP: needs _H, _L, _alpha, _x_dev, _native, _hps, _noise, _np, _posterior_chunk, cartesian_product."""

    def _design_refusals(self):
        if self._sharded:
            raise NotImplementedError("select_batch sweeps the factor on one device; the row-sharded mode (args['process_group']) has "
                                      "no batch selection: " + _HOST_ROUTE)
        if self._native is None:
            raise NotImplementedError("select_batch evaluates the kernel on the device: a kernel callable has no batch selection "
                                      "(use one of the named kernels); " + _HOST_ROUTE)
        if self._linalg_callables is not None:
            raise NotImplementedError("select_batch needs the Cholesky factor on this device: linalg_mode callables keep their own "
                                      "factorisation object on the host; " + _HOST_ROUTE)

    def _design_variances(self, xc_dev, P):
        """the candidates' latent posterior variances on the device, chunk by chunk through one chunk scratch (no P x P array)"""
        H, n = self._H, self.point_number
        C = int(self._posterior_chunk)
        assert C % 128 == 0 and C >= 128, "posterior_chunk must be a multiple of 128"
        var = H.empty(P)
        kx = H.empty(self._np, _lib.pad128(min(P, C)))
        for a in range(0, P, C):
            b = min(a + C, P)
            Pp = _lib.pad128(b - a)
            H.posterior(self._native.kernel_id, self._x_dev, self._hps, self._L, self._alpha, self.y_data.shape[1], xc_dev[a:b],
                        kx.view(-1)[:self._np * Pp].view(self._np, Pp), var_out=var[a:b])
        return var

    def select_batch(self, x_candidates, n_select, x_out=None, criterion="variance", noise_variances=None, allow_repeats=False,
                     tol=1e-12):
        """The greedy batch of at most n_select of the candidates, at the current hyperparameters.

        x_candidates (P, D); with x_out (fvGP) the candidates are cartesian_product(x_candidates, x_out) as in posterior_covariance, and
        the indices refer to that product (returned as "x_pred").  criterion "variance": the largest conditional latent variance;
        "information": the largest gain 1/2 log(1 + v / noise) (every candidate's noise must be > 0).  noise_variances: None takes the
        model's noise at the candidates (as add_noise=True does), a scalar or a (P,) array overrides it.  allow_repeats: a candidate
        may be picked again (a repeat measurement of a noisy point).  The batch ends early ("exhausted") once the best candidate's
        variance is at most tol times the largest initial one, or no candidate is left.

        Returns a dict; m <= n_select picks were made: "indices" (m,), "x" (m, D') the picked rows of "x_pred", "v_before" (P,) the
        latent posterior variances, "v_after" (P,) those every candidate would have after the batch is measured, "v_selected" (m,) the
        conditional latent variance of each pick when it was made, "noise_selected" (m,), "information_gain" (m,) the cumulative
        1/2 sum log(1 + v_selected / noise_selected) (None if a picked noise is 0), "exhausted".  The GP's state and cached results
        are untouched."""
        self._design_refusals()
        assert isinstance(n_select, (int, np.integer)) and n_select >= 1, "n_select must be a positive integer"
        if criterion not in CRITERIA:
            raise ValueError(f"criterion must be one of {sorted(CRITERIA)}, got {criterion!r}")
        if not (np.isfinite(tol) and tol >= 0.0):
            raise ValueError("tol must be a finite number >= 0")
        if x_out is None:
            x_out = self.x_out
        self._perform_input_checks(x_candidates, x_out)
        x_pred = x_candidates
        if isinstance(x_out, np.ndarray):
            x_pred = self.cartesian_product(x_candidates, x_out)
        assert x_pred.shape[1] == self.index_set_dim, "wrong number of columns in x_candidates"
        x_pred = np.ascontiguousarray(x_pred, dtype=np.float64)
        P, q = len(x_pred), int(n_select)
        assert P >= 1, "no candidates"
        if noise_variances is None:
            noise = np.asarray(self._noise(x_pred, self._hps), dtype=np.float64)
            if noise.ndim == 2:
                raise NotImplementedError("select_batch conditions on one candidate at a time: a matrix-valued noise model has no "
                                          "batch selection; pass noise_variances as a scalar or a (P,) array")
        else:
            noise = np.asarray(noise_variances, dtype=np.float64)
            if noise.ndim == 0:
                noise = np.full(P, float(noise))
        if noise.shape != (P,):
            raise ValueError(f"noise_variances must be a scalar or of shape ({P},), got {noise.shape}")
        if np.any(~(noise >= 0.0)):
            raise ValueError("noise variances must be >= 0")
        if criterion == "information" and np.any(noise <= 0.0):
            raise ValueError("criterion 'information' ranks by v / noise: every candidate's noise variance must be > 0")
        noise = np.ascontiguousarray(noise)

        H, torch = self._H, self._H.torch
        xc = H.to_device(x_pred)
        var = self._design_variances(xc, P)
        v_raw = var.cpu().numpy()
        if np.any(v_raw < -0.0001):
            warnings.warn("Negative variances encountered. That normally means that the model is unstable. "
                          "Rethink the kernel definition, add more noise to the data, "
                          "or double check the hyperparameter optimization bounds. This will not "
                          "terminate the algorithm, but expect anomalies.")
        idx = torch.empty(q, dtype=torch.int64, device=var.device)
        pick = H.empty(q)
        H.select_batch(self._native.kernel_id, self._x_dev, self._hps, self._L, xc, var, q, idx, pick,
                       noise=H.to_device(noise) if np.any(noise > 0.0) else None, criterion=CRITERIA[criterion],
                       allow_repeats=allow_repeats, tol=float(tol))
        H.sync()
        idx_h = idx.cpu().numpy()
        m = int(np.argmax(idx_h < 0)) if np.any(idx_h < 0) else q
        indices = idx_h[:m].copy()
        v_sel, n_sel = pick.cpu().numpy()[:m].copy(), noise[indices]
        gain = 0.5 * np.cumsum(np.log1p(v_sel / n_sel)) if np.all(n_sel > 0.0) else None
        exhausted = m < q
        if exhausted:
            warnings.warn(f"select_batch stopped after {m} of {q} picks: no candidate is left whose conditional variance exceeds "
                          f"tol = {tol:g} times the largest initial variance.")
        return {"indices": indices, "x": x_pred[indices], "x_pred": x_pred, "v_before": np.maximum(v_raw, 0.0),
                "v_after": var.cpu().numpy(), "v_selected": v_sel, "noise_selected": n_sel, "information_gain": gain,
                "exhausted": exhausted}
