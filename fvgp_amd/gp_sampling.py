"""Joint draws from the posterior and the prior, on the device.

Thompson sampling, Monte-Carlo acquisition functions (q-EI, entropy search) and a plot of plausible functions need JOINT samples
f ~ N(m(x*), S(x*)).  With the reference a user pulls the P x P covariance of posterior_covariance (gp_posterior.py:229-288) to the host,
adds a jitter, runs numpy.linalg.cholesky and multiplies host-generated normals.  Here S stays where the posterior path formed it:

    S + jitter I  --fvgp_hip_potrf-->  L        samples = m + (L Z)^T        Z[p][s] = z(seed, stream, p, s)

with z the library's counter-based normal (include/fvgp_hip.h "sampling"; tests/samples_ref.py is its numpy twin): the same arguments give
the same bits on every run, sample s is the same whether it is drawn alone or among others, and `stream` gives independent draws under one
seed.  The jitter is the reference's own 1e-9 I (gp_kl_div adds it before its factorisations).  The GP's state is never touched: the
factorisation runs on the square the covariance was formed in.
"""
import numpy as np

from . import _lib


class SamplingMixin:
    """Mixed into fvgp_amd.GP: needs _posterior_device, _mean, _noise, _native, _host_kernel, _hps, _L, _alpha, cartesian_product."""

    def _sampling_handle(self):
        if self._H is not None:
            return self._H
        H = getattr(self._sh.ops, "H", None) if self._sh is not None else None
        if H is None:
            raise NotImplementedError("sampling factors the covariance on this rank's device: the row-sharded GP needs its HIP ops")
        return H

    def _sampling_points(self, x_pred, x_out, n_samples):
        assert isinstance(n_samples, (int, np.integer)) and n_samples >= 1, "n_samples must be a positive integer"
        if self.y_data.shape[1] != 1:
            raise NotImplementedError("joint samples are drawn for one output column; a multi-task model is an fvGP (x_out)")
        if x_out is None:
            x_out = self.x_out
        self._perform_input_checks(x_pred, x_out)
        x_orig = x_pred.copy()
        if isinstance(x_out, np.ndarray):
            x_pred = self.cartesian_product(x_pred, x_out)
        assert x_pred.shape[1] == self.index_set_dim, "wrong number of columns in x_pred"
        return x_orig, x_pred, x_out

    def _draw(self, H, mean, S, noise, n_samples, seed, stream, jitter, return_normals, x_orig, x_pred, x_out):
        """samples from N(mean, S + noise + jitter I): S a host (P, P) array or the padded device square the posterior path left (it is
        factored in place), noise None, a P-vector or a (P, P) host array"""
        P = len(mean)
        Pp = _lib.pad128(P)
        if isinstance(S, np.ndarray):
            A = H.empty(Pp, Pp)
            A[:P, :P] = H.to_device(S)
        else:
            A = S
        diag = A.diagonal()[:P]
        diag.clamp_(min=0.0)                               # posterior_covariance's clipping of negative variances (gp_posterior.py:248-259)
        if noise is not None:
            if np.ndim(noise) == 2:
                A[:P, :P] += H.to_device(noise)
            else:
                diag += H.to_device(noise)
        diag += float(jitter)
        info = H.potrf(A, P)
        H.invalidate_factor()                              # A is a temporary: its address may come back as somebody's factor
        if info != 0:
            raise Exception(f"The covariance at the {P} prediction points is not positive definite with jitter = {jitter:g}: dpotrf "
                            f"info = {info} (the leading minor of that order). Pass a larger `jitter`.")
        Y = H.empty(n_samples, P)
        Z = H.empty(P, n_samples) if return_normals else None
        H.mvn_sample(A, P, Y, mean=H.to_device(mean), seed=seed, stream=stream, Z_out=Z)
        H.sync()
        samples = H.to_host(Y)
        out = {"x": x_orig, "x_pred": x_pred, "samples": samples, "m(x)_flat": mean, "jitter": float(jitter)}
        if isinstance(x_out, np.ndarray):                  # ordered as m(x): (points, tasks) of the task-major flat vector
            out["samples(x)"] = samples.reshape(n_samples, len(x_out), len(x_orig)).transpose(0, 2, 1)
        if return_normals:
            out["normals"] = H.to_host(Z)
        return out

    def posterior_samples(self, x_pred, n_samples=1, x_out=None, add_noise=False, seed=0, stream=0, jitter=1e-9, return_normals=False):
        """n_samples joint draws f ~ N(m(x_pred), S(x_pred) + jitter I) from the posterior at the current hyperparameters, with m and S
        as posterior_mean and posterior_covariance(add_noise=...) return them, for every mode those serve.  Returns "x", "x_pred",
        "samples" (n_samples, P) over the flat prediction points, "samples(x)" (n_samples, len(x_pred), len(x_out)) with x_out,
        "m(x)_flat", "jitter" and, with return_normals, "normals" (P, n_samples): samples - m(x)_flat = (chol(S + jitter I) normals)^T.
        Draw s depends on (seed, stream, s) and the GP only: a longer call extends a shorter one, another `stream` or `seed` gives
        independent draws.  A covariance that is not positive definite with this jitter raises (no retry with another one: the same
        call always returns the same bits)."""
        x_orig, x_pred, x_out = self._sampling_points(x_pred, x_out, n_samples)
        H = self._sampling_handle()
        hps = self._hps
        A, S = self._posterior_device(x_pred, hps, None if self._sharded else self._L, None if self._sharded else self._alpha,
                                      want_cov=True, keep_device=True)
        mean = self._mean(x_pred, hps) + np.asarray(A)[:, 0]
        noise = self._noise(x_pred, hps) if add_noise else None          # gp_posterior.py:554-569
        return self._draw(H, mean, S, noise, int(n_samples), seed, stream, jitter, return_normals, x_orig, x_pred, x_out)

    def prior_samples(self, x, n_samples=1, x_out=None, seed=0, stream=0, jitter=1e-9, return_normals=False):
        """n_samples joint draws f ~ N(m(x), k(x, x) + jitter I) from the prior at the current hyperparameters; the dictionary of
        posterior_samples with the prior mean as "m(x)_flat".  Smooth kernels at many points need a larger jitter than 1e-9."""
        x_orig, x_pred, x_out = self._sampling_points(x, x_out, n_samples)
        H = self._sampling_handle()
        hps = self._hps
        if self._native is not None:
            P = len(x_pred)
            xp = H.to_device(x_pred)
            S = H.empty(_lib.pad128(P), _lib.pad128(P))
            H.kmat(self._native.kernel_id, xp, xp, hps, S, pad=_lib.PAD_ZERO)
        else:
            S = self._host_kernel(x_pred, x_pred, hps)
        return self._draw(H, self._mean(x_pred, hps), S, None, int(n_samples), seed, stream, jitter, return_normals, x_orig, x_pred, x_out)
