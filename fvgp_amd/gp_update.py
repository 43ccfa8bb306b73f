"""Removal of data points from a GP whose factor is resident on the device -- the other half of update_gp_data(append=True).

The reference can only replace the data (update_gp_data(append=False), fvgp/gp.py:689-779: a new K, a new O(n^3) factorisation), however
few points leave.  A sliding window of an autonomous experiment, dropping the outliers loo_predictions has found or thinning after
select_batch take out a handful.  With KV = L L^T, R the removed and S the kept indices,

    KV[S,S] = L[S,S] L[S,S]^T + L[S,R] L[S,R]^T

so the factor of the kept points is a positive rank-|R| update of the compacted triangle (fvgp_hip_chol_delete, csrc/chol_update.hip,
DESIGN 23): one read and one write of the part of the factor behind the first removed point per 16 removed points, no kernel evaluation,
nothing that can lose positive definiteness.  It needs only the resident factor, so it serves kernel callables and matrix-valued noise too.
"""
import numpy as np

from . import _lib

# remove_data takes the update route while the removed points are at most this fraction of the data (args["remove_update_max_fraction"]
# overrides it per GP) AND the cost model below expects it to be the faster route (args["remove_update_cost_model"] = False switches the
# model off); DESIGN 23 has the measurements behind both
REMOVE_UPDATE_MAX_FRACTION = 0.05

# wall times of update_gp_data(append=False) on one MI355X, ms (profiles/r16_remove_data.txt); between the sizes: log-log interpolation
_REFACTOR_MS = ((2000, 1.4), (8000, 6.2), (20000, 47.5), (50000, 590.0))


def refactor_ms(n):
    """what the refactor route costs at n points: the measured table, ~ n^3 above it; below it (not measured) half of the 1.4 ms at
    N = 2000 is taken to be the fixed cost of a call"""
    ns, ts = np.log([p[0] for p in _REFACTOR_MS]), np.log([p[1] for p in _REFACTOR_MS])
    x = np.log(max(int(n), 1))
    if x <= ns[0]:
        t0 = _REFACTOR_MS[0][1]
        return 0.5 * t0 * (1.0 + n / _REFACTOR_MS[0][0])
    if x >= ns[-1]:
        return float(np.exp(ts[-1] + 3.0 * (x - ns[-1])))
    return float(np.exp(np.interp(x, ns, ts)))


def update_ms(n, removed):
    """what the update route costs: per pass of 16 removed points a diagonal and a panel launch for every 128-column block behind the
    pass's first point ((0.062 + 0.0105 kp + 5e-8 kp n) ms a block, kp the pass's columns rounded up to 1, 2, 4, 8 or 16 -- the chain of
    diagonal steps is most of it), the compaction's two copies of the rows behind the first removed point at 2.5 TB/s, and the solve, log-determinant
    and uploads every removal pays (0.5 ms + 0.2 us a point)"""
    R = np.asarray(removed, dtype=np.int64)
    k, m = len(R), int(n) - len(R)
    ms = 0.5 + 0.0002 * n
    first = int(R[0])
    if first >= m:
        return ms
    ms += 32.0 * (m * m - first * first) / 2 / 2.5e9
    for p0 in range(0, k, _lib.CHOL_UPDATE_MAX_RANK):
        kp = min(_lib.CHOL_UPDATE_MAX_RANK, k - p0)
        bucket = next(b for b in (1, 2, 4, 8, 16) if b >= kp)
        row0 = int(R[p0]) - p0
        if row0 < m:
            ms += (-(-m // 128) - row0 // 128) * (0.062 + 0.0105 * bucket + 5e-8 * bucket * m)
    return ms


def removal_indices(indices, n):
    """sorted unique int64 indices from an integer array or a boolean mask of length n; raises before anything is touched"""
    idx = np.asarray(indices)
    if idx.dtype == bool:
        if idx.shape != (n,):
            raise ValueError(f"remove_data: a boolean mask must have length {n}, got shape {idx.shape}")
        return np.flatnonzero(idx).astype(np.int64)
    if idx.size == 0:
        return np.zeros(0, dtype=np.int64)
    if not np.issubdtype(idx.dtype, np.integer):
        raise TypeError("remove_data: indices must be an integer array or a boolean mask")
    idx = np.unique(idx.astype(np.int64).ravel())
    if idx[0] < 0 or idx[-1] >= n:
        raise IndexError(f"remove_data: indices must lie in 0 .. {n - 1}")
    return idx


class UpdateMixin:
    """Mixed into fvgp_amd.GP: needs _set_data, set_hyperparameters, _mean, _noise, _refresh_inverse, _eval_dim and the state fields."""

    def remove_data(self, indices):
        """Take the points `indices` (rows of x_data: an integer array, duplicates collapsed, or a boolean mask of length n) out of the GP.
        Afterwards the object is in the state update_gp_data(x_kept, y_kept, noise_variances_kept, append=False) would leave.

        Returns {"removed": the sorted unique indices, "kept": the kept indices, "route": "update" | "refactor" (None: nothing to remove)}.
        "update": the resident factor is updated in place (fvgp_hip_chol_delete) and KVinvY, log|KV| and the log-likelihood are
        recomputed from it, as after an append.  It is taken when the factor is on this device (not row-sharded, no linalg_mode
        callables), the removed points are at most args["remove_update_max_fraction"] of the data (default 0.05) and the measured cost
        model expects the update to be the faster route (update_ms / refactor_ms in this module: the update pays per 128-column block
        behind the first removed point, so the newest points leave almost for free at every size and the oldest ones only from
        N ~ 20 000 on; args["remove_update_cost_model"] = False leaves the fraction alone to decide), and the noise of the kept points is
        the same before and after -- given noise_variances and noise functions of x qualify; the DEFAULT noise rule is
        (mean|y| / 100)^2, changes with the data and so normally takes the "refactor" route: _set_data + set_hyperparameters, what
        update_gp_data(append=False) runs.  An index out of range or a set that keeps no point raises before anything is touched; a
        device failure after the factor was modified rebuilds the state of the OLD data by the refactor route and re-raises."""
        n = self.point_number
        R = removal_indices(indices, n)
        keep = np.ones(n, dtype=bool)
        keep[R] = False
        S = np.flatnonzero(keep)
        if len(S) == 0:
            raise ValueError("remove_data: at least one data point must remain")
        out = {"removed": R, "kept": S, "route": None}
        if len(R) == 0:
            return out
        x = np.ascontiguousarray(self.x_data[S])
        y = np.ascontiguousarray(self.y_data[S])
        nv = None if self.noise_variances is None else np.ascontiguousarray(self.noise_variances[S])
        V_new = self._removal_noise(x, y, nv, R, S)
        if V_new is None:
            self._set_data(x, y, nv)
            self.set_hyperparameters(self._hps)
            out["route"] = "refactor"
        else:
            self._remove_factor(R, x, y, nv, V_new)
            out["route"] = "update"
        return out

    def _removal_noise(self, x, y, nv, R, S):
        """the noise of the kept points when the update route may run, else None"""
        if self._sharded or self._linalg_callables is not None:
            return None
        if len(R) > float(self.args.get("remove_update_max_fraction", REMOVE_UPDATE_MAX_FRACTION)) * self.point_number:
            return None
        if self.args.get("remove_update_cost_model", True) and update_ms(self.point_number, R) > refactor_ms(len(S)):
            return None
        old = (self.x_data, self.y_data, self.noise_variances)
        try:                                  # the noise rule reads the object's data (default rule: mean|y|; given variances: their length)
            self.x_data, self.y_data, self.noise_variances = x, y, nv
            V_new = self._noise(x, self._hps)
        finally:
            self.x_data, self.y_data, self.noise_variances = old
        V_old = self.V[S] if np.ndim(self.V) == 1 else self.V[np.ix_(S, S)]
        return V_new if np.array_equal(V_new, V_old) else None

    def _remove_factor(self, R, x, y, nv, V_new):
        H, hps, n = self._H, self._hps, self.point_number
        m, ncol = len(x), y.shape[1]
        np_new = _lib.pad128(m)
        names = ("x_data", "y_data", "noise_variances", "point_number", "_np", "_x_dev", "_alpha", "m", "V", "_loglik", "_logdet", "_K_host")
        old = {k: self.__dict__[k] for k in names}
        touched = False
        try:
            # everything that can fail without the factor: the workspace, the uploads, the mean of the kept data
            work = H.empty(max(1, _lib.chol_update_workspace_bytes(n, len(R))) // 8)
            self.x_data, self.y_data, self.noise_variances, self.point_number, self._np = x, y, nv, m, np_new
            mean = self._mean(x, hps)
            ymean = y - mean[:, None]
            ym_dev = H.to_device(ymean)
            x_dev = H.to_device(x)
            alpha = H.zeros(np_new, ncol)
            alpha[:m] = ym_dev
            touched = True
            H.chol_delete(self._L, n, R, work)
            H.invalidate_factor()                                 # the factor changed under the handle's cached block inverses
            self._x_dev, self._alpha = x_dev, alpha
            if ncol <= _lib.MAX_RHS_VEC:
                H.potrs(self._L, m, alpha, ncol)
            else:
                rhs = H.zeros(np_new, _lib.pad128(ncol))
                rhs[:m, :ncol] = alpha[:m]
                H.potrs(self._L, m, rhs, _lib.pad128(ncol))
                alpha[:m] = rhs[:m, :ncol]
            self._logdet = H.logdet(self._L, m)
            quad = H.dot(ym_dev, alpha, m) / ncol
            self._loglik = -0.5 * (quad + self._logdet + m * np.log(2.0 * np.pi))
            self.m, self.V = mean, V_new
            self._K_host = None
            if self._native is not None:
                H.posterior_prepare(self._L, m)                   # as set_hyperparameters leaves a new state
            if not (self._work is not None and self._work.shape[0] == self._eval_dim() and self._alpha_work.shape[0] == np_new):
                self._work = self._work2 = self._work3 = self._alpha_work = None
            self._refresh_inverse()
        except BaseException:
            self.__dict__.update(old)
            if touched:
                # the old factor is gone and cannot be copied back: the state of the OLD data by the refactor route
                H.invalidate_factor()
                self._set_data(old["x_data"], old["y_data"], old["noise_variances"])
                self.set_hyperparameters(hps)
            raise
