"""Prediction with ALL the data at sizes where no N x N factor fits: (K(theta) + V) X = B by preconditioned conjugate gradients.

K is never stored.  Every product with K evaluates the kernel on the fly (fvgp_hip_kmatvec), the preconditioner is the rank-q
pivoted Cholesky G^T G + V of K + V applied through Woodbury (fvgp_hip_pchol, fvgp_hip_precond_factor), the recurrences' scalars live
on the device (fvgp_hip_pcg).  Memory is O(N (q + 16)): N = 10^6 at rank 256 holds about 2 GB of preconditioner.

Two uses: train on a subset with the dense fvgp_amd.GP, then predict with everything --

    gp = GP(x_sub, y_sub, ...); gp.train(...)
    big = gp.matrix_free(x_all, y_all, noise_all)
    big.posterior_mean(x_pred); big.posterior_covariance(x_pred, variance_only=True)

-- or learn from everything with the stochastic likelihood: big.train_stochastic(bounds).

With alpha = (K + V)^-1 (y - m) and Z = (K + V)^-1 k(X, x*):   m(x*) = m + k(x*, X) alpha,   v = k** - sum k o Z,
S = k** - k(x*, X) Z.

The likelihood on this path is an ESTIMATE with a reported standard error.  With A = K + V, M = G^T G + V the preconditioner and probes
z_c ~ N(0, M) (fvgp_hip_precond_probes):   log det A = log det M + mean_c rho_0 e_1^T log(T_c) e_1, T_c the Lanczos tridiagonal the
preconditioned CG on A u_c = z_c records (fvgp_hip_pcg_lanczos), log det M in closed form;   tr(A^-1 dK_j) = mean_c u_c^T dK_j (M^-1 z_c)
(fvgp_hip_precond_apply, fvgp_hip_kgrad_form).  Only the kernel's own hyperparameters get a gradient: the noise is numbers here.  The
exact Hessian stays with the dense GP.

A second preconditioner, args={"preconditioner": "vecchia"}: the sparse inverse Cholesky factor W of the nearest-neighbour
approximation, (K + V)^-1 ~ W^T W (fvgp_hip_nn_factor, fvgp_hip_pcg_nn).  It is local where the pivoted Cholesky is global: its iteration
count stays flat once the data outnumber what q columns can span, and it loses on small, globally smooth problems, which is why "pchol"
stays the default.  The object then owns a VecchiaGP over the same data for the ordering and the neighbour lists and holds its rows in
that ordering; the caller's order shows in solve and in x_data / y_data / noise_variances alone.  The stochastic likelihood needs probes
z ~ N(0, M), a sparse triangular solve that is not built: those names raise NotImplementedError under this preconditioner.
"""
import warnings

import numpy as np

from . import _lib
from . import gp_training as _training
from . import kernels as _kernels
from .device import default_handle
from .gp_lin_alg import NonPositiveDefiniteError

# device bytes the solved columns Z = (K + V)^-1 k(X, x*) of one posterior_covariance call may take (n x P doubles);
# args["z_max_bytes"] overrides it per object
Z_MAX_BYTES = 2 << 30
_DENSE = "the dense fvgp_amd.GP has it (train on a subset there, then GP.matrix_free(...) predicts with all the data)"


class MatrixFreeGP:
    """Posterior mean, variance and small joint covariances of an exact GP whose covariance matrix is never formed.

    x_data (N, D), y_data (N,), hyperparameters in the named kernel's layout, noise_variances (N,) or None (the rule and the warning
    of GP: (0.01 mean|y|)^2).  The prior mean is mean(y).  args: "precond_rank" (128; 0 = Jacobi), "tol" (1e-10, relative
    residual), "max_iter" (1000), "check_every" (8), "max_restarts" (3), "pchol_tol" (1e-12), "z_max_bytes"; for the stochastic
    likelihood "probe_tol" (1e-6: the relative residual of the probe solves, a default and not a measured optimum; alpha keeps "tol"),
    "lanczos_steps" (64: CG coefficients recorded per probe) and "stochastic_likelihood" (False; True lets the fvgp.GP method names
    log_likelihood, neg_log_likelihood, neg_log_likelihood_gradient and train return the estimates).

    "preconditioner": "pchol" (default: the rank-q pivoted Cholesky above) or "vecchia": the nearest-neighbour factor, with
    "precond_neighbors" (32; 1 .. 64), "precond_ordering" ("random" (default), "maxmin", "given" or a permutation), "seed" (0),
    "maxmin_points", "neighbor_scales" and "neighbor_search" as VecchiaGP takes them (its checks and messages).  The lists and their
    transpose are built once per data set (the transpose on the host: a stable sort); set_hyperparameters keeps them and recomputes the
    factor alone, lazily.  neighbors() and preconditioner_factor() show the structure."""

    def __init__(self, x_data, y_data, hyperparameters, noise_variances=None, kernel_function="matern32_ard", args=None, _vecchia=None):
        native = _kernels.resolve(kernel_function) if not callable(kernel_function) or isinstance(kernel_function, _kernels.NativeKernel) \
            else None
        if native is None:
            raise NotImplementedError("MatrixFreeGP evaluates the kernel on the device inside every product: only the named kernels of "
                                      "fvgp_amd.kernels run here; a kernel callable belongs to the dense fvgp_amd.GP")
        assert isinstance(x_data, np.ndarray) and np.ndim(x_data) == 2, "x_data must be 2-d (n_points x input_dim)"
        assert isinstance(y_data, np.ndarray) and np.ndim(y_data) == 1, "y_data must be a 1-d np.ndarray (fvGP / x_out: " + _DENSE + ")"
        assert len(x_data) == len(y_data), "x_data and y_data do not have the same lengths."
        self._native = native
        self.args = {} if args is None else dict(args)
        self.preconditioner = self.args.get("preconditioner", "pchol")
        if self.preconditioner not in ("pchol", "vecchia"):
            raise ValueError(f"args['preconditioner'] must be 'pchol' or 'vecchia', got {self.preconditioner!r}")
        self._vecchia_given = _vecchia          # VecchiaGP.matrix_free: the object whose ordering and lists this one shares
        self._init_hps = hyperparameters
        self.precond_rank = int(self.args.get("precond_rank", 128))
        assert 0 <= self.precond_rank <= _lib.PCG_MAX_RANK, f"precond_rank must lie in 0 .. {_lib.PCG_MAX_RANK}"
        self.tol = float(self.args.get("tol", 1e-10))
        self.max_iter = int(self.args.get("max_iter", 1000))
        self.check_every = int(self.args.get("check_every", 8))
        self.max_restarts = int(self.args.get("max_restarts", 3))
        self.probe_tol = float(self.args.get("probe_tol", 1e-6))
        self.lanczos_steps = int(self.args.get("lanczos_steps", 64))
        assert 1 <= self.lanczos_steps <= _lib.LANCZOS_MAX_STEPS, f"lanczos_steps must lie in 1 .. {_lib.LANCZOS_MAX_STEPS}"
        self.stochastic_likelihood = bool(self.args.get("stochastic_likelihood", False))
        self._scratch = {}
        self._H = default_handle()
        if noise_variances is None:
            warnings.warn("No noise function or measurement noise provided. "
                          "Noise variances will be set to (0.01 * mean(|y_data|))^2.", stacklevel=2)
        self._set_data(x_data, y_data, noise_variances)
        self._alpha = None                  # device (n, 1): (K + V)^-1 (y - m) at self._hps
        self._alpha_info = None
        self.set_hyperparameters(hyperparameters)

    # ---- state -----------------------------------------------------------------------------------------------------------
    def _set_data(self, x_data, y_data, noise_variances):
        H = self._H
        self.x_data = np.ascontiguousarray(x_data, dtype=np.float64)
        self.y_data = np.ascontiguousarray(y_data, dtype=np.float64)
        self.point_number, self.index_set_dim = self.x_data.shape
        if self.index_set_dim > 16:
            raise NotImplementedError("the device kernels take input dimension <= 16")
        if noise_variances is None:
            V = np.ones(self.point_number) * (np.mean(abs(self.y_data)) / 100.0) ** 2
        else:
            V = np.asarray(noise_variances, dtype=np.float64)
            assert V.shape == (self.point_number,), "noise_variances must be 1-d, one per data point"
            assert np.all(V > 0.0), "all noise_variances must be positive"
        self.noise_variances = noise_variances
        self._V = np.ascontiguousarray(V)
        self._m = float(np.mean(self.y_data))
        self._G = self._C = self._W = None
        if self.preconditioner == "vecchia":
            self._set_structure()
        else:
            self._x_dev, self._V_dev = H.to_device(self.x_data), H.to_device(self._V)
            self._ym_dev = H.to_device((self.y_data - self._m)[:, None])
        self._scratch = {}
        self._rank = 0

    def _set_structure(self):
        """the "vecchia" preconditioner's structure for the data as they are: a VecchiaGP over them (the one given by
        VecchiaGP.matrix_free the first time, else one of this object's own) lends its ordering, its ordered device arrays and its
        lists; the transposed lists are built here, once"""
        from .gp_vecchia import VecchiaGP
        nn, a = self._vecchia_given, self.args
        if nn is None:
            hps = getattr(self, "_hps", None)
            kw = {k: a[k] for k in ("maxmin_points", "neighbor_scales", "neighbor_search") if k in a}
            nn = VecchiaGP(self.x_data, self.y_data, self._init_hps if hps is None else hps, noise_variances=self._V,
                           kernel_function=self._native, n_neighbors=a.get("precond_neighbors", 32),
                           ordering=a.get("precond_ordering", "random"), seed=a.get("seed", 0), args=kw)
        else:
            # (an update of this object's data makes its own structure by the given object's rules)
            self.args.update({"precond_neighbors": nn.n_neighbors, "precond_ordering": nn._ordering_rule[0], "seed": nn._ordering_rule[1]})
            self.args.update({k: nn.args[k] for k in ("maxmin_points", "neighbor_scales", "neighbor_search") if k in nn.args})
            self._vecchia_given = None
        if not isinstance(self.args.get("precond_ordering", "random"), str):
            self.args["precond_ordering"] = "given"     # (a permutation orders the data it came with; later data come as given)
        self._nn = nn
        self.precond_neighbors = nn.n_neighbors
        self.ordering = nn.ordering
        self._x_dev, self._V_dev, self._ym_dev, self._idx = nn._x_dev, nn._V_dev, nn._r_dev[:, None], nn._idx
        self._perm_dev = self._H.torch.as_tensor(self.ordering, device=self._x_dev.device)
        self._transposed = self._H.nn_transpose(self._idx, self.precond_neighbors)

    def neighbors(self):
        """("vecchia" preconditioner) (N, m) int64: row i lists the neighbours of the caller's data point i as the caller's indices,
        nearest first, -1 where the ordering leaves fewer than m earlier points"""
        self._vecchia_only("neighbors")
        idx = self._idx.cpu().numpy().astype(np.int64)
        out = np.full_like(idx, -1)
        out[self.ordering] = np.where(idx >= 0, self.ordering[np.clip(idx, 0, None)], -1)
        return out

    def preconditioner_factor(self):
        """("vecchia" preconditioner) the _lib.NNFactor at the current hyperparameters, rows in the ordering: built once per
        hyperparameter vector; the lists and their transpose are those of the data"""
        self._vecchia_only("preconditioner_factor")
        if self._W is None:
            H = self._H
            self._W, info = H.nn_factor(self._native.kernel_id, self._x_dev, self._hps, self._idx, self.precond_neighbors, self._V_dev,
                                        transposed=self._transposed)
            if info:
                self._W = None
                raise NonPositiveDefiniteError(
                    f"the nearest-neighbour preconditioner: the conditional of data point {int(self.ordering[int(info) - 1])} is not "
                    f"positive definite in double precision -- its {self.precond_neighbors} x {self.precond_neighbors} neighbour block "
                    "K + V or its conditional variance has a pivot that is not positive; duplicated points need positive noise, or "
                    "rethink the hyperparameters")
        return self._W

    def _vecchia_only(self, what):
        if self.preconditioner != "vecchia":
            raise NotImplementedError(f"{what} belongs to args={{'preconditioner': 'vecchia'}}: the pivoted-Cholesky preconditioner has "
                                      "no neighbour lists")

    def _no_probes(self, what):
        if self.preconditioner == "vecchia":
            raise NotImplementedError(
                f"{what}: the stochastic likelihood draws probes z ~ N(0, M) from the preconditioner, which for the nearest-neighbour "
                "factor is a sparse triangular solve that is not built.  Use preconditioner=\"pchol\" for the estimates, or VecchiaGP, "
                "whose deterministic likelihood (log_likelihood, neg_log_likelihood_and_gradient, train) is built on the same factor")

    @property
    def hyperparameters(self):
        return self._hps

    def get_hyperparameters(self):
        return self._hps

    def set_hyperparameters(self, hps):
        hps = np.array(hps, dtype=np.float64)
        assert hps.shape == (self._native.n_hyperparameters(self.index_set_dim),), "wrong number of hyperparameters for this kernel"
        self._hps = hps
        self._alpha = self._alpha_info = None
        self._G = self._C = self._W = None

    def _build_preconditioner(self, hps):
        """(G, q, C) at hps: the pivoted Cholesky of K and the factor of I + G V^-1 G^T; nothing is kept"""
        if self.precond_rank == 0:
            return None, 0, None
        H, n = self._H, self.point_number
        q = min(self.precond_rank, n)
        G = H.empty(q, n)
        piv = H.torch.empty(q, dtype=H.torch.int64, device=G.device)
        rank = H.pchol(self._native.kernel_id, self._x_dev, hps, q, G, piv, tol=float(self.args.get("pchol_tol", 1e-12)))
        qp = _lib.pad128(q)
        C = H.empty(qp, qp)
        info = H.precond_factor(G, q, n, self._V_dev, C)
        if info != 0:
            raise NonPositiveDefiniteError(f"the preconditioner's {q} x {q} system I + G V^-1 G^T is not positive definite "
                                           f"(pivot {info}): the noise variances or the hyperparameters are no numbers")
        self._rank = rank
        return G, q, C

    def _preconditioner(self):
        """(G, q, C) at the current hyperparameters, built once"""
        if self.precond_rank == 0:
            return None, 0, None
        if self._G is None:
            self._G, self._q, self._C = self._build_preconditioner(self._hps)
        return self._G, self._q, self._C

    def _buffer(self, name, doubles):
        """a flat device buffer of at least `doubles` doubles, kept under `name` and regrown when too small"""
        buf = self._scratch.get(name)
        if buf is None or buf.numel() < doubles:
            buf = self._scratch[name] = self._H.empty(max(1, int(doubles)))
        return buf

    def _pcg(self, B, X, s, warm=False, at=None, tol=None, lanczos_steps=0):
        """one solver call of s <= 16 columns; at = (hps, G, q, C) solves at other hyperparameters than the object's; lanczos_steps > 0
        also returns the records (alpha, beta, steps, rho0)"""
        H, n = self._H, self.point_number
        tol = self.tol if tol is None else tol
        if self.preconditioner == "vecchia":
            assert at is None and not lanczos_steps, "the nearest-neighbour preconditioner serves the plain solves at the object's hyperparameters"
            work = self._buffer("pcg", _lib.pcg_nn_workspace_bytes(n) // 8)
            return H.pcg_nn(self._native.kernel_id, self._x_dev, self._hps, self._V_dev, B, X, self.preconditioner_factor(), s=s, warm=warm,
                            tol=tol, max_iter=self.max_iter, check_every=self.check_every, max_restarts=self.max_restarts, work=work)
        hps, G, q, C = at if at is not None else (self._hps,) + self._preconditioner()
        kw = dict(G=G, q=q, C=C, s=s, warm=warm, tol=tol, max_iter=self.max_iter, check_every=self.check_every,
                  max_restarts=self.max_restarts)
        if lanczos_steps:
            work = self._buffer("pcg", _lib.pcg_lanczos_workspace_bytes(n, q, lanczos_steps) // 8)
            return H.pcg_lanczos(self._native.kernel_id, self._x_dev, hps, self._V_dev, B, X, lanczos_steps, work=work, **kw)
        work = self._buffer("pcg", _lib.pcg_workspace_bytes(n, q) // 8)
        return H.pcg(self._native.kernel_id, self._x_dev, hps, self._V_dev, B, X, work=work, **kw)

    def _breakdown(self):
        return NonPositiveDefiniteError(
            f"conjugate gradients broke down on K + V ({self.point_number} points, smallest noise variance "
            f"{float(np.min(self._V)):.3e}): p^T (K + V) p or r^T M^-1 r was not positive -- the matrix is not positive "
            "definite in double precision; add noise or rethink the hyperparameters")

    def _solve_device(self, B, X, warm=False, at=None):
        """X (n, c) <- (K + V)^-1 B (n, c) on the device in blocks of 16 columns; (iterations, residuals, converged) per column"""
        c = B.shape[1]
        its, res, ok = np.zeros(c, dtype=np.int64), np.zeros(c), np.zeros(c, dtype=bool)
        for a in range(0, c, _lib.PCG_MAX_RHS):
            b = min(a + _lib.PCG_MAX_RHS, c)
            it, rr, st = self._pcg(B[:, a:b], X[:, a:b], b - a, warm=warm, at=at)
            if np.any(st == 2):
                raise self._breakdown()
            its[a:b], res[a:b], ok[a:b] = it, rr, st == 0
        if not np.all(ok):
            warnings.warn(f"conjugate gradients did not converge: relative residual {float(np.max(res)):.3e} reached, "
                          f"tol = {self.tol:.1e} asked, after at most {int(np.max(its))} iterations (args: max_iter, "
                          "precond_rank, tol)", stacklevel=3)
        return its, res, ok

    # ---- public ----------------------------------------------------------------------------------------------------------
    def solve(self, b):
        """(K + V)^-1 b for b (n,) or (n, c); the prediction state (alpha) is not touched"""
        b = np.asarray(b, dtype=np.float64)
        one = b.ndim == 1
        b = b.reshape(self.point_number, -1)
        ordered = self.preconditioner == "vecchia"      # (the rows are held in the ordering: b goes in permuted, x comes out permuted)
        B = self._H.to_device(b[self.ordering] if ordered else b)
        X = self._H.empty(*B.shape)
        its, res, ok = self._solve_device(B, X)
        x = self._H.to_host(X)
        if ordered:
            xo = x
            x = np.empty_like(xo)
            x[self.ordering] = xo
        return {"x": x[:, 0].copy() if one else x, "iterations": its, "relative_residual": res, "converged": bool(np.all(ok))}

    def _ensure_alpha(self, warm_from=None):
        if self._alpha is None:
            X = self._H.zeros(self.point_number, 1)
            if warm_from is not None:
                X[:warm_from.shape[0]] = warm_from
            its, res, ok = self._solve_device(self._ym_dev, X, warm=warm_from is not None)
            self._alpha = X
            self._alpha_info = {"iterations": int(its[0]), "relative_residual": float(res[0]), "converged": bool(ok[0])}
        return self._alpha

    def _check_pred(self, x_pred, x_out=None):
        if x_out is not None:
            raise NotImplementedError("x_out / fvGP outputs are not on the matrix-free path: " + _DENSE)
        assert isinstance(x_pred, np.ndarray) and np.ndim(x_pred) == 2, "x_pred must be a 2-d np.ndarray"
        assert x_pred.shape[1] == self.index_set_dim, "wrong number of columns in x_pred"
        return self._H.to_device(x_pred)

    def _cross(self, xp_dev, B, c):
        """k(x_pred, X) B[:, :c] on the device: the rectangular product, split over chunk ranges when few points meet many rows"""
        H, n, P = self._H, self.point_number, xp_dev.shape[0]
        out = H.empty(P, c)
        work = H.empty(max(1, _lib.kmatvec_workspace_bytes(P, n, c) // 8)) if P < 32768 else None
        H.kmatvec(self._native.kernel_id, xp_dev, self._x_dev, self._hps, B, out, s=c, work=work)
        return out

    def posterior_mean(self, x_pred, hyperparameters=None, x_out=None):
        if hyperparameters is not None:
            raise NotImplementedError("posterior_mean(hyperparameters=...) would solve for a second alpha: call "
                                      "set_hyperparameters first, or use the dense GP; " + _DENSE)
        xp = self._check_pred(x_pred, x_out)
        alpha = self._ensure_alpha()
        mean = self._m + self._H.to_host(self._cross(xp, alpha, 1))[:, 0]
        return {"x": x_pred.copy(), "m(x)": mean, "m(x)_flat": mean, "x_pred": x_pred, **self._alpha_info}

    def posterior_covariance(self, x_pred, x_out=None, variance_only=False, add_noise=False):
        xp = self._check_pred(x_pred, x_out)
        H, n, P = self._H, self.point_number, len(x_pred)
        budget = int(self.args.get("z_max_bytes", Z_MAX_BYTES))
        if 2 * n * P * 8 > budget:
            raise MemoryError(f"posterior_covariance at {P} points needs k(X, x*) and its solved columns, 2 x {n} x {P} doubles = "
                              f"{2 * n * P * 8 / 2 ** 30:.2f} GiB, above the budget of {budget / 2 ** 30:.2f} GiB "
                              "(args['z_max_bytes']): predict in smaller batches of points")
        kid = self._native.kernel_id
        Kx, Z = H.empty(n, P + (P & 1))[:, :P], H.empty(n, P)
        H.kmat(kid, self._x_dev, xp, self._hps, Kx)                      # k(X, x*): the right-hand sides
        self._solve_device(Kx, Z)
        sig = float(self._hps[0])
        # k(x*, X) Z through the product's bit contract: a point's variance does not depend on what else is in the call
        v, S = np.empty(P), None
        if not variance_only:
            S = np.empty((P, P))
        for a in range(0, P, _lib.PCG_MAX_RHS):
            b = min(a + _lib.PCG_MAX_RHS, P)
            if variance_only:
                v[a:b] = sig - np.diag(H.to_host(self._cross(xp[a:b], Z[:, a:b], b - a)))
            else:
                S[:, a:b] = H.to_host(self._cross(xp, Z[:, a:b], b - a))
        if S is not None:
            kk = H.empty(P, P + (P & 1))
            H.kmat(kid, xp, xp, self._hps, kk)
            v = sig - np.diag(S)
            S = H.to_host(kk)[:, :P] - S
            S = 0.5 * (S + S.T)
            np.fill_diagonal(S, v)
        if np.any(v < -0.0001):
            warnings.warn("Negative variances encountered. That normally means that the model is unstable. "
                          "Rethink the kernel definition, add more noise to the data, "
                          "or double check the hyperparameter optimization bounds. This will not "
                          "terminate the algorithm, but expect anomalies.")
        if np.any(v < 0.0):
            v[v < 0.0] = 0.0
            if S is not None:
                np.fill_diagonal(S, v)
        if add_noise:
            noise = self._V if len(x_pred) == n else np.zeros(P) + np.mean(self._V)
            v = v + noise
            if S is not None:
                S = S + np.diag(noise)
        return {"x": x_pred.copy(), "x_pred": x_pred, "v(x)": v, "S": S, "S_flat": S, "v_flat": v}

    def update_gp_data(self, x_new, y_new, noise_variances_new=None, append=True):
        """new data (appended, or replacing everything): the preconditioner is rebuilt and alpha warm-starts from the old one padded
        with zeros"""
        assert isinstance(x_new, np.ndarray) and np.ndim(x_new) == 2 and isinstance(y_new, np.ndarray) and np.ndim(y_new) == 1
        old = self._alpha if append else None
        if old is not None and self.preconditioner == "vecchia":
            old = self._H.torch.empty_like(old)
            old[self._perm_dev] = self._alpha           # (the old alpha in the caller's order)
        if append:
            if (self.noise_variances is None) != (noise_variances_new is None):
                raise Exception("noise_variances_new must be given exactly when the object was built with noise_variances")
            x_new = np.vstack([self.x_data, x_new])
            y_new = np.concatenate([self.y_data, y_new])
            if noise_variances_new is not None:
                noise_variances_new = np.concatenate([self.noise_variances, noise_variances_new])
        self._set_data(x_new, y_new, noise_variances_new)
        self._alpha = self._alpha_info = None
        if old is not None:
            # (the prior mean moved with the data: the old alpha still nearly solves the old rows, which is all a start needs)
            if self.preconditioner == "vecchia":        # (into the new ordering, the new rows zero)
                full = self._H.zeros(self.point_number, 1)
                full[:old.shape[0]] = old
                old = full[self._perm_dev]
            self._ensure_alpha(warm_from=old)

    # ---- the stochastic likelihood -----------------------------------------------------------------------------------
    @staticmethod
    def _quadrature(alpha, beta, rho0):
        """rho_0 e_1^T log(T) e_1 with T the Lanczos tridiagonal of the recorded CG coefficients: T[k, k] = 1 / alpha_k +
        beta_{k-1} / alpha_{k-1}, T[k, k+1] = sqrt(beta_k) / alpha_k; numpy.linalg.eigh on the dense T (a few hundred rows at most)"""
        m = len(alpha)
        if m == 0:
            return 0.0
        T = np.zeros((m, m))
        for k in range(m):
            T[k, k] = 1.0 / alpha[k] + (beta[k - 1] / alpha[k - 1] if k else 0.0)
            if k + 1 < m:
                T[k, k + 1] = T[k + 1, k] = np.sqrt(beta[k]) / alpha[k]
        lam, Q = np.linalg.eigh(T)
        return float(rho0 * np.sum(Q[0] ** 2 * np.log(lam)))

    def log_likelihood_estimate(self, hyperparameters=None, n_probes=16, seed=0, gradient=False):
        """The log marginal likelihood at the object's hyperparameters, or at `hyperparameters` with a preconditioner of its own and
        the object's state untouched.  A dict: "log_likelihood" and its "std_error" (over the probes), "logdet" = log det(K + V) with
        "logdet_std_error", "logdet_preconditioner", "data_fit" = 1/2 (y - m)^T alpha, "per_probe" (n_probes,): every probe's
        rho_0 e_1^T log(T) e_1, "iterations" and "lanczos_steps" per probe, "alpha_iterations", "converged"; with gradient=True also
        "neg_gradient" over the kernel's own hyperparameters, d(-log L)/dtheta_j = -1/2 alpha^T dK_j alpha + 1/2 tr((K + V)^-1 dK_j), and
        "neg_gradient_std_error": half the spread of the trace over groups of 4 probes (one fvgp_hip_kgrad_form call each).  The same
        (hyperparameters, n_probes, seed) returns the same bits: the probes are a pure function of the seed."""
        self._no_probes("log_likelihood_estimate")
        H, n, kid = self._H, self.point_number, self._native.kernel_id
        n_probes = int(n_probes)
        assert n_probes >= 1, "n_probes must be at least 1"
        if hyperparameters is None:
            hps = self._hps
            G, q, C = self._preconditioner()
            at = None
            alpha = self._ensure_alpha()
            alpha_info = self._alpha_info
        else:
            hps = np.array(hyperparameters, dtype=np.float64)
            assert hps.shape == self._hps.shape, "wrong number of hyperparameters for this kernel"
            G, q, C = self._build_preconditioner(hps)
            at = (hps, G, q, C)
            alpha = H.zeros(n, 1)
            its, res, ok = self._solve_device(self._ym_dev, alpha, at=at)
            alpha_info = {"iterations": int(its[0]), "relative_residual": float(res[0]), "converged": bool(ok[0])}
        fit = 0.5 * H.dot(self._ym_dev, alpha, n)
        ldm = float(np.sum(np.log(self._V))) + (H.logdet(C, q) if q else 0.0)

        S = _lib.PCG_MAX_RHS
        Z, U, W = H.empty(n, S), H.empty(n, S), H.empty(n, S)
        awork = self._buffer("apply", _lib.precond_apply_workspace_bytes(n, q) // 8)
        gwork = self._buffer("form", _lib.kgrad_form_workspace_bytes(n, n) // 8)
        quad, its, steps, res = np.zeros(n_probes), np.zeros(n_probes, dtype=np.int64), np.zeros(n_probes, dtype=np.int64), np.zeros(n_probes)
        ok = np.zeros(n_probes, dtype=bool)
        n_own = self._native.n_hyperparameters(self.index_set_dim)
        sums, means = np.zeros(n_own), []
        for c0 in range(0, n_probes, S):
            s = min(S, n_probes - c0)
            H.precond_probes(Z[:, :s], self._V_dev, G=G, q=q, seed=seed, stream=0, col0=c0)
            it, rr, st, al, be, stp, rho0 = self._pcg(Z, U, s, at=at, tol=self.probe_tol, lanczos_steps=self.lanczos_steps)
            if np.any(st == 2):
                raise self._breakdown()
            for c in range(s):
                m = int(stp[c])
                quad[c0 + c] = self._quadrature(al[c, :m], be[c, :max(m - 1, 0)], rho0[c])
            its[c0:c0 + s], steps[c0:c0 + s], res[c0:c0 + s], ok[c0:c0 + s] = it, stp, rr, st == 0
            if gradient:
                H.precond_apply(Z, W, self._V_dev, G=G, q=q, C=C, s=s, work=awork)
                for g0 in range(0, s, 4):
                    g1 = min(g0 + 4, s)
                    f = H.kgrad_form(kid, self._x_dev, U[:, g0:g1], self._x_dev, W[:, g0:g1], hps, work=gwork)[:n_own]
                    sums += f
                    means.append(f / (g1 - g0))
        if not np.all(ok):
            warnings.warn(f"conjugate gradients did not converge on the probes: relative residual {float(np.max(res)):.3e} reached, "
                          f"probe_tol = {self.probe_tol:.1e} asked, after at most {int(np.max(its))} iterations (args: max_iter, "
                          "precond_rank, probe_tol)", stacklevel=2)
        logdet = ldm + float(np.mean(quad))
        ld_se = float(np.std(quad, ddof=1) / np.sqrt(n_probes)) if n_probes > 1 else float("nan")
        out = {"log_likelihood": -(fit + 0.5 * logdet + 0.5 * n * np.log(2.0 * np.pi)), "std_error": 0.5 * ld_se, "logdet": logdet,
               "logdet_std_error": ld_se, "logdet_preconditioner": ldm, "data_fit": fit, "per_probe": quad, "iterations": its,
               "lanczos_steps": steps, "alpha_iterations": alpha_info["iterations"],
               "converged": bool(np.all(ok) and alpha_info["converged"])}
        if gradient:
            a_term = H.kgrad_form(kid, self._x_dev, alpha, self._x_dev, alpha, hps, s=1, work=gwork)[:n_own]
            trace = sums / n_probes
            tr_se = np.std(np.array(means), axis=0, ddof=1) / np.sqrt(len(means)) if len(means) > 1 else np.full(n_own, np.nan)
            out.update({"neg_gradient": -0.5 * a_term + 0.5 * trace, "neg_gradient_std_error": 0.5 * tr_se, "trace": trace,
                        "trace_std_error": tr_se})
        return out

    def stochastic_log_likelihood(self, hyperparameters=None, n_probes=16, seed=0):
        self._no_probes("stochastic_log_likelihood")
        return self.log_likelihood_estimate(hyperparameters, n_probes, seed)["log_likelihood"]

    def stochastic_neg_log_likelihood(self, hyperparameters=None, n_probes=16, seed=0):
        self._no_probes("stochastic_neg_log_likelihood")
        return -self.log_likelihood_estimate(hyperparameters, n_probes, seed)["log_likelihood"]

    def stochastic_neg_log_likelihood_gradient(self, hyperparameters=None, n_probes=16, seed=0):
        self._no_probes("stochastic_neg_log_likelihood_gradient")
        return self.log_likelihood_estimate(hyperparameters, n_probes, seed, gradient=True)["neg_gradient"]

    def stochastic_neg_log_likelihood_and_gradient(self, hyperparameters=None, n_probes=16, seed=0):
        self._no_probes("stochastic_neg_log_likelihood_and_gradient")
        e = self.log_likelihood_estimate(hyperparameters, n_probes, seed, gradient=True)
        return -e["log_likelihood"], e["neg_gradient"]

    def train_stochastic(self, hyperparameter_bounds, init_hyperparameters=None, max_iter=200, lr=1e-2, tolerance=1e-4, n_probes=16, seed=0,
                         callback=None):
        """Adam (gp_training.adam_optimize) on the estimated negative log-likelihood with the SAME seed at every step -- common random
        numbers: the objective is then a deterministic function of theta -- every iterate clipped into hyperparameter_bounds (H, 2).
        Ends with set_hyperparameters(theta) and returns (theta, history)."""
        self._no_probes("train_stochastic")
        bounds = np.asarray(hyperparameter_bounds, dtype=np.float64)
        assert bounds.ndim == 2 and bounds.shape == (len(self._hps), 2), "wrong bounds format"
        theta0 = np.array(self._hps if init_hyperparameters is None else init_hyperparameters, dtype=np.float64)
        if np.any(theta0 < bounds[:, 0]) or np.any(theta0 > bounds[:, 1]):
            raise Exception("Starting positions outside of optimization bounds.", theta0, bounds)
        last = {}

        def evaluate(theta):
            key = theta.tobytes()
            if last.get("key") != key:
                last["key"], last["value"] = key, self.stochastic_neg_log_likelihood_and_gradient(theta, n_probes, seed)
            return last["value"]

        theta, history = _training.adam_optimize(lambda t: evaluate(t)[0], lambda t: evaluate(t)[1], theta0, lr=lr, max_iter=max_iter,
                                                 tol=tolerance, callback=callback,
                                                 project=lambda t: np.clip(t, bounds[:, 0], bounds[:, 1]))
        self.set_hyperparameters(theta)
        return theta, history

    # ---- the fvgp.GP method names ----------------------------------------------------------------------------------------------
    def _dense_only(self, what):
        raise NotImplementedError(f"{what} needs log det(K + V) or traces with (K + V)^-1; on the matrix-free path these are stochastic "
                                  "estimates (log_likelihood_estimate, stochastic_neg_log_likelihood_gradient, train_stochastic), and "
                                  "this method name returns them only with args={'stochastic_likelihood': True}.  Exact values: "
                                  + _DENSE)

    def log_likelihood(self, hyperparameters=None):
        if not self.stochastic_likelihood:
            self._dense_only("log_likelihood")
        return self.stochastic_log_likelihood(hyperparameters)

    def neg_log_likelihood(self, hyperparameters=None):
        if not self.stochastic_likelihood:
            self._dense_only("neg_log_likelihood")
        return self.stochastic_neg_log_likelihood(hyperparameters)

    def neg_log_likelihood_gradient(self, hyperparameters=None, component=0):
        if not self.stochastic_likelihood:
            self._dense_only("neg_log_likelihood_gradient")
        return self.stochastic_neg_log_likelihood_gradient(hyperparameters)

    def neg_log_likelihood_hessian(self, hyperparameters=None):
        raise NotImplementedError("neg_log_likelihood_hessian: there is no stochastic Hessian on the matrix-free path: " + _DENSE)

    def train(self, hyperparameter_bounds=None, init_hyperparameters=None, **kw):
        if not self.stochastic_likelihood:
            self._dense_only("train")
        assert hyperparameter_bounds is not None, "train needs hyperparameter_bounds"
        return self.train_stochastic(hyperparameter_bounds, init_hyperparameters, **kw)[0]


class MatrixFreeMixin:
    """Mixed into fvgp_amd.GP: needs _native, _hps, _noise_callable, _mean_callable, x_data, y_data, noise_variances."""

    def matrix_free(self, x_data=None, y_data=None, noise_variances=None, args=None):
        """A MatrixFreeGP with this GP's kernel and CURRENT hyperparameters, over this GP's data or -- the point of it -- over MORE
        data than a dense factor can hold (x_data, y_data, noise_variances)."""
        if self._native is None:
            raise NotImplementedError("matrix_free evaluates the kernel on the device: a kernel callable stays with the dense GP "
                                      "(use one of the named kernels)")
        if self._noise_callable is not None or self._mean_callable is not None:
            raise NotImplementedError("matrix_free takes noise variances as numbers and the default prior mean: noise and mean "
                                      "callables stay with the dense GP")
        if self.y_data.shape[1] != 1:
            raise NotImplementedError("matrix_free takes one column of y (fvGP / x_out: the dense GP has it)")
        if (x_data is None) != (y_data is None):
            raise Exception("x_data and y_data come together")
        if x_data is None:
            x_data, y_data = self.x_data, self.y_data[:, 0]
            if noise_variances is None:
                noise_variances = self.noise_variances
        return MatrixFreeGP(x_data, y_data, self._hps.copy(), noise_variances=noise_variances, kernel_function=self._native, args=args)
