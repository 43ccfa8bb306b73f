"""A deterministic likelihood and prediction at sizes where no N x N factor fits: the nearest-neighbour (Vecchia / NNGP "response")
approximation (include/fvgp_hip_nn.h).

The data are put in an ordering, and the likelihood is written as a product of N small conditionals,

    p(y) ~ prod_i p(y_i | y_c(i)),      c(i) = the m nearest of the points that come EARLIER in the ordering,

each of them an m x m problem: with A = K(x_c, x_c) + diag(v_c), k = K(x_c, x_i), A = L L^T, w = L^-1 k, z = L^-1 (y_c - mean):
mu_i = mean + w^T z, d_i = k(x_i, x_i) + v_i - w^T w, and log p = -1/2 sum_i [(y_i - mu_i)^2 / d_i + log d_i + log 2 pi].  O(N m^3) time,
O(N m) memory, no iteration count and no standard error; with m >= N - 1 it IS the exact likelihood, and it approaches the exact GP's
values as m grows.  Prediction at x* conditions on the m nearest data points: the same small problem.

    big = VecchiaGP(x_all, y_all, hps, noise_all, n_neighbors=32)         # or gp.vecchia(x_all, y_all, noise_all)
    big.log_likelihood(); big.train(bounds, method="mcmc")
    f, g = big.neg_log_likelihood_and_gradient(); big.train_gradient(bounds, method="local")
    big.train_gradient(bounds, method="fisher"); big.hyperparameter_laplace()["std_error"]
    big.posterior_mean(x_pred); big.posterior_covariance(x_pred, variance_only=True)

The ordering decides how good the approximation is at a given m.  ordering="maxmin" is the literature's default (GpGp, GPvecchia): the
exact farthest-point ordering, computed on the device (fvgp_hip_nn_maxmin_order, DESIGN 27: N steps of O(N) work, one launch each), so
that the early conditioning sets span the domain and the late ones are local; args["maxmin_points"] = q orders only the first q
positions that way and bounds the construction to q launches.  ordering_distances keeps the distance at which each point entered.

"Nearest" is measured after dividing every coordinate by a scale (args["neighbor_scales"]: the length scales at construction, 1, or a
vector), and the neighbour lists stay FIXED while the hyperparameters move (set_hyperparameters, training): the likelihood is then a
smooth function of theta.  refresh_neighbors() rebuilds them, with reorder=True the maxmin ordering under the new scales as well.

The exact gradient of this likelihood comes from the same device call as its value (fvgp_hip_nn_loglik_grad: two back-substitutions with
the m x m factor that is already there, and one more sweep over each block's kernel entries with their derivatives):
neg_log_likelihood_and_gradient, its _batch forms, conditional_scores (the per-point terms that sum to it) and train_gradient ("local":
scipy's bounded optimisers, "adam": projected Adam, multi-start with args["adam_starts"]) are always there.  The fvgp.GP names
neg_log_likelihood_gradient and train(method="local" | "adam") take this route with args={"likelihood_gradient": True}.  Joint
covariances are not built.

The neighbour search itself has two routes that return the same lists element for element (args["neighbor_search"]): the brute search
(fvgp_hip_nn_search, O(N^2 d)) and, at input dimension <= 3, an exact search through a uniform cell grid over the ordered data
(fvgp_hip_nn_grid_build / _search, DESIGN 28, near-linear in N for data spread evenly).  The grid is built with the lists and kept for
prediction and appends; it is made again whenever the data, the ordering or the scales change.

The Fisher information of this likelihood -- the expected Hessian of neg_log_likelihood under the exact GP, positive semidefinite, in
closed form from the same factors (fvgp_hip_nn_loglik_fisher) -- comes from one more device call of about the gradient's cost
again: fisher_information, neg_log_likelihood_gradient_and_fisher and its _batch form, conditional_fisher (the per-point terms),
train_gradient(method="fisher") (projected Fisher scoring; train(method="fisher") with args={"likelihood_gradient": True}) and
hyperparameter_laplace (standard errors and hyperparameter samples from F^-1: the expected curvature, not the observed one)."""
import collections
import warnings

import numpy as np

from . import _lib
from . import fisher_scoring as _fisher
from . import gp_training as _training
from . import kernels as _kernels
from .device import default_handle
from .gp_lin_alg import NonPositiveDefiniteError

_DENSE = "the dense fvgp_amd.GP has it"
_LOG_2PI = float(np.log(2.0 * np.pi))
# args["neighbor_search"]: "auto" takes the cell grid (the same lists) at input dimension <= 3 from this many data points on --
# the smallest size measured (profiles/r21_vecchia_grid.txt: 10^4 .. 10^6) from which on grid build + search beat the brute search on
# every measured configuration; below it nothing was measured and the brute search stays
NEIGHBOR_SEARCH_DEFAULT = "auto"
NEIGHBOR_SEARCH_AUTO_POINTS = 10000
_Evaluation = collections.namedtuple("_Evaluation", "out grad fisher info mu var score rows")      # what VecchiaGP._evaluate returns


def first_point(x, scales=None):
    """where a maxmin ordering of the rows of x (n, d) starts: the point nearest, in the scaled coordinates x / scales, to their mean
    (ties to the lowest index) -- GpGp's convention"""
    z = x if scales is None else x * (1.0 / np.asarray(scales, dtype=np.float64))
    return int(np.argmin(np.sum((z - np.mean(z, axis=0)) ** 2, axis=1)))


class VecchiaGP:
    """The nearest-neighbour GP over x_data (N, D), y_data (N,): hyperparameters in the named kernel's layout, noise_variances (N,) or
    None (the rule and the warning of GP: (0.01 mean|y|)^2), prior mean = mean(y).

    n_neighbors: m in 1 .. 64.  ordering: "random" (a permutation drawn from `seed`), "given" (the caller's order), "maxmin" (the exact
    farthest-point ordering under the neighbour scales, from the point nearest the centre of the scaled data) or a permutation array;
    the data are held in that order and everything returned per data point is in the CALLER's order.  ordering_distances (N,), in
    ordering position: under "maxmin" the scaled distance to the nearest earlier point at which each point entered (inf at position 0,
    nan past args["maxmin_points"] and for appended points), else None.  args: "maxmin_points" (None: all N; q in 1 .. N: only the
    first q positions are ordered by maxmin, the other points follow in a random order drawn from `seed`);
    "neighbor_scales" = "lengthscales" (default: the kernel's length scales at construction), "unit" or a D-vector;
    "batch_population" (True: train(method="global") scores a generation in one device call); "likelihood_gradient" (True: the fvgp.GP
    names neg_log_likelihood_gradient and train(method="local" | "adam" | "fisher") run the exact gradient); "adam_starts" (S >= 2:
    train_gradient(method="adam") runs S trajectories in lockstep on the batched gradient); "grad_batch_bytes" (default 1 GiB: the most
    device memory one batched gradient or Fisher call may take for its per-row outputs); "neighbor_search" = "auto" (default: the cell
    grid where the input dimension is <= 3 and there are at least NEIGHBOR_SEARCH_AUTO_POINTS = 10 000 data points, else the brute
    search), "grid" (the cell grid; ValueError at input dimension > 3) or "brute" -- the same neighbour lists, likelihood bits and
    predictions on either route."""

    def __init__(self, x_data, y_data, hyperparameters, noise_variances=None, kernel_function="matern32_ard", n_neighbors=32,
                 ordering="random", seed=0, args=None):
        native = _kernels.resolve(kernel_function) if not callable(kernel_function) or isinstance(kernel_function, _kernels.NativeKernel) \
            else None
        if native is None:
            raise NotImplementedError("VecchiaGP evaluates the kernel on the device inside every conditional: only the named kernels of "
                                      "fvgp_amd.kernels run here; a kernel callable belongs to the dense fvgp_amd.GP")
        assert isinstance(x_data, np.ndarray) and np.ndim(x_data) == 2, "x_data must be 2-d (n_points x input_dim)"
        if not isinstance(y_data, np.ndarray) or np.ndim(y_data) != 1:
            raise NotImplementedError("y_data must be a 1-d np.ndarray: fvGP / x_out outputs are not on the nearest-neighbour path, "
                                      + _DENSE)
        assert len(x_data) == len(y_data), "x_data and y_data do not have the same lengths."
        self.args = {} if args is None else dict(args)
        if self.args.get("process_group") not in (None, False):
            raise NotImplementedError("the row-sharded mode (args['process_group']) belongs to the dense fvgp_amd.GP: the "
                                      "nearest-neighbour path runs on one device")
        self.args.setdefault("batch_population", True)
        self.likelihood_gradient = bool(self.args.get("likelihood_gradient", False))
        if int(n_neighbors) != n_neighbors or not 1 <= int(n_neighbors) <= _lib.NN_MAX_NEIGHBORS:
            raise ValueError(f"n_neighbors must lie in 1 .. {_lib.NN_MAX_NEIGHBORS}, got {n_neighbors!r}")
        self.n_neighbors = int(n_neighbors)
        self._native = native
        self._H = default_handle()
        if noise_variances is None:
            warnings.warn("No noise function or measurement noise provided. "
                          "Noise variances will be set to (0.01 * mean(|y_data|))^2.", stacklevel=2)
        self._check_dim(x_data)
        self._hps = self._check_hps(hyperparameters, x_data.shape[1])
        self._scale_mode = self.args.get("neighbor_scales", "lengthscales")
        self._scales = self._scales_at(self._hps, x_data.shape[1])
        self._ordering_rule = (ordering if isinstance(ordering, str) else "given", seed)
        self._set_data(x_data, y_data, noise_variances, *self._ordering_of(ordering, x_data))
        self._search_all()

    # ---- state -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_dim(x_data):
        if x_data.shape[1] > 16:
            raise NotImplementedError("the device kernels take input dimension <= 16")

    def _check_hps(self, hps, d=None):
        hps = np.array(hps, dtype=np.float64)
        d = self.index_set_dim if d is None else d
        assert hps.shape == (self._native.n_hyperparameters(d),), "wrong number of hyperparameters for this kernel"
        return hps

    def _scales_at(self, hps, d):
        mode = self._scale_mode
        if isinstance(mode, str):
            if mode == "lengthscales":
                return np.array(self._native.length_scales(hps, d), dtype=np.float64)
            if mode == "unit":
                return None
            raise ValueError(f"args['neighbor_scales'] must be 'lengthscales', 'unit' or a vector of {d} positive numbers, got {mode!r}")
        sc = np.array(mode, dtype=np.float64)
        if sc.shape != (d,) or not np.all(sc > 0.0) or not np.all(np.isfinite(sc)):
            raise ValueError(f"args['neighbor_scales'] must be 'lengthscales', 'unit' or a vector of {d} positive numbers")
        return sc

    @staticmethod
    def _make_ordering(ordering, n, seed):
        if isinstance(ordering, str):
            if ordering == "random":
                return np.random.default_rng(seed).permutation(n).astype(np.int64)
            if ordering == "given":
                return np.arange(n, dtype=np.int64)
            raise ValueError(f"ordering must be 'random', 'given', 'maxmin' or a permutation of range({n}), got {ordering!r}")
        perm = np.array(ordering, dtype=np.int64)
        if perm.shape != (n,) or not np.array_equal(np.sort(perm), np.arange(n)):
            raise ValueError(f"ordering must be 'random', 'given', 'maxmin' or a permutation of range({n})")
        return perm

    def _maxmin(self, x_data):
        """(perm, entry distances): the maxmin ordering of x_data under the object's scales from first_point's point, its first
        args["maxmin_points"] positions by the device (fvgp_hip_nn_maxmin_order), the points left over behind them in a random order"""
        x = np.ascontiguousarray(x_data, dtype=np.float64)
        n = len(x)
        if not np.all(np.isfinite(x)):
            raise ValueError("ordering='maxmin' needs finite coordinates in x_data")
        q = self.args.get("maxmin_points")
        q = n if q is None else q
        if isinstance(q, bool) or int(q) != q or not 1 <= int(q) <= n:
            raise ValueError(f"args['maxmin_points'] must be None or an integer in 1 .. {n} (the number of data points), got {q!r}")
        q = int(q)
        head, dist2 = self._H.nn_maxmin_order(self._H.to_device(x), first_point(x, self._scales), q, scales=self._scales)
        rest = np.setdiff1d(np.arange(n, dtype=np.int64), head)
        rest = rest[np.random.default_rng(self._ordering_rule[1]).permutation(len(rest))]
        return np.concatenate([head, rest]), np.concatenate([np.sqrt(dist2), np.full(n - q, np.nan)])

    def _ordering_of(self, ordering, x_data):
        """(perm, entry distances or None) of x_data by `ordering`: a rule's name or a permutation"""
        if isinstance(ordering, str) and ordering == "maxmin":
            return self._maxmin(x_data)
        return self._make_ordering(ordering, len(x_data), self._ordering_rule[1]), None

    def _set_data(self, x_data, y_data, noise_variances, perm, distances=None):
        """the caller's arrays as they came, and on the device in the ordering `perm` (position p holds the caller's row perm[p]);
        `distances`: what ordering_distances becomes"""
        H = self._H
        self._check_dim(x_data)
        self.x_data = np.ascontiguousarray(x_data, dtype=np.float64)
        self.y_data = np.ascontiguousarray(y_data, dtype=np.float64)
        self.point_number, self.index_set_dim = self.x_data.shape
        if noise_variances is None:
            V = np.ones(self.point_number) * (np.mean(abs(self.y_data)) / 100.0) ** 2
        else:
            V = np.asarray(noise_variances, dtype=np.float64)
            assert V.shape == (self.point_number,), "noise_variances must be 1-d, one per data point"
            assert np.all(V > 0.0), "all noise_variances must be positive"
        self.noise_variances = noise_variances
        self._V = np.ascontiguousarray(V)
        self._m = float(np.mean(self.y_data))
        self.ordering = perm
        self.ordering_distances = distances
        self._x_dev = H.to_device(self.x_data[perm])
        self._grid = None                          # (of the rows that were: _build_grid makes the new one)
        self._V_dev = H.to_device(self._V[perm])
        self._r_dev = H.to_device((self.y_data - self._m)[perm])

    def _search_route(self):
        """"brute" or "grid": args["neighbor_search"] resolved for the data as they are"""
        mode = self.args.get("neighbor_search", NEIGHBOR_SEARCH_DEFAULT)
        if mode not in ("brute", "grid", "auto"):
            raise ValueError(f"args['neighbor_search'] must be 'brute', 'grid' or 'auto', got {mode!r}")
        fits = self.index_set_dim <= _lib.NN_GRID_MAX_DIM
        if mode == "grid" and not fits:
            raise ValueError(f"args['neighbor_search'] = 'grid' takes input dimension <= {_lib.NN_GRID_MAX_DIM}, got "
                             f"{self.index_set_dim}: use 'brute', or 'auto', which takes the brute search there")
        if mode == "auto":
            return "grid" if fits and self.point_number >= NEIGHBOR_SEARCH_AUTO_POINTS else "brute"
        return mode

    def _build_grid(self):
        """the cell grid over the ordered data under the object's scales (None on the brute route): made again whenever the data, the
        ordering or the scales change, kept for prediction and appends"""
        self._grid = self._H.nn_grid_build(self._x_dev, self._scales) if self._search_route() == "grid" else None

    def _search(self, xq_dev, c0):
        """int32 (nq, m) device tensor: the neighbours of the rows of xq_dev among the ordered data under the object's scales, by the
        grid where there is one (the same lists element for element)"""
        H = self._H
        idx = H.torch.empty((xq_dev.shape[0], self.n_neighbors), dtype=H.torch.int32, device=xq_dev.device)
        if self._grid is not None:
            H.nn_grid_search(xq_dev, self._x_dev, self.n_neighbors, idx, self._grid, c0=c0)
        else:
            H.nn_search(xq_dev, self._x_dev, self.n_neighbors, idx, scales=self._scales, c0=c0)
        return idx

    def _search_all(self):
        self._build_grid()
        self._idx = self._search(self._x_dev, 0)

    @property
    def hyperparameters(self):
        return self._hps

    def get_hyperparameters(self):
        return self._hps

    def set_hyperparameters(self, hps):
        """new hyperparameters; the neighbour lists stay as they are (refresh_neighbors rebuilds them)"""
        self._hps = self._check_hps(hps)

    def refresh_neighbors(self, hyperparameters=None, reorder=False):
        """rebuild the neighbour lists: under the length scales of `hyperparameters` (default: the current ones) where
        args["neighbor_scales"] is "lengthscales", else under the same scales as before.  reorder=True (ordering="maxmin" only): the
        ordering is made again under those scales first and the data are uploaded in it"""
        if reorder and self._ordering_rule[0] != "maxmin":
            raise ValueError(f"refresh_neighbors(reorder=True) recomputes a maxmin ordering: this object's ordering rule is "
                             f"{self._ordering_rule[0]!r}, which does not depend on the scales")
        hps = self._hps if hyperparameters is None else self._check_hps(hyperparameters)
        self._scales = self._scales_at(hps, self.index_set_dim)
        if reorder:
            self._set_data(self.x_data, self.y_data, self.noise_variances, *self._maxmin(self.x_data))
        self._search_all()

    def neighbors(self):
        """(N, m) int64: row i lists the neighbours of the caller's data point i as the caller's indices, nearest first, -1 where the
        ordering leaves fewer than m earlier points"""
        idx = self._idx.cpu().numpy().astype(np.int64)
        out = np.full_like(idx, -1)
        out[self.ordering] = np.where(idx >= 0, self.ordering[np.clip(idx, 0, None)], -1)
        return out

    def _unorder(self, a):
        """per-point values in the ordering (first axis) -> the caller's order"""
        out = np.empty_like(a)
        out[self.ordering] = a
        return out

    def _not_pd(self, info, nq, what, points=None):
        b, row = divmod(int(info) - 1, nq)
        where = f"data point {int(self.ordering[row])}" if points is None else f"prediction point {row}"
        return NonPositiveDefiniteError(
            f"{what}: the conditional of {where} (hyperparameter vector {b}) is not positive definite in double precision -- its "
            f"{self.n_neighbors} x {self.n_neighbors} neighbour block K + V or its conditional variance has a pivot that is not positive; "
            "duplicated points need positive noise, or rethink the hyperparameters")

    # ---- the likelihood, its gradient and its Fisher information: one evaluation at three levels -----------------------------------
    def _evaluate(self, thetas, level):
        """one device call at the rows of thetas (B, H), as far as `level` (_lib.NN_VALUE, NN_GRAD, NN_FISHER): out (B, 3), grad (B, H) =
        d log p / d theta, fisher (B, H, H), info, and on the device mu, var (B, n), score (B, n, H), rows (B, n, H (H + 1) / 2); None
        where the level has none"""
        H, n = self._H, self.point_number
        B, nth = thetas.shape
        mu, var = H.empty(B, n), H.empty(B, n)
        score = H.torch.empty((B, n, nth), dtype=H.torch.float64, device=mu.device) if level >= _lib.NN_GRAD else None
        rows = H.torch.empty((B, n, nth * (nth + 1) // 2), dtype=H.torch.float64, device=mu.device) if level == _lib.NN_FISHER else None
        out, grad, fisher, info = H._nn_likelihood(level, self._native.kernel_id, self._x_dev, thetas, self._idx, self.n_neighbors,
                                                   self._r_dev, self._V_dev, mu, var, score, rows, None)
        return _Evaluation(out, grad, fisher, info, mu, var, score, rows)

    def _one(self, hyperparameters):
        hps = self._hps if hyperparameters is None else self._check_hps(hyperparameters)
        return hps.reshape(1, -1)

    def _at(self, hyperparameters, level, what):
        """_evaluate at the object's hyperparameters or at `hyperparameters`; `what` names the caller where a conditional fails"""
        ev = self._evaluate(self._one(hyperparameters), level)
        if ev.info:
            raise self._not_pd(ev.info, self.point_number, what)
        return ev

    def _chunk(self, level, nth):
        """hyperparameter vectors per device call: 4096 for the value; with the gradient or the Fisher information, as many as keep the
        call's per-row outputs (mu, var, score, fisher_rows) under args["grad_batch_bytes"]"""
        if level == _lib.NN_VALUE:
            return 4096
        per_row = 2 + nth + (nth * (nth + 1) // 2 if level == _lib.NN_FISHER else 0)
        cap = int(self.args.get("grad_batch_bytes", 1 << 30))
        return int(max(1, min(65535, cap // (8 * self.point_number * per_row))))

    def _grad_chunk(self, nth):
        return self._chunk(_lib.NN_GRAD, nth)

    def _fisher_chunk(self, nth):
        return self._chunk(_lib.NN_FISHER, nth)

    def _batch(self, thetas, level):
        """(log p (B,), G (B, H) = -d log p / d theta, F (B, H, H)) at the B rows of `thetas`, in chunks of _chunk; None where the level
        has none, NaN all three where a conditional is not positive definite"""
        thetas = np.ascontiguousarray(np.asarray(thetas, dtype=np.float64))
        assert thetas.ndim == 2 and thetas.shape[1] == len(self._hps), "thetas must be (B, number of hyperparameters)"
        B, nth = thetas.shape
        lp = np.empty(B)
        G = np.empty((B, nth)) if level >= _lib.NN_GRAD else None
        F = np.empty((B, nth, nth)) if level == _lib.NN_FISHER else None
        step = self._chunk(level, nth)
        for a in range(0, B, step):
            ev = self._evaluate(thetas[a:a + step], level)
            lp[a:a + step] = ev.out[:, 0]
            if G is not None:
                G[a:a + step] = -ev.grad
            if F is not None:
                F[a:a + step] = ev.fisher
        for A in (G, F):
            if A is not None:
                A[np.isnan(lp)] = np.nan
        return lp, G, F

    def log_likelihood(self, hyperparameters=None):
        """the nearest-neighbour log marginal likelihood at the object's hyperparameters or at `hyperparameters`: deterministic, the
        same bits on every call"""
        return float(self._at(hyperparameters, _lib.NN_VALUE, "log_likelihood").out[0, 0])

    def neg_log_likelihood(self, hyperparameters=None):
        return -self.log_likelihood(hyperparameters)

    def log_likelihood_batch(self, thetas):
        """(B,): the log-likelihood at the B rows of `thetas` in one device call, each equal bit for bit to log_likelihood(thetas[b]);
        NaN where a conditional is not positive definite"""
        return self._batch(thetas, _lib.NN_VALUE)[0]

    def neg_log_likelihood_batch(self, thetas):
        """-log_likelihood_batch with +inf where it is NaN (what a population optimiser wants to see)"""
        f = -self.log_likelihood_batch(thetas)
        return np.where(np.isnan(f), np.inf, f)

    def conditionals(self, hyperparameters=None):
        """{"mean", "variance", "log_predictive"} (N,) each, in the caller's order: every data point's conditional given its neighbours,
        the factors of the likelihood (their log_predictive sum to it up to rounding) and the approximation's residual diagnostics"""
        ev = self._at(hyperparameters, _lib.NN_VALUE, "conditionals")
        mu, var = self._H.to_host(ev.mu)[0], self._H.to_host(ev.var)[0]
        r = (self.y_data - self._m)[self.ordering]
        lp = -0.5 * ((r - mu) ** 2 / var + np.log(var) + _LOG_2PI)
        return {"mean": self._unorder(self._m + mu), "variance": self._unorder(var), "log_predictive": self._unorder(lp)}

    def neg_log_likelihood_and_gradient(self, hyperparameters=None):
        """(f, g (H,)): the negative nearest-neighbour log-likelihood and its exact gradient from one device call; deterministic, the
        same bits on every call"""
        ev = self._at(hyperparameters, _lib.NN_GRAD, "neg_log_likelihood_and_gradient")
        return -float(ev.out[0, 0]), -ev.grad[0]

    def neg_log_likelihood_and_gradient_batch(self, thetas):
        """(f (B,), G (B, H)) at the B rows of `thetas`, each row equal bit for bit to neg_log_likelihood_and_gradient(thetas[b]); the
        batch goes in chunks whose per-row outputs fit args["grad_batch_bytes"].  Where a conditional is not positive definite the value
        is +inf and the gradient NaN."""
        lp, G, _ = self._batch(thetas, _lib.NN_GRAD)
        return np.where(np.isnan(lp), np.inf, -lp), G

    def neg_log_likelihood_gradient_batch(self, thetas):
        return self.neg_log_likelihood_and_gradient_batch(thetas)[1]

    def conditional_scores(self, hyperparameters=None):
        """(N, H), in the caller's order: row i is d log p(y_i | its neighbours) / d theta, the per-point terms that sum to the gradient
        of log_likelihood (diagnostics, and the raw material of minibatch methods)"""
        return self._unorder(self._at(hyperparameters, _lib.NN_GRAD, "conditional_scores").score[0].cpu().numpy())

    def neg_log_likelihood_gradient_and_fisher(self, hyperparameters=None):
        """(f, g (H,), F (H, H)) from one device call: the negative nearest-neighbour log-likelihood, its exact gradient and the Fisher
        information of the approximation -- the EXPECTED Hessian of f under the exact GP at these hyperparameters, positive semidefinite
        by construction, for about the cost of a second gradient"""
        ev = self._at(hyperparameters, _lib.NN_FISHER, "neg_log_likelihood_gradient_and_fisher")
        return -float(ev.out[0, 0]), -ev.grad[0], ev.fisher[0]

    def fisher_information(self, hyperparameters=None):
        """(H, H): the Fisher information of the nearest-neighbour likelihood; its inverse is the asymptotic covariance of the
        maximum-likelihood hyperparameters"""
        return self.neg_log_likelihood_gradient_and_fisher(hyperparameters)[2]

    def neg_log_likelihood_gradient_and_fisher_batch(self, thetas):
        """(f (B,), G (B, H), F (B, H, H)) at the B rows of `thetas`, each row equal bit for bit to
        neg_log_likelihood_gradient_and_fisher(thetas[b]); the batch goes in chunks whose per-row outputs fit args["grad_batch_bytes"].
        Where a conditional is not positive definite the value is +inf, the gradient and the Fisher matrix NaN."""
        lp, G, F = self._batch(thetas, _lib.NN_FISHER)
        return np.where(np.isnan(lp), np.inf, -lp), G, F

    def conditional_fisher(self, hyperparameters=None):
        """(N, H, H), in the caller's order: entry i is data point i's term of the Fisher information, E[-d^2 log p(y_i | its
        neighbours)]; positive semidefinite each, they sum to fisher_information"""
        packed = self._at(hyperparameters, _lib.NN_FISHER, "conditional_fisher").rows[0].cpu().numpy()
        h, k = np.tril_indices(len(self._hps))            # the packed lower triangle: (h, k <= h) at h (h + 1) / 2 + k
        full = np.empty((self.point_number, len(self._hps), len(self._hps)))
        full[:, h, k] = full[:, k, h] = packed
        return self._unorder(full)

    def hyperparameter_laplace(self, hyperparameters=None, n_samples=0, seed=0, bounds=None):
        """gp_hessian.laplace_from_hessian at `hyperparameters` (None: the current, trained ones) with the Fisher information in the
        Hessian's place: N(theta, F^-1), the asymptotic distribution of the maximum-likelihood estimate.  The curvature is the EXPECTED
        one (the Fisher information of the nearest-neighbour likelihood), not the observed Hessian the dense GP's method of this name
        uses: the two agree as N grows, and "log_evidence" is the Laplace formula with F for H.  Returns that function's dictionary
        ("mean", "hessian" = F, "covariance", "log_evidence", "samples" (n_samples, H) inside `bounds`) plus "fisher" and "std_error" =
        sqrt(diag F^-1).  Raises ValueError where F is not positive definite (a hyperparameter the data do not determine)."""
        from .gp_hessian import laplace_from_hessian
        hps = self._hps if hyperparameters is None else self._check_hps(hyperparameters)
        f, _, fisher = self.neg_log_likelihood_gradient_and_fisher(hps)
        out = laplace_from_hessian(hps, f, fisher, n_samples=n_samples, seed=seed, bounds=bounds)
        out["fisher"] = fisher
        out["std_error"] = np.sqrt(np.diag(out["covariance"]))
        return out

    # ---- prediction ----------------------------------------------------------------------------------------------------------
    def _check_pred(self, x_pred, x_out=None):
        if x_out is not None:
            raise NotImplementedError("x_out / fvGP outputs are not on the nearest-neighbour path: " + _DENSE)
        assert isinstance(x_pred, np.ndarray) and np.ndim(x_pred) == 2, "x_pred must be a 2-d np.ndarray"
        assert x_pred.shape[1] == self.index_set_dim, "wrong number of columns in x_pred"
        return self._H.to_device(x_pred)

    def _predict(self, x_pred, hyperparameters, x_out, s=None, what="posterior_mean"):
        H = self._H
        xp = self._check_pred(x_pred, x_out)
        P = xp.shape[0]
        idx = self._search(xp, -1)
        mu, var = H.empty(1, P), H.empty(1, P)
        info = H.nn_conditionals(self._native.kernel_id, xp, self._x_dev, self._one(hyperparameters), idx, self.n_neighbors,
                                 self._r_dev, self._V_dev, mu, var, s=None if s is None else H.to_device(s))
        if info:
            raise self._not_pd(info, P, what, points=x_pred)
        return H.to_host(mu)[0], H.to_host(var)[0]

    def posterior_mean(self, x_pred, hyperparameters=None, x_out=None):
        """{"x", "m(x)"}: the mean at every row of x_pred given its n_neighbors nearest data points"""
        mu, _ = self._predict(x_pred, hyperparameters, x_out)
        mean = self._m + mu
        return {"x": x_pred.copy(), "m(x)": mean, "m(x)_flat": mean, "x_pred": x_pred}

    def posterior_covariance(self, x_pred, variance_only=True, add_noise=False, hyperparameters=None, x_out=None):
        """{"x", "v(x)"}: the variance at every row of x_pred given its n_neighbors nearest data points; add_noise adds the data's
        noise (point for point when x_pred has as many rows as the data, else its mean)"""
        if not variance_only:
            raise NotImplementedError("posterior_covariance(variance_only=False): the nearest-neighbour approximation conditions every "
                                      "point on its own neighbours and defines no joint covariance; MatrixFreeGP (all the data, matrix-free) "
                                      "and the dense fvgp_amd.GP have it")
        s = None
        if add_noise:
            s = self._V.copy() if len(x_pred) == self.point_number else np.zeros(len(x_pred)) + np.mean(self._V)
        _, v = self._predict(x_pred, hyperparameters, x_out, s=s, what="posterior_covariance")
        if np.any(v < -0.0001):
            warnings.warn("Negative variances encountered. That normally means that the model is unstable. "
                          "Rethink the kernel definition, add more noise to the data, "
                          "or double check the hyperparameter optimization bounds. This will not "
                          "terminate the algorithm, but expect anomalies.")
        v = np.where(v < 0.0, 0.0, v)
        return {"x": x_pred.copy(), "x_pred": x_pred, "v(x)": v, "v_flat": v, "S": None}

    # ---- data ------------------------------------------------------------------------------------------------------------------
    def update_gp_data(self, x_new, y_new, noise_variances_new=None, append=True):
        """append=True: the new points go to the END of the ordering and only their neighbours are searched (the old rows' lists stay:
        the state equals a fresh object with the same ordering and the new rows last; their ordering_distances are nan); the prior mean
        is recomputed.  append=False replaces everything (the ordering is made again by the constructor's rule, "maxmin" runs on the
        new data; a permutation array there: the caller's order)."""
        assert isinstance(x_new, np.ndarray) and np.ndim(x_new) == 2 and isinstance(y_new, np.ndarray) and np.ndim(y_new) == 1
        assert x_new.shape[1] == self.index_set_dim and len(x_new) == len(y_new), "x_new / y_new do not fit the data"
        if not append:
            self._set_data(x_new, y_new, noise_variances_new, *self._ordering_of(self._ordering_rule[0], x_new))
            self._search_all()
            return
        if (self.noise_variances is None) != (noise_variances_new is None):
            raise Exception("noise_variances_new must be given exactly when the object was built with noise_variances")
        n_old, k = self.point_number, len(x_new)
        if k == 0:
            return
        old_idx = self._idx
        x_all, y_all = np.vstack([self.x_data, x_new]), np.concatenate([self.y_data, y_new])
        v_all = None if noise_variances_new is None else np.concatenate([self.noise_variances, noise_variances_new])
        dist = None if self.ordering_distances is None else np.concatenate([self.ordering_distances, np.full(k, np.nan)])
        self._set_data(x_all, y_all, v_all, np.concatenate([self.ordering, n_old + np.arange(k, dtype=np.int64)]), dist)
        self._build_grid()
        self._idx = self._H.torch.cat([old_idx, self._search(self._x_dev[n_old:], n_old)], dim=0)

    # ---- the exact answer beside the approximation ------------------------------------------------------------------------------------
    def matrix_free(self, args=None):
        """A MatrixFreeGP over the same data, kernel and CURRENT hyperparameters whose conjugate gradients are preconditioned by this
        object's own factor (args["preconditioner"] = "vecchia"): it shares this object's ordering, ordered device arrays and
        neighbour lists -- no second search -- and solves with the exact K + V.  args: MatrixFreeGP's other ones ("tol", "max_iter", ..)."""
        from .gp_matrix_free import MatrixFreeGP
        args = dict(args or {})
        if args.setdefault("preconditioner", "vecchia") != "vecchia":
            raise ValueError("VecchiaGP.matrix_free preconditions with this object's factor: args['preconditioner'] is 'vecchia' here; "
                             "MatrixFreeGP(...) itself takes 'pchol'")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")       # (the noise rule's warning was given when this object was built)
            return MatrixFreeGP(self.x_data, self.y_data, self._hps.copy(), noise_variances=self.noise_variances, kernel_function=self._native,
                                args=args, _vecchia=self)

    # ---- training ----------------------------------------------------------------------------------------------------------------
    def neg_log_likelihood_gradient(self, hyperparameters=None, component=0):
        """with args={"likelihood_gradient": True}: the exact gradient (H,) of neg_log_likelihood"""
        if not self.likelihood_gradient:
            raise NotImplementedError("neg_log_likelihood_gradient: under this fvgp.GP name the exact gradient of the nearest-neighbour "
                                      "likelihood is not built yet -- the name answers only with args={'likelihood_gradient': True}; "
                                      "neg_log_likelihood_and_gradient, conditional_scores and train_gradient are always there")
        return self.neg_log_likelihood_and_gradient(hyperparameters)[1]

    def train_gradient(self, hyperparameter_bounds, init_hyperparameters=None, method="local", local_optimizer="L-BFGS-B", max_iter=200,
                       tolerance=1e-4, lr=1e-2, info=False, seed=None):
        """Training on the exact gradient, the neighbour lists fixed throughout.  "local": gp_training.train's scipy route with this
        object's value and gradient as the objective (one device call serves both).  "adam": gp_training.adam_optimize with every iterate
        clipped into the bounds; with args["adam_starts"] = S >= 2, S trajectories in lockstep (adam_optimize_batch) on the batched value
        and gradient, the first from init_hyperparameters, the others uniform in the bounds from `seed`, the best end point kept
        (adam_multistart_info).  adam_history keeps the iterates.  "fisher": projected Fisher scoring (fisher_scoring.fisher_scoring) on
        neg_log_likelihood_gradient_and_fisher: Newton-type steps with the Fisher information as the curvature, a backtracking line
        search inside the bounds, every trial point one device call; a trial at which a conditional is not positive definite counts as
        +inf.  It stops when the decrement -g^T step falls below `tolerance`; fisher_history keeps the iterates as (theta, f, decrement,
        step length) and fisher_evaluations the number of device calls.  Ends with set_hyperparameters(theta) and returns theta."""
        if method not in ("local", "adam", "fisher"):
            raise ValueError(f"train_gradient: method must be 'local' or 'adam', or 'fisher' for Fisher scoring, got {method!r}")
        bounds = np.asarray(hyperparameter_bounds, dtype=np.float64)
        assert bounds.ndim == 2 and bounds.shape == (len(self._hps), 2), "wrong bounds format"
        theta0 = np.array(self._hps if init_hyperparameters is None else init_hyperparameters, dtype=np.float64)
        if np.any(theta0 < bounds[:, 0]) or np.any(theta0 > bounds[:, 1]):
            raise Exception("Starting positions outside of optimization bounds.", theta0, bounds)
        last = {}

        def evaluate(theta):
            key = np.asarray(theta, dtype=np.float64).tobytes()
            if last.get("key") != key:
                last["key"], last["value"] = key, self.neg_log_likelihood_and_gradient(np.asarray(theta, dtype=np.float64))
            return last["value"]

        clip = lambda t: np.clip(t, bounds[:, 0], bounds[:, 1])      # noqa: E731
        starts = int(self.args.get("adam_starts", 0) or 0)
        if method == "fisher":
            def evaluate3(theta):
                f, G, F = self.neg_log_likelihood_gradient_and_fisher_batch(theta.reshape(1, -1))
                return float(f[0]), G[0], F[0]

            progress = None
            if info:
                def progress(theta, fval, decrement, iteration):
                    print(f"fvGP fisher scoring iteration {iteration} out of {max_iter}: f(x)= {float(fval)}, decrement= {float(decrement)}")
            hps, self.fisher_history, self.fisher_evaluations = _fisher.fisher_scoring(evaluate3, theta0, bounds, max_iter=max_iter,
                                                                                      tolerance=tolerance, callback=progress)
        elif method == "local":
            hps = _training.train(self, bounds, theta0, method="local", tolerance=tolerance, max_iter=max_iter,
                                  local_optimizer=local_optimizer, info=info, objective_function=lambda t: evaluate(t)[0],
                                  objective_function_gradient=lambda t: evaluate(t)[1])
        elif starts >= 2:
            x0 = _training.adam_start_points(theta0, bounds, starts, seed)

            def project(thetas, idx, fvals, grads, iteration):                # (the callback sees the optimiser's own array, after the step)
                thetas[idx] = clip(thetas[idx])

            xs, histories = _training.adam_optimize_batch(self.neg_log_likelihood_and_gradient_batch, x0, lr=lr, max_iter=max_iter,
                                                          tol=tolerance, callback=project)
            fx = self.neg_log_likelihood_batch(xs)
            best = int(np.argmin(fx))
            self.adam_history = histories[best]
            self.adam_multistart_info = {"x0": x0, "x": xs, "f(x)": fx, "best": best}
            hps = xs[best].copy()
        else:
            progress = None
            if info:
                def progress(theta, fval, grad, iteration):
                    if iteration % 10 == 0 or iteration == 1:
                        print(f"fvGP adam iteration {iteration} out of {max_iter}: f(x)= {float(fval)}, |grad|= {float(np.linalg.norm(grad))}")
            hps, self.adam_history = _training.adam_optimize(lambda t: evaluate(t)[0], lambda t: evaluate(t)[1], theta0, lr=lr,
                                                             max_iter=max_iter, tol=tolerance, callback=progress, project=clip)
        self.set_hyperparameters(hps)
        return hps

    def train(self, hyperparameter_bounds, init_hyperparameters=None, method="mcmc", pop_size=20, tolerance=1e-4, max_iter=1000,
              info=False, seed=None, constraints=(), mcmc_prior=None, mcmc_args=None, mcmc_prop_distrs="normal"):
        """gp_training.train on the deterministic likelihood with the value-only methods: "mcmc" (default), "global" (a generation of
        the population in one device call unless args["batch_population"] is False) or a callable; with
        args={"likelihood_gradient": True} also "local", "adam" and "fisher", which run train_gradient.  The neighbour lists stay fixed
        throughout.  Ends with set_hyperparameters(theta) and returns theta."""
        if method in ("local", "adam", "fisher") and self.likelihood_gradient:
            return self.train_gradient(hyperparameter_bounds, init_hyperparameters, method=method, tolerance=tolerance, max_iter=max_iter,
                                       info=info, seed=seed)
        if method in ("hgdl", "bo"):
            raise NotImplementedError(f"train(method={method!r}) needs HGDL / the BO surrogate loop; under this name the exact gradient of "
                                      "the nearest-neighbour likelihood is not built yet for them: 'mcmc', 'global', a callable, and with "
                                      "args={'likelihood_gradient': True} 'local' and 'adam' run here")
        if method in ("local", "adam", "fisher"):
            raise NotImplementedError(f"train(method={method!r}) needs a gradient, and under this fvgp.GP name the exact gradient of the "
                                      "nearest-neighbour likelihood is not built yet -- it answers only with "
                                      "args={'likelihood_gradient': True}; train_gradient(bounds, method='local' | 'adam' | 'fisher') is always there")
        bounds = np.asarray(hyperparameter_bounds, dtype=np.float64)
        assert bounds.ndim == 2 and bounds.shape == (len(self._hps), 2), "wrong bounds format"
        theta0 = np.array(self._hps if init_hyperparameters is None else init_hyperparameters, dtype=np.float64)
        hps = _training.train(self, bounds, theta0, method=method, pop_size=pop_size, tolerance=tolerance, max_iter=max_iter,
                              constraints=constraints, info=info, seed=seed, mcmc_prior=mcmc_prior, mcmc_args=mcmc_args,
                              mcmc_prop_distrs=mcmc_prop_distrs)
        self.set_hyperparameters(hps)
        return hps


class VecchiaMixin:
    """Mixed into fvgp_amd.GP: needs _native, _hps, _sharded, _noise_callable, _mean_callable, x_data, y_data, noise_variances."""

    def vecchia(self, x_data=None, y_data=None, noise_variances=None, n_neighbors=32, **kw):
        """A VecchiaGP with this GP's kernel and CURRENT hyperparameters, over this GP's data or over MORE data than a dense factor can
        hold (x_data, y_data, noise_variances); kw: ordering, seed, args."""
        if self._native is None:
            raise NotImplementedError("vecchia evaluates the kernel on the device: a kernel callable stays with the dense GP "
                                      "(use one of the named kernels)")
        if self._noise_callable is not None or self._mean_callable is not None:
            raise NotImplementedError("vecchia takes noise variances as numbers and the default prior mean: noise and mean "
                                      "callables stay with the dense GP")
        if getattr(self, "_sharded", False):
            raise NotImplementedError("vecchia runs on one device: the row-sharded mode (args['process_group']) stays with the dense GP")
        if self.y_data.shape[1] != 1:
            raise NotImplementedError("vecchia takes one column of y (fvGP / x_out: the dense GP has it)")
        if (x_data is None) != (y_data is None):
            raise Exception("x_data and y_data come together")
        if x_data is None:
            x_data, y_data = self.x_data, self.y_data[:, 0]
            if noise_variances is None:
                noise_variances = self.noise_variances
        return VecchiaGP(x_data, y_data, self._hps.copy(), noise_variances=noise_variances, kernel_function=self._native,
                         n_neighbors=n_neighbors, **kw)
