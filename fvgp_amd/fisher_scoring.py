"""Projected Fisher scoring: a bounded second-order minimiser for an objective that comes with its gradient and a positive semidefinite
curvature (the Fisher information of a likelihood) from ONE evaluation.  VecchiaGP.train_gradient(method="fisher") runs it on
fvgp_hip_nn_loglik_fisher; it knows nothing of the device.

Per iteration, at theta with (f, g, F):
    free set    every component not pinned at a bound by an outward-pointing gradient (theta_h at its lower bound with g_h > 0, or at its
                upper bound with g_h < 0)
    step        -(F + lam diag F)^-1 g on the free set, 0 elsewhere; lam starts at 0 and rises (1e-3, then tenfold) only when the solve
                fails or no step length is accepted, and falls tenfold after every accepted step
    stop        when the decrement -g^T step is below `tolerance`, or at max_iter
    line search theta_new = clip(theta + alpha step) into the bounds, alpha = 1, 1/2, ..: the first with a finite f_new <= f + 1e-4 g^T
                (theta_new - theta) is taken (an objective of +inf -- a conditional that is not positive definite -- is a rejected trial,
                not an error)
Every trial point is one evaluation, and the accepted trial's (f, g, F) are the next iteration's: nothing is evaluated twice."""
import numpy as np

ARMIJO = 1e-4
MAX_HALVINGS = 30
LAMBDA_MAX = 1e8


def _step(g, F, free, lam):
    """(-(F + lam diag F)^-1 g on the free set and 0 elsewhere, the decrement -g^T step), or None where the matrix is not positive
    definite or the step is not a finite descent direction"""
    Ff = F[np.ix_(free, free)]
    A = Ff + lam * np.diag(np.diag(Ff))
    try:
        L = np.linalg.cholesky(0.5 * (A + A.T))
    except np.linalg.LinAlgError:
        return None
    sf = -np.linalg.solve(L.T, np.linalg.solve(L, g[free]))
    dec = -float(g[free] @ sf)
    if not np.all(np.isfinite(sf)) or not dec >= 0.0:
        return None
    step = np.zeros(len(g))
    step[free] = sf
    return step, dec


def fisher_scoring(evaluate, theta0, bounds, max_iter=200, tolerance=1e-4, callback=None):
    """Minimise over the box `bounds` (H, 2) from theta0.  evaluate(theta) -> (f, g (H,), F (H, H)); f may be +inf (g and F are then not
    read).  Returns (theta, history, evaluations): history is a list of (theta, f, decrement, step length), one entry per iterate --
    the step length that left it, 0.0 for the last.  callback(theta, f, decrement, iteration) is called once per iterate."""
    bounds = np.asarray(bounds, dtype=np.float64)
    lo, hi = bounds[:, 0], bounds[:, 1]
    theta = np.clip(np.asarray(theta0, dtype=np.float64), lo, hi)
    f, g, F = evaluate(theta)
    evaluations = 1
    if not np.isfinite(f):
        raise ValueError("fisher_scoring: the objective is not finite at the starting point")
    g, F = np.asarray(g, dtype=np.float64), np.asarray(F, dtype=np.float64)
    history, lam = [], 0.0
    for iteration in range(int(max_iter) + 1):
        free = np.nonzero(~(((theta <= lo) & (g > 0.0)) | ((theta >= hi) & (g < 0.0))))[0]
        accepted = None
        step, dec = np.zeros(len(theta)), 0.0
        while len(free) and lam <= LAMBDA_MAX:
            sd = _step(g, F, free, lam)
            if sd is not None:
                step, dec = sd
                if dec < tolerance or iteration == max_iter:
                    break
                alpha = 1.0
                for _ in range(MAX_HALVINGS):
                    trial = np.clip(theta + alpha * step, lo, hi)
                    if np.array_equal(trial, theta):               # (the bounds took the whole step: a shorter one fares no better)
                        break
                    ft, gt, Ft = evaluate(trial)
                    evaluations += 1
                    if np.isfinite(ft) and ft <= f + ARMIJO * float(g @ (trial - theta)):
                        accepted = (trial, float(ft), np.asarray(gt, dtype=np.float64), np.asarray(Ft, dtype=np.float64), alpha)
                        break
                    alpha *= 0.5
                if accepted is not None:
                    break
            lam = 1e-3 if lam == 0.0 else 10.0 * lam
        if callback is not None:
            callback(theta, f, dec, iteration)
        if accepted is None:
            history.append((theta.copy(), float(f), dec, 0.0))
            break
        history.append((theta.copy(), float(f), dec, accepted[4]))
        theta, f, g, F = accepted[:4]
        lam = lam / 10.0 if lam > 1e-3 else 0.0
    return theta, history, evaluations
