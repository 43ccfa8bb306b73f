"""A numpy twin of the greedy batch selection (fvgp_hip_select_batch, GP.select_batch) with the oracle's kernel functions (a helper
module of the tests, not a conftest), and the list of fixtures the GPU tests compare indices on.

With d the candidates' conditional latent variances, s their noise variances, KV = K + diag(V) over the data:

    step t:  score_i = d_i ("variance") or d_i / s_i ("information"); picked candidates do not score unless allow_repeats;
             j = the largest score, ties to the lowest index;  stop if d_j <= tol max_i d_i(initial) or nothing scores;
             r_i = k(x_i, x_j) - sum_n k(x_i, X_n) w_n,  w = KV^-1 k(X, x_j)                    (the alpha-form column)
             c_i = (r_i - sum_{s<t} G[s,i] G[s,j]) / sqrt(d_j + s_j);  G[t,i] = c_i;  d_i <- max(d_i - c_i^2, 0)

`brute_force_after` states what the result must equal: the posterior variance at every candidate once the picked points, with their
noise, are appended to the data."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import fvgp_oracle as orc

KERNELS = ["rbf_ard", "matern32_ard", "matern52_ard", "rbf_iso", "matern32_iso", "matern52_iso"]
SIGMA2 = 1.2


def initial_variances(kernel, x, theta, V, xc):
    """sigma^2 - k^T KV^-1 k at every candidate (unclipped), and the Cholesky factor object of KV"""
    kfun = orc.KERNELS[kernel]
    fac = cho_factor(orc.addKV(kfun(x, x, theta), V), lower=True)
    k = kfun(x, xc, theta)
    return theta[0] - np.sum(k * cho_solve(fac, k), axis=0), fac


def select_batch_ref(kernel, x, theta, V, xc, q, noise=None, criterion=0, allow_repeats=False, tol=1e-12, var0=None):
    """the twin.  Returns a dict: "indices" (q,) with -1 from the first exhausted step on, "pick_var" (q,) (0 there), "var" (P,) after the
    batch, "var0" (P,) the clipped initial variances, "G" (q, P) (zero rows from the first exhausted step on), "m" the number of picks,
    "exhausted", and "gaps" (m,): per step the absolute gap between the best and the second-best admissible score (inf if only one)."""
    kfun = orc.KERNELS[kernel]
    theta = np.asarray(theta, dtype=np.float64)
    P = len(xc)
    v0, fac = initial_variances(kernel, x, theta, V, xc)
    d = np.maximum(v0 if var0 is None else np.array(var0, dtype=np.float64), 0.0)
    out_var0 = d.copy()
    s = np.zeros(P) if noise is None else np.asarray(noise, dtype=np.float64)
    if criterion == 1:
        assert np.all(s > 0.0), "the information criterion needs noise > 0"
    Kcx = kfun(xc, x, theta)                                       # (P, n)
    dmax = float(np.max(d))
    G = np.zeros((q, P))
    idx, pick, gaps = np.full(q, -1, dtype=np.int64), np.zeros(q), []
    taken = np.zeros(P, dtype=bool)
    m = 0
    for t in range(q):
        score = d.copy() if criterion == 0 else d / s
        ok = np.ones(P, dtype=bool) if allow_repeats else ~taken
        ok &= score >= 0.0
        if not np.any(ok):
            break
        sc = np.where(ok, score, -np.inf)
        j = int(np.argmax(sc))                                     # the first of equal maxima: the lowest index
        if d[j] <= tol * dmax:
            break
        rest = np.delete(sc, j)
        gaps.append(float(sc[j] - np.max(rest)) if np.any(np.isfinite(rest)) else np.inf)
        idx[t], pick[t] = j, d[j]
        p = d[j] + s[j]
        w = cho_solve(fac, kfun(x, xc[j:j + 1], theta)[:, 0])
        r = kfun(xc, xc[j:j + 1], theta)[:, 0] - Kcx @ w
        c = (r - G[:t].T @ G[:t, j]) / np.sqrt(p)
        G[t] = c
        d = np.maximum(d - c * c, 0.0)
        taken[j] = True
        m += 1
    return {"indices": idx, "pick_var": pick, "var": d, "var0": out_var0, "G": G, "m": m, "exhausted": m < q, "gaps": np.array(gaps)}


def brute_force_after(kernel, x, theta, V, xc, picks, noise):
    """the latent posterior variance at every candidate with xc[picks], noise[picks] appended to the data (repeats included)"""
    picks = np.asarray(picks, dtype=np.int64)
    xa = np.vstack([x, xc[picks]])
    Va = np.concatenate([V, (np.zeros(len(xc)) if noise is None else np.asarray(noise, dtype=np.float64))[picks]])
    v, fac = initial_variances(kernel, xa, theta, Va, xc)
    return v, 2.0 * np.sum(np.log(np.diag(fac[0])))


def logdet_KV(kernel, x, theta, V):
    fac = cho_factor(orc.addKV(orc.KERNELS[kernel](x, x, theta), V), lower=True)
    return 2.0 * np.sum(np.log(np.diag(fac[0])))


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
# mode: "var0" criterion 0 without noise, "var" criterion 0 with noise, "info" criterion 1 (needs noise)
MODES = ("var0", "var", "info")


def make_case(kernel, n, d, P, seed, mode):
    """data x (n, d) with noise V in 0.01 .. 0.02, theta = [1.2, length scales], candidates xc (P, d), their noise (None for "var0").
    Length scales 0.3 .. 0.6, times 0.05 in one dimension and 0.5 in two: there 17 noise-free picks of a smooth kernel would otherwise
    bring every variance down to rounding, where no gap between two scores is left to compare indices on; and doubled for a single
    data point, which otherwise leaves most candidates at the prior variance, tied."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    V = rng.uniform(0.01, 0.02, n)
    scale = 2.0 if n == 1 else (0.05 if d == 1 else 0.5 if d == 2 else 1.0)
    theta = np.concatenate([[SIGMA2], scale * rng.uniform(0.3, 0.6, 1 if kernel.endswith("_iso") else d)])
    xc = rng.random((P, d))
    noise = None if mode == "var0" else (np.full(P, 0.05) if seed % 2 else rng.uniform(0.02, 0.2, P))
    return x, V, theta, xc, noise


def _abi_fixtures():
    """every (n, P) pair of the sizes at which the kernels take another path -- one, two and three 256-row slices, a partial last wave,
    the factor's padding edge; one candidate, a wave less one, a full wave, a wave and one, five waves with a ragged last one -- with q,
    the kernel, the dimension and the mode rotating through them so that each value meets each n and each P at least once; then every
    kernel in every dimension that has an instantiation of its own (1 .. 4) and one that takes the runtime dimension (5)."""
    out = []
    ns, Ps = (1, 127, 128, 129, 257, 513), (1, 63, 64, 65, 300)
    c = 0
    for a, n in enumerate(ns):
        for b, P in enumerate(Ps):
            q = (1, 5, min(P, 17))[(a + b) % 3]
            out.append({"kernel": KERNELS[(a + 2 * b) % 6], "n": n, "d": (1, 2, 3, 5)[(a + b) % 4], "P": P, "q": min(q, P),
                        "mode": MODES[(2 * a + b) % 3], "seed": 1000 + c})
            c += 1
    for kernel in KERNELS:
        for d in (1, 2, 3, 4, 5):
            out.append({"kernel": kernel, "n": 257, "d": d, "P": 65, "q": 5, "mode": MODES[(d + len(kernel)) % 3], "seed": 2000 + c})
            c += 1
    return out


ABI_FIXTURES = _abi_fixtures()
# the bitwise tests (repeatability, prefix, select_block, sub-list) and the facade tests
BITS_FIXTURE = {"kernel": "matern52_ard", "n": 257, "d": 2, "P": 300, "q": 12, "mode": "var", "seed": 3001}
FACADE_FIXTURE = {"kernel": "rbf_ard", "n": 200, "d": 2, "P": 300, "q": 12, "mode": "var", "seed": 3003}
ALL_FIXTURES = ABI_FIXTURES + [BITS_FIXTURE, FACADE_FIXTURE]


def fixture_id(fx):
    return f"{fx['kernel']}-n{fx['n']}-d{fx['d']}-P{fx['P']}-q{fx['q']}-{fx['mode']}"


def run_fixture(fx):
    """(inputs, twin result) of a fixture"""
    x, V, theta, xc, noise = make_case(fx["kernel"], fx["n"], fx["d"], fx["P"], fx["seed"], fx["mode"])
    ref = select_batch_ref(fx["kernel"], x, theta, V, xc, fx["q"], noise=noise, criterion=1 if fx["mode"] == "info" else 0)
    return (x, V, theta, xc, noise), ref


def fvgp_case(seed=3005, V=60, P=40, q=8, noise=0.05):
    """a two-task fvGP: (x_data (V, 2), y (V, 2), noise variances (V, 2), theta, candidates (P, 2), x_out) and the twin on the product
    set cartesian_product(candidates, x_out), over the task-major index set, with the scalar candidate noise"""
    rng = np.random.default_rng(seed)
    xd = rng.random((V, 2))
    y = np.stack([np.sin(3.0 * xd.sum(axis=1)), np.cos(2.0 * xd.sum(axis=1))], axis=1) + 0.1 * rng.standard_normal((V, 2))
    nv = rng.uniform(0.01, 0.02, (V, 2))
    theta = np.array([SIGMA2, 0.3, 0.4, 1.5])
    xq, x_out = rng.random((P, 2)), np.array([0.0, 1.0])
    xs, _, vs = orc.transform_index_set(xd, y, nv)
    xc = orc.cartesian_product(xq, x_out)
    ref = select_batch_ref("matern32_ard", xs, theta, vs, xc, q, noise=np.full(len(xc), noise))
    return (xd, y, nv, theta, xq, x_out, noise), xc, ref
