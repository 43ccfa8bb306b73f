"""The exact Hessian's third scratch square is scratch: it stays out of a pickled GP and follows the data when the GP grows."""
import pickle
import warnings

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _gp(n=None):
    import fvgp_amd
    fx = load_golden("G9_derivatives_rbf_n256_d2.npz")
    n = len(fx["x"]) if n is None else n
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(fx["x"][:n], fx["y"][:n], init_hyperparameters=fx["theta"], noise_variances=fx["noise_variances"][:n],
                         kernel_function="rbf_ard")
    return gp, fx


def test_pickle_after_an_exact_hessian_call_leaves_the_scratch_out():
    """train / Laplace / save: the pickled state holds none of the scratch squares, and the round trip reproduces the likelihood and
    the Hessian"""
    gp, fx = _gp()
    hess = gp.neg_log_likelihood_exact_hessian()
    assert gp._work3 is not None
    state = gp.__getstate__()
    for key in ("_work", "_work2", "_work3", "_alpha_work"):
        assert key not in state
    blob = pickle.dumps(gp)
    # the factor (n^2 doubles, lower triangle) and the data; a scratch square would add padded_dim(n)^2 doubles, another 0.5 MB here
    assert len(blob) < 256 * 256 * 8 + 200_000
    gp2 = pickle.loads(blob)
    assert gp2._work3 is None
    np.testing.assert_allclose(gp2.log_likelihood(), gp.log_likelihood(), rtol=1e-10)
    assert np.max(np.abs(gp2.neg_log_likelihood_exact_hessian() - hess)) <= 1e-12 * np.max(np.abs(hess))


def test_scratch_follows_the_data_after_an_append():
    """an exact call, then points appended across a tile boundary (200 -> 256, padded 256 -> 256 stays; 256 -> 300 grows to 384): the
    next exact call works on squares of the new size and agrees with a GP built on the union"""
    gp, fx = _gp(200)
    gp.neg_log_likelihood_exact_hessian()
    x, y, nv = fx["x"], fx["y"], fx["noise_variances"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.update_gp_data(x[200:], y[200:], noise_variances_new=nv[200:], append=True)
    whole, _ = _gp()
    got, ref = gp.neg_log_likelihood_exact_hessian(), whole.neg_log_likelihood_exact_hessian()
    assert gp._work3.shape[0] == gp._np
    assert np.max(np.abs(got - ref)) <= 1e-8 * np.max(np.abs(ref))
    rng = np.random.default_rng(5)
    xn = rng.random((44, 2))
    yn = np.sin(3.0 * xn.sum(axis=1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.update_gp_data(xn, yn, noise_variances_new=np.full(44, 0.01), append=True)
    h = gp.neg_log_likelihood_exact_hessian()
    assert gp._np == 384 and gp._work3.shape[0] == 384 and np.all(np.isfinite(h))
