"""What the GPU tests of the nearest-neighbour likelihood share (test_gpu_vecchia.py, test_gpu_vecchia_grad.py, test_gpu_vecchia_fisher.py,
test_gpu_vecchia_family.py):
canary-framed device outputs and the three likelihood entries of Handle called into them.  Each test file keeps its own H fixture."""
import numpy as np

import vecchia_ref as vr

CANARY = -7.25e300
VALUE, GRAD, FISHER = 0, 1, 2     # the entry: Handle.nn_loglik, nn_loglik_grad, nn_loglik_fisher


def _kid(kernel):
    from fvgp_amd import _lib
    return _lib.KERNEL_IDS[kernel]


def _framed(H, *shape):
    """a contiguous view of `shape` inside a canary-filled flat buffer: (buffer, view)"""
    size = int(np.prod(shape))
    big = H.torch.full((size + 16,), CANARY, dtype=H.torch.float64, device=f"cuda:{H.device}")
    return big, big[8:8 + size].view(*shape)


def _frame_untouched(big):
    a = big.cpu().numpy()
    return np.all(a[:8] == CANARY) and np.all(a[-8:] == CANARY)


def _same(a, b):
    """bit for bit, NaN in the same places"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _device(H, level, name, x, thetas, idx, m, r, v):
    """the likelihood entry of `level` into framed mu / var / score / fisher_rows, everything on the host:
    VALUE (out (B, 3), info, mu, var), GRAD (out, grad (B, H), info, mu, var, score (B, n, H)),
    FISHER (out, grad, fisher (B, H, H), info, mu, var, score, rows (B, n, P))"""
    thetas = np.atleast_2d(thetas)
    B, nth = thetas.shape
    n = len(x)
    shapes = [(B, n), (B, n), (B, n, nth), (B, n, nth * (nth + 1) // 2)][:2 + level]
    bigs, views = zip(*(_framed(H, *s) for s in shapes))
    # (a device tensor goes in as it is: a view with a leading dimension of its own)
    idx_d = idx if isinstance(idx, H.torch.Tensor) else H.torch.as_tensor(np.ascontiguousarray(idx), device=views[0].device)
    call = (H.nn_loglik, H.nn_loglik_grad, H.nn_loglik_fisher)[level]
    host = call(_kid(name), H.to_device(x), thetas, idx_d, m, H.to_device(r), H.to_device(v), *views)
    assert all(_frame_untouched(b) for b in bigs)
    if level == FISHER:
        assert not np.any(views[3].cpu().numpy() == CANARY), "every entry of fisher_rows is written"
    return (*host, *(a.cpu().numpy() for a in views))


def _device_value(H, name, x, thetas, idx, m, r, v):
    return _device(H, VALUE, name, x, thetas, idx, m, r, v)


def _device_grad(H, name, x, thetas, idx, m, r, v):
    return _device(H, GRAD, name, x, thetas, idx, m, r, v)


def _device_fisher(H, name, x, thetas, idx, m, r, v):
    return _device(H, FISHER, name, x, thetas, idx, m, r, v)


def _device_loglik(H, case, thetas=None):
    """_device_value on a case's inputs (the twin's neighbour lists), at the case's thetas or at `thetas`"""
    name, d, n, m, B = case
    x, th, r, v, idx = vr.case_inputs(case)
    return _device_value(H, name, x, th if thetas is None else thetas, idx, m, r, v)
