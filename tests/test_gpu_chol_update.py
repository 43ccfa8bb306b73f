"""fvgp_hip_chol_update / fvgp_hip_chol_delete through _lib.Handle against the numpy twin of the sweep (tests/chol_update_ref.py),
numpy.linalg.cholesky and scipy: values, what must not be touched (the strict upper triangle, the padding), repeatability, the bit
invariant of the header and the argument checks."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla

import chol_update_ref as cr

pytestmark = pytest.mark.gpu

TOL = 1e-11


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return B @ B.T + n * np.eye(n)


_FACTORS = {}


def _chol(n):
    if n not in _FACTORS:
        M = _spd(n, 100 + n)
        _FACTORS[n] = (M, np.linalg.cholesky(M))
    return _FACTORS[n]


def _factor_buffer(L, ld=None):
    """host image of a factor buffer: padded_dim(n) rows, NaN in the strict upper triangle (never to be read), identity padding"""
    from fvgp_amd._lib import pad128
    n = len(L)
    npad = pad128(n)
    ld = ld or npad
    buf = np.full((npad, ld), np.nan)
    buf[:n, :n] = np.tril(L) + np.triu(np.full((n, n), np.nan), 1)
    pad = np.eye(npad)[n:]
    pad[np.triu(np.ones_like(pad, dtype=bool), n + 1)] = np.nan
    buf[n:, :npad] = pad
    return buf


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def _w_cases(n, k):
    """(name, row0, W): dense from row0 = 0 / 128 / 130 where the size has such a row, and columns that start at different rows"""
    rng = np.random.default_rng(1000 * n + k)
    out = []
    for row0 in (0, 128, 130):
        if row0 < n or row0 == 0:
            W = rng.standard_normal((n, k))
            W[:row0] = 0.0
            out.append((f"row0={row0}", row0, W))
    W = rng.standard_normal((n, k))
    for p in range(k):
        W[:(37 * p) % n, p] = 0.0
    out.append(("staggered", 0, W))
    return out


@pytest.mark.parametrize("k", [1, 3, 16, 17, 33])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300, 512])
def test_chol_update(H, n, k):
    M, L = _chol(n)
    scale = np.max(np.abs(L))
    for name, row0, W in _w_cases(n, k):
        ref = np.linalg.cholesky(M + W @ W.T)
        twin = cr.chol_update(L, W, row0=row0)
        host = _factor_buffer(L)
        buf = H.to_device(host)
        H.chol_update(buf, n, H.to_device(W), row0=row0)
        H.sync()
        got = buf.cpu().numpy()
        Lg = np.tril(got[:n, :n])
        e_ref, e_twin = np.max(np.abs(Lg - ref)) / scale, np.max(np.abs(Lg - twin)) / scale
        print(f"chol_update|n={n}|k={k}|{name}|vs cholesky {e_ref:.3g}|vs twin {e_twin:.3g}")
        assert e_ref <= TOL and e_twin <= TOL, name
        # untouched: the strict upper triangle (still NaN), the padding rows, and with a row0 every column left of its block
        upper = np.triu(np.ones_like(host, dtype=bool), 1)
        assert _same_bits(got[upper], host[upper]) and _same_bits(got[n:], host[n:]), name
        c0 = row0 // 128 * 128
        assert _same_bits(np.tril(got[:n, :c0]), np.tril(host[:n, :c0])), name
        # the same call, the same bits
        buf2 = H.to_device(host)
        H.chol_update(buf2, n, H.to_device(W), row0=row0)
        H.sync()
        assert _same_bits(np.tril(buf2.cpu().numpy()[:n, :n]), Lg), name


@pytest.mark.parametrize("k", [3, 17])
def test_leading_rows_do_not_depend_on_what_follows(H, k):
    """row i of the result depends on rows <= i only: the update of n = 300 and that of its leading 129 rows agree bit for bit on
    those rows, and so do two leading dimensions"""
    _, L = _chol(300)
    rng = np.random.default_rng(77 + k)
    W = rng.standard_normal((300, k))
    W[:5] = 0.0
    res = {}
    for n, ld in ((300, 384), (129, 256), (300, 512), (129, 512)):
        buf = H.to_device(_factor_buffer(L[:n, :n], ld=ld))
        H.chol_update(buf, n, H.to_device(W[:n].copy()), row0=5)
        H.sync()
        res[n, ld] = np.tril(buf.cpu().numpy()[:n, :n])
    assert _same_bits(res[300, 384][:129, :129], res[129, 256])
    assert _same_bits(res[300, 384], res[300, 512])
    assert _same_bits(res[129, 256], res[129, 512])


def _delete_sets(n):
    rng = np.random.default_rng(9)
    return {"first": [0], "last": [n - 1], "straddle128": [127, 128, 129], "first16": list(range(16)),
            "scattered17": sorted(rng.choice(n, 17, replace=False).tolist()), "every_second": list(range(0, n, 2)),
            "tail5": list(range(n - 5, n))}


@pytest.mark.parametrize("which", ["first", "last", "straddle128", "first16", "scattered17", "every_second", "tail5"])
def test_chol_delete(H, which):
    from fvgp_amd._lib import pad128
    n = 300
    M, L = _chol(n)
    R = _delete_sets(n)[which]
    Rr, S = cr.split_indices(n, R)
    m = len(S)
    Ms = M[np.ix_(S, S)]
    ref = np.linalg.cholesky(Ms)
    host = _factor_buffer(L)
    buf = H.to_device(host)
    H.chol_delete(buf, n, R)
    H.invalidate_factor()
    H.sync()
    got = buf.cpu().numpy()
    scale = np.max(np.abs(L))
    err = np.max(np.abs(np.tril(got[:m, :m]) - ref)) / scale
    e_twin = np.max(np.abs(np.tril(got[:m, :m]) - cr.chol_delete(L, R))) / scale
    print(f"chol_delete|n={n}|{which}|k={len(Rr)}|vs cholesky {err:.3g}|vs twin {e_twin:.3g}")
    assert err <= TOL and e_twin <= TOL
    # rows n - k .. buffer end: identity padding (zeros, unit diagonal) on and below the diagonal
    npad = pad128(n)
    pad = np.tril(got[m:npad, :npad], m)
    assert np.array_equal(pad, np.eye(npad)[m:])
    # ... and what stands there serves as a factor of m points: solves and log-determinant as test_potrf_solve_logdet asks of potrf
    np.testing.assert_allclose(H.logdet(buf, m), 2 * np.sum(np.log(np.diag(ref))), rtol=1e-13)
    rng = np.random.default_rng(m)
    for nrhs in (1, 3, 8):
        rhs = rng.standard_normal((m, nrhs))
        B = np.full((pad128(m), nrhs), 7.0)          # junk in the padding rows must be cleared
        B[:m] = rhs
        Bd = H.to_device(B)
        H.potrs(buf, m, Bd, nrhs)
        H.sync()
        sol = sla.cho_solve((ref, True), rhs)
        out = Bd.cpu().numpy()
        assert np.max(np.abs(out[:m] - sol)) / np.max(np.abs(sol)) < 1e-12
        assert np.all(out[m:] == 0)
    # the same call, the same bits
    buf2 = H.to_device(host)
    H.chol_delete(buf2, n, R)
    H.invalidate_factor()
    H.sync()
    assert _same_bits(np.tril(buf2.cpu().numpy()[:npad, :npad]), np.tril(got[:npad, :npad]))


def test_argument_errors_name_their_position_and_write_nothing(H):
    from fvgp_amd import _lib
    n = 300
    _, L = _chol(n)
    host = _factor_buffer(L)
    buf = H.to_device(host)
    lib = _lib.lib()
    ws = H.empty(_lib.chol_update_workspace_bytes(n, 16) // 8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def delete(idx, k=None, ws_bytes=None, n_=n):
        a = np.asarray(idx, dtype=np.int64)
        return lib.fvgp_hip_chol_delete(H._h, p(buf), n_, buf.stride(0), a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        len(a) if k is None else k, p(ws), ws.numel() * 8 if ws_bytes is None else ws_bytes)
    assert delete([5, 3]) == -5                                  # unsorted
    assert delete([3, 3]) == -5                                  # duplicated
    assert delete([3, n]) == -5 and delete([-1, 2]) == -5        # out of range
    assert delete([0], k=0) == -6
    assert delete(np.arange(16), n_=16) == -6                    # k >= n
    assert delete(np.arange(16), ws_bytes=_lib.chol_update_workspace_bytes(n, 16) - 8) == -8
    assert lib.fvgp_hip_chol_delete(H._h, p(buf), n, buf.stride(0), None, 1, p(ws), ws.numel() * 8) == -5
    assert lib.fvgp_hip_chol_delete(H._h, p(buf), n, buf.stride(0) - 1, None, 1, p(ws), ws.numel() * 8) == -4
    W = H.zeros(n, 4)
    upd = lambda k, ldw, row0, wsb: lib.fvgp_hip_chol_update(H._h, p(buf), n, buf.stride(0), p(W), k, ldw, row0, p(ws), wsb)
    assert upd(0, 4, 0, ws.numel() * 8) == -6
    assert upd(4, 3, 0, ws.numel() * 8) == -7
    assert upd(4, 4, n + 1, ws.numel() * 8) == -8 and upd(4, 4, -1, ws.numel() * 8) == -8
    assert upd(4, 4, 0, _lib.CHOL_UPDATE_TABLE_BYTES - 8) == -10
    assert lib.fvgp_hip_chol_update(H._h, p(buf), n, buf.stride(0), None, 4, 4, 0, p(ws), ws.numel() * 8) == -5
    assert lib.fvgp_hip_chol_update(H._h, p(buf), n, buf.stride(0), p(W), 4, 4, 0, None, ws.numel() * 8) == -9
    with pytest.raises(_lib.HipExtensionError, match="status -5"):
        H.chol_delete(buf, n, [7, 7])
    H.sync()
    assert _same_bits(buf.cpu().numpy(), host)
