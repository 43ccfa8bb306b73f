"""A numpy twin of the rank-k Cholesky update the device runs (fvgp_amd/csrc/chol_update.hip), a helper module of the tests (not a
conftest), and the identity that turns the removal of data points into such an update.

With KV = L L^T, R the sorted removed indices and S the kept ones in their original order,

    KV[S,S] = L[S,S] L[S,S]^T + L[S,R] L[S,R]^T

L[S,S] is lower triangular with a positive diagonal, so the factor of the kept points is chol(L[S,S] L[S,S]^T + W W^T), W = L[S,R]:
a positive rank-|R| update.  `chol_update` is the sweep of the kernels, operation for operation up to fused multiply-adds: passes of at
most 16 columns of W; in a pass column j of L is rotated against the columns p of W in turn with

    q_p = L_jj^2 + sum_{u <= p} W_ju^2,   r_p = sqrt(q_p),   c_p = r_{p-1} / r_p,   s_p = W_jp / r_p      (r_{-1} = L_jj)
    rows i > j:  (L_ij, W_ip) <- (c_p L_ij + s_p W_ip,  c_p W_ip - s_p L_ij),         L_jj <- r_{kp-1}
"""
import numpy as np

MAX_RANK = 16


def split_indices(n, removed):
    """(R, S): the sorted unique removed indices and the kept ones, in order"""
    R = np.unique(np.asarray(removed, dtype=np.int64))
    keep = np.ones(n, dtype=bool)
    keep[R] = False
    return R, np.flatnonzero(keep)


def compaction(L, removed):
    """(L[S,S], W = L[S,R]) of a lower-triangular factor: the operands of the update that removes `removed`"""
    L = np.tril(L)
    R, S = split_indices(len(L), removed)
    return L[np.ix_(S, S)].copy(), L[np.ix_(S, R)].copy()


def chol_update(L, W, row0=0):
    """chol(L L^T + W W^T) by the kernels' sweep; rows < row0 of W are taken to be zero (columns left of row0 are skipped).  Returns a new
    array; only the lower triangle of L is read."""
    L = np.tril(np.array(L, dtype=np.float64))
    W = np.array(W, dtype=np.float64).reshape(len(L), -1)
    n, k = W.shape
    for p0 in range(0, k, MAX_RANK):
        Wp = W[:, p0:p0 + MAX_RANK]
        kp = Wp.shape[1]
        for j in range(row0, n):
            l = L[j, j]
            q = l * l + np.cumsum(Wp[j] * Wp[j])
            r = np.sqrt(q)
            rprev = np.concatenate([[l], r[:-1]])
            c, s = rprev / r, Wp[j] / r
            col = L[j + 1:, j].copy()
            for p in range(kp):
                sw = s[p] * Wp[j + 1:, p]
                Wp[j + 1:, p] = c[p] * Wp[j + 1:, p] - s[p] * col
                col = c[p] * col + sw
            L[j + 1:, j] = col
            L[j, j] = r[-1]
    return L


def chol_delete(L, removed):
    """the factor of the kept points from the factor of all of them"""
    Lss, W = compaction(L, removed)
    R, _ = split_indices(len(L), removed)
    return chol_update(Lss, W, row0=int(R[0]) if len(R) and R[0] < len(Lss) else len(Lss))
