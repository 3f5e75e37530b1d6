"""Float64 numpy model of gpmpc_gp_love_root (csrc/gp_love.hip): Lanczos with full
reorthogonalisation on the live rows of Khat, the host code's breakdown rule, and the root of
Q T^-1 Q^T from the bidiagonal Cholesky factor of T instead of its eigendecomposition.  Inert rows
(``inert`` True) take no part: their row and column of Khat are zero, their start entry is never
read and their rows of Q and R are exact zeros."""

import numpy as np


def bidiagonal_factor(alpha, beta):
    """T = C C^T for the tridiagonal T (diagonal alpha [m], off-diagonal beta [m - 1]), C lower
    bidiagonal: (diagonal c, subdiagonal l with l[0] = 0, ok).  ok = 0 at the first pivot that is
    not finite and positive; c and l are then meaningless."""
    m = len(alpha)
    c, l = np.zeros(m), np.zeros(m)
    lj = 0.0
    for j in range(m):
        piv = alpha[j] - lj * lj
        if not (np.isfinite(piv) and piv > 0.0):
            return c, l, 0
        c[j] = np.sqrt(piv)
        l[j] = lj
        if j + 1 < m:
            lj = beta[j] / c[j]
    return c, l, 1


def bidiagonal_root(Q, c, l):
    """R = Q C^-T: R[:, j] = (Q[:, j] - l_j R[:, j-1]) / c_j."""
    R = np.zeros_like(Q)
    prev = np.zeros(Q.shape[0])
    for j in range(Q.shape[1]):
        prev = (Q[:, j] - l[j] * prev) / c[j]
        R[:, j] = prev
    return R


def love_root(K, rank, start, inert=None):
    """(R (n, m), m, ok) as the device builds them from Khat = K, the rank asked for and the start
    vector.  ok = 0: no root (R is None)."""
    n = K.shape[0]
    live = np.ones(n, dtype=bool) if inert is None else ~np.asarray(inert, dtype=bool)
    Km = np.where(live[:, None] & live[None, :], K, 0.0)
    q = np.where(live, start, 0.0)
    kmax = min(int(rank), int(live.sum()))
    if kmax < 1:
        return None, 0, 0
    Q = np.zeros((n, kmax))
    alpha, beta = np.zeros(kmax), np.zeros(kmax)
    q = q / np.sqrt(q @ q)
    m = kmax
    for j in range(kmax):
        Q[:, j] = q
        v = Km @ q
        alpha[j] = q @ v
        v = v - alpha[j] * q
        if j > 0:
            v = v - beta[j - 1] * Q[:, j - 1]
        for _ in range(2):
            v = v - Q[:, : j + 1] @ (Q[:, : j + 1].T @ v)
        b = np.sqrt(v @ v)
        if j + 1 >= kmax or not b > 1e-12 * np.abs(alpha[: j + 1]).max():
            m = j + 1
            break
        beta[j] = b
        q = v / b
    c, l, ok = bidiagonal_factor(alpha[:m], beta[: m - 1])
    if not ok:
        return None, m, 0
    return bidiagonal_root(Q[:, :m], c, l), m, 1
