"""Float64 numpy model of gpmpc_gp_refactor (csrc/gp_refactor.hip), the cases its
tests share (tests/test_gp_refactor_cpu.py, tests/test_gpu_gp_refactor.py) and their margin.

The model follows the kernels block by block, over the padded size npad = 16 nt:

    Khat = k(X, X) + sn2 I with the diagonal exactly sf2 + sn2; an inert or padding row is an
    identity row (diagonal 1, off-diagonal 0)
    for k = 0 .. nt-1                                  (right-looking, 16-wide panels)
        L_kk = chol(A_kk), L_kk^-1                      unblocked, by columns
        L_ik = A_ik L_kk^-T                  i > k
        A_ij -= L_ik L_jk^T                  k < j <= i
        X_kj = L_kk^-1 B_kj (B_kk = I)       j <= k     row tile k of M = L^-1
        B_ij -= L_ik X_kj                    i > k, j <= k   (first touch at j == k: B_ij = -L_ik X_kk)
    w = M y, alpha = M^T w                              the two substitutions, with the inverse factor
    inert rows: zero row and column of M, zero weight; their target is never read

State and `predict` are those of tests/gp_drop_ref.py: (X, M, alpha) with M = L^-1 lower triangular.

Criterion, as for the append and the drop: with e_full the worst error of a float64 full recompute
(GaussianProcess.device_layout, the upload path) against the np.longdouble reference
(gp_append_ref.reference), a refactorised GP's worst error must be at most MARGIN_REFACTOR e_full, per
quantity.

R_MODEL.  The worst e_model / e_full of this model over `model_cases()` (both GPs; mean, variance and
gradient), measured with tests/test_gp_refactor_cpu.py -s: R_MODEL = 5.06 (gradient, refresh at 33
rows, gp1: e_model 3.8e-12 against e_full 7.5e-13; mean 2.9 with inert rows, variance 3.9 at 16 rows;
0.5 .. 2 in most other cases, and 0.002 .. 0.04 for gp0's mean and gradient, where the upload path's
weights K^-1 y from an explicit inverse are the less accurate ones).  MARGIN_REFACTOR =
ceil(4 R_MODEL) = 21: the factor 4 covers the MFMA summation order, as for the drop.  The CPU test recomputes the ratio and
fails when ceil(4 x it) exceeds the constant stored here.
"""

from __future__ import annotations

import math

import numpy as np

import gp_drop_ref as D

SF2, SN2, NPTS = D.SF2, D.SN2, D.NPTS
# refresh at unchanged hyperparameters: (rows, capacity)
REFRESH = [(5, 16), (16, 16), (17, 40), (33, 64), (100, 128), (200, 200), (272, 272)]
REFRESH_IDS = [f"{n}-cap{c}" for n, c in REFRESH]
# new hyperparameters: ell' = ELL_SCALE ell, sf2', sn2'
NEW_ROWS = (33, 200)
ELL_SCALE, SF2_NEW, SN2_NEW = 0.8, 2.0, 5e-3

R_MODEL = 5.06
MARGIN_REFACTOR = float(math.ceil(4 * R_MODEL))


def seed_for(n: int) -> int:
    return 1300 + n


def refactor(X, y, ell, sf2=SF2, sn2=SN2, inert=None):
    """The model: (state, ok) from inputs X (n, d), targets y (n,), a boolean mask of inert rows."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    y = np.asarray(y, dtype=np.float64)
    n = X.shape[0]
    npad = (n + 15) // 16 * 16
    nt = npad // 16
    mask = np.ones(npad, dtype=bool)
    mask[:n] = False if inert is None else np.asarray(inert, dtype=bool)
    Xp = np.zeros((npad, X.shape[1]))
    Xp[:n] = X
    A = D.kernel64(Xp, ell, sf2, Xp)
    A[np.arange(npad), np.arange(npad)] = sf2 + sn2
    A[mask, :] = 0.0
    A[:, mask] = 0.0
    A[mask, mask] = 1.0
    ok = bool(np.isfinite(y[~mask[:n]]).all())
    t = lambda i: slice(16 * i, 16 * i + 16)   # noqa: E731
    M = np.zeros((npad, npad))
    B = np.zeros((npad, npad))
    for k in range(nt):
        Lkk, okk = D._chol(A[t(k), t(k)])
        ok = ok and okk
        Li = D._inv_lower(Lkk)
        for i in range(k + 1, nt):
            A[t(i), t(k)] = A[t(i), t(k)] @ Li.T
        for i in range(k + 1, nt):
            for j in range(k + 1, i + 1):
                A[t(i), t(j)] -= A[t(i), t(k)] @ A[t(j), t(k)].T
        for j in range(k + 1):
            Xkj = Li if j == k else Li @ B[t(k), t(j)]
            M[t(k), t(j)] = Xkj
            for i in range(k + 1, nt):
                upd = A[t(i), t(k)] @ Xkj
                B[t(i), t(j)] = -upd if j == k else B[t(i), t(j)] - upd
    M[mask, :] = 0.0
    M[:, mask] = 0.0
    ym = np.zeros(npad)
    ym[:n][~mask[:n]] = y[~mask[:n]]
    w = M @ ym
    alpha = M.T @ w
    alpha[mask] = 0.0
    Xs = X.copy()
    return (Xs, M[:n, :n].copy(), alpha[:n].copy()), ok


def new_hypers(dg):
    return ELL_SCALE * dg["ell"], SF2_NEW, SN2_NEW


def inert_case():
    """20 rows, a rejected block of 6, an accepted block of 8, a rejected block of 5: 39 rows, 28 live.
    Returns (data of 28 + 32 rows per GP, boolean inert mask of the 39 rows, index of the live rows)."""
    data = D.data(28 + 32, seed=1500)
    mask = np.zeros(39, dtype=bool)
    mask[20:26] = True
    mask[34:39] = True
    return data, mask, np.flatnonzero(~mask)


def model_cases():
    """Every refactorised state the GPU tests judge, as (name, g, state, ok, dg, rows, hypers): `rows`
    index the GP's data the state must equal a recompute of, hypers = (ell, sf2, sn2)."""
    out = []
    for n, _ in REFRESH:
        for g, dg in enumerate(D.data(n, seed=seed_for(n))):
            st, ok = refactor(dg["X"], dg["y"], dg["ell"])
            out.append((f"refresh {n}", g, st, ok, dg, slice(0, n), (dg["ell"], SF2, SN2)))
    for n in NEW_ROWS:
        for g, dg in enumerate(D.data(n, seed=seed_for(n))):
            hyp = new_hypers(dg)
            st, ok = refactor(dg["X"], dg["y"], *hyp)
            out.append((f"new hyperparameters {n}", g, st, ok, dg, slice(0, n), hyp))
    for g, dg in enumerate(D.data(64 + 96, seed=800)):   # the window the drop tests' six rounds end on
        st, ok = refactor(dg["X"][96:160], dg["y"][96:160], dg["ell"])
        out.append(("after drift", g, st, ok, dg, slice(96, 160), (dg["ell"], SF2, SN2)))
    data, mask, live = inert_case()
    for g, dg in enumerate(data):
        X, y = np.zeros((39, dg["d"])), np.full(39, np.nan)
        X[live], y[live] = dg["X"][:28], dg["y"][:28]
        st, ok = refactor(X, y, dg["ell"], inert=mask)
        out.append(("inert rows", g, st, ok, dg, slice(0, 28), (dg["ell"], SF2, SN2)))
    for g, dg in enumerate(D.data(48 + 16, seed=1600)):
        st, ok = refactor(dg["X"][:48], dg["y"][:48], dg["ell"])
        out.append(("before append and drop", g, st, ok, dg, slice(0, 48), (dg["ell"], SF2, SN2)))
    return out
