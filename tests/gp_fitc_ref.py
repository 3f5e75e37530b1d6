"""Float64 numpy model of gpmpc_gp_fitc (csrc/gp_fitc.hip), the np.longdouble reference,
the cases its tests share (tests/test_gp_fitc_cpu.py, tests/test_gpu_gp_fitc.py) and their margin.

The model follows the kernels tile by tile, over the padded sizes npad = 16 nt (training rows) and
mpad = 16 mt (inducing rows S = X[idx]):

    K_ss + jitter I with the diagonal exactly sf2 + jitter; a padding row is an identity row
    L, L^-1 by the right-looking 16-wide panels of gp_refactor.hip (tests/gp_refactor_ref.py)
    V tile (I, :) = sum over kt = 0 .. I, ascending, of L^-1 tile (I, kt) k(S tile kt, X); an inert or
        padding column of V is exact zeros
    Gamma_i = sf2 + sn2 - |V[:, i]|^2 with the rows summed in four interleaved sums, (s0 + s1) + (s2 + s3);
        Gamma^-1 = 0 for an inert row, whose target is never read
    B tile (I, J) = I + V_I Gamma^-1 V_J^T in four sums over the columns = j mod 4, added (g0 + g1) + (g2 + g3)
    C, C^-1 by the same panels;  u = V Gamma^-1 y,  p = C^-1 u,  q = C^-T p,  w = L^-T q

The status is 0 for an index outside 0 .. n-1 or naming an inert row, a live target that is not finite, a
pivot of L or C or a live row's Gamma that is not finite and positive.

Reference.  The reference's own formula (gpmpc/gpmpc.py:392-397) with K_ss + jitter I in place of K_ss, in
np.longdouble on the live rows, the two solves by a longdouble Cholesky factorisation (both matrices are
symmetric positive definite; chol_ld asserts every pivot):

    Gamma = diag(K) - rowsum(K_xs * solve(K_ss, K_sx)^T)   (diag(K) = sf2 + sn2)
    KG = K_sx / Gamma,  w = solve(K_ss + KG K_xs, KG y)

Criterion, the convention of gp_drop_ref.py / gp_refactor_ref.py: with e_full the worst error of a plain
float64 numpy evaluation of that same formula (np.linalg.solve) against the longdouble one, per quantity
(FITC mean and its gradient at the case's Z, 64 points), the model's and the device's worst error must be at
most MARGIN_FITC e_full.  Weights are never compared: they are not determined when K_ss is ill-conditioned.

R_MODEL.  The worst e_model / e_full of this model over `cases()` and the inert-row case (mean and gradient),
measured with tests/test_gp_fitc_cpu.py -s: R_MODEL = 1.34 (gradient, 33 rows, M = 1, gp0: e_model 4.4e-16
against e_full 3.3e-16, both a few ulp; mean 1.0 in the same case).  Everywhere else the factored form is the
more accurate one: 0.2 .. 0.7 for the 3-D GP at 21 rows (errors of 1e-14), and 0.0001 .. 0.006 in the other
cases, where K_ss is ill-conditioned and the solve form loses more digits (e_full 1e-10 .. 7e-4, e_model
1e-13 .. 3e-7; the largest at 200 rows, M = 72, gp1).  MARGIN_FITC = ceil(4 R_MODEL) = 6: the factor 4 covers
the MFMA summation order, as for the drop and the refactorisation.  The CPU test recomputes the ratio and fails
when ceil(4 x it) exceeds the constant stored here.
"""

from __future__ import annotations

import math

import numpy as np

import gp_drop_ref as D
import gp_ref as R
from gp_append_ref import chol_ld, solve_lower_ld, solve_upper_ld

LD = R.LD
SF2, SN2, NPTS = D.SF2, D.SN2, D.NPTS
JITTER = 1e-8
# (rows, capacity, inducing rows)
SHAPES = [(21, 32, 5), (33, 64, 1), (40, 40, 16), (40, 64, 40), (150, 160, 40), (200, 200, 72), (272, 272, 100)]
# jitter 0, the reference's own formula: the 3-D GP (gp 1) where cond(K_ss) is 43 and 4e4
JITTER0 = [(21, 32, 5), (40, 40, 16)]

R_MODEL = 1.34
MARGIN_FITC = float(math.ceil(4 * R_MODEL))


def seed_for(n: int, M: int) -> int:
    return 1700 + 7 * n + M


def draw(n: int, M: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).choice(n, M, replace=False).astype(np.int32)


def cases():
    """(id, n, capacity, M, jitter, gps): every build the tests judge; gps the GPs it runs on."""
    out = [(f"{n}-cap{c}-M{M}", n, c, M, JITTER, (0, 1)) for n, c, M in SHAPES]
    out += [(f"{n}-cap{c}-M{M}-jitter0", n, c, M, 0.0, (1,)) for n, c, M in JITTER0]
    return out


CASES = cases()
CASE_IDS = [c[0] for c in CASES]


def case_data(n: int, M: int):
    """(data per GP as gp_drop_ref.data, idx (M,) int32)."""
    seed = seed_for(n, M)
    return D.data(n, seed=seed), draw(n, M, seed)


def inert_case():
    """40 rows, then a rejected block of 5 (gp_update_util.nan_block): 45 rows, 40 live; M = 16 over the live
    rows.  Returns (data of 40 rows per GP, boolean inert mask of the 45 rows, idx (16,), targets with NaN on
    the inert rows per GP)."""
    data = D.data(40, seed=1900)
    mask = np.zeros(45, dtype=bool)
    mask[40:] = True
    idx = draw(40, 16, 1900)
    ys = [np.r_[dg["y"], np.full(5, np.nan)] for dg in data]
    return data, mask, idx, ys


def _factor(A, mask):
    """gp_refactor.hip's panels on a matrix already in A (lower tiles): (M = L^-1 with masked rows and columns
    zeroed, every pivot finite and positive)."""
    npad = A.shape[0]
    nt = npad // 16
    A = A.copy()
    ok = True
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
    return M, ok


def fitc(X, y, idx, ell, sf2=SF2, sn2=SN2, jitter=0.0, inert=None):
    """The model: ((S (M, d), w (M,)), ok) from the n training rows X, their targets y, the inducing indices
    and a boolean mask of inert rows."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    y = np.asarray(y, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    n, d = X.shape
    M = len(idx)
    npad, mpad = (n + 15) // 16 * 16, (M + 15) // 16 * 16
    nt, mt = npad // 16, mpad // 16
    lmask = np.ones(npad, dtype=bool)
    lmask[:n] = False if inert is None else np.asarray(inert, dtype=bool)
    with np.errstate(all="ignore"):
        ok = bool(np.isfinite(y[~lmask[:n]]).all())
        bad = (idx < 0) | (idx >= n)
        bad[~bad] = lmask[idx[~bad]]
        ok = ok and not bad.any()
        idx = np.where(bad, 0, idx)
        S = np.zeros((mpad, d))
        S[:M] = X[idx]
        smask = np.arange(mpad) >= M
        A = D.kernel64(S, ell, sf2, S)
        A[np.arange(mpad), np.arange(mpad)] = sf2 + jitter
        A[smask, :] = 0.0
        A[:, smask] = 0.0
        A[smask, smask] = 1.0
        Li, okl = _factor(A, smask)
        Xp = np.zeros((npad, d))
        Xp[:n] = X
        Ksx = D.kernel64(Xp, ell, sf2, S)               # (mpad, npad)
        Ksx[:, lmask] = 0.0
        t = lambda i: slice(16 * i, 16 * i + 16)   # noqa: E731
        V = np.zeros((mpad, npad))
        for I in range(mt):
            for kt in range(I + 1):
                V[t(I)] += Li[t(I), t(kt)] @ Ksx[t(kt)]
        V2 = V * V
        s = [V2[k::4].sum(0) for k in range(4)]
        gam = (sf2 + sn2) - ((s[0] + s[1]) + (s[2] + s[3]))
        good = np.isfinite(gam) & (gam > 0.0)
        okg = bool(good[~lmask].all())
        ginv = np.where(~lmask & good, 1.0 / np.where(good, gam, 1.0), 0.0)
        ym = np.zeros(npad)
        ym[:n][~lmask[:n]] = y[~lmask[:n]]
        tt = ginv * ym
        Bm = np.zeros((mpad, mpad))
        for I in range(mt):
            for J in range(I + 1):
                g = [(V[t(I), j::4] * ginv[j::4]) @ V[t(J), j::4].T for j in range(4)]
                Bm[t(I), t(J)] = (g[0] + g[1]) + (g[2] + g[3])
        Bm[np.arange(mpad), np.arange(mpad)] += 1.0
        Bm[smask, :] = 0.0
        Bm[:, smask] = 0.0
        Bm[smask, smask] = 1.0
        Ci, okc = _factor(Bm, smask)
        u = V @ tt
        w = Li.T @ (Ci.T @ (Ci @ u))
    return (S[:M].copy(), w[:M].copy()), bool(ok and okl and okg and okc)


def evaluate(S, w, ell, Z, sf2=SF2) -> dict:
    """FITC mean (P,) and gradient (P, d) at Z in float64: sum_j w_j k(z, S_j), k carrying sf2."""
    S = np.asarray(S, dtype=np.float64).reshape(len(w), -1)
    Z = np.asarray(Z, dtype=np.float64).reshape(len(Z), -1)
    k = D.kernel64(S, ell, sf2, Z)
    grad = np.stack([((k * w[None, :]) * (S[None, :, c] - Z[:, c, None])).sum(1) / ell ** 2
                     for c in range(S.shape[1])], axis=1)
    return dict(mean=k @ w, grad=grad)


def reference(X, y, idx, ell, Z, sf2=SF2, sn2=SN2, jitter=0.0) -> dict:
    """FITC mean and gradient at Z from the reference's formula in np.longdouble (live rows only), rounded to
    float64.  chol_ld asserts every pivot: the formula itself goes through."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    Z = np.asarray(Z, dtype=np.float64).reshape(len(Z), -1)
    S = X[np.asarray(idx)]
    M = S.shape[0]
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    Kss = R.kernel_ld(S, ell, sf2, S) + LD(float(jitter)) * np.eye(M, dtype=LD)
    Kxs = R.kernel_ld(S, ell, sf2, X)                    # (n, M)
    L = chol_ld(Kss)
    sol = solve_upper_ld(L.T, solve_lower_ld(L, Kxs.T.copy()))   # K_ss^-1 K_sx (M, n)
    gamma = (LD(float(sf2)) + LD(float(sn2))) - (Kxs * sol.T).sum(1)
    assert float(gamma.min()) > 0.0, float(gamma.min())
    KG = Kxs.T / gamma[None, :]
    L2 = chol_ld(Kss + KG @ Kxs)
    w = solve_upper_ld(L2.T, solve_lower_ld(L2, KG @ yl))
    kz = R.kernel_ld(S, ell, sf2, Z)
    l2 = LD(float(ell)) ** 2
    grad = np.stack([((kz * w[None, :]) * (S[None, :, c].astype(LD) - Z[:, c, None].astype(LD))).sum(1) / l2
                     for c in range(S.shape[1])], axis=1)
    return dict(mean=(kz @ w).astype(np.float64), grad=grad.astype(np.float64), gamma_min=float(gamma.min()))


def numpy64(X, y, idx, ell, Z, sf2=SF2, sn2=SN2, jitter=0.0) -> dict:
    """The yardstick: the same formula in plain float64 numpy, the solve form of gpmpc/gpmpc.py:392-397."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    y = np.asarray(y, dtype=np.float64)
    S = X[np.asarray(idx)]
    Kss = D.kernel64(S, ell, sf2, S) + jitter * np.eye(S.shape[0])
    Kxs = D.kernel64(S, ell, sf2, X)
    gamma = (sf2 + sn2) - (Kxs * np.linalg.solve(Kss, Kxs.T).T).sum(1)
    KG = Kxs.T / gamma
    w = np.linalg.solve(Kss + KG @ Kxs, KG @ y)
    return evaluate(S, w, ell, Z, sf2)
