"""Float64 numpy model of gpmpc_gp_drop_oldest (csrc/gp_drop.hip), the cases its
tests share (tests/test_gp_drop_cpu.py, tests/test_gpu_gp_drop.py) and their margin.

State of a GP with n rows: X (n, d), M = L^-1 (n, n) lower triangular (K + sn2 I = L L^T) and
alpha = (K + sn2 I)^-1 y.  Dropping the first m <= 16 rows (index 1; the n2 = n - m kept rows are
index 2), in the block form the kernels use:

    L11 = M11^-1,  V = -M21 L11  (= L22^-1 L21),  K22 + sn2 I = L22 (I + V V^T) L22^T
    M'  = C^-1 M22,  C = chol(I + V V^T), applied per 16-row tile T of the kept rows (p: the kept
    rows before the tile):
        G_T = I_m + V_p^T V_p,  E_T = V_T G_T^-1,  D_T = chol(I_16 + E_T V_T^T)^-1,
        S_T = V_p^T B_p (B = M22),  M'_T = D_T (B_T - E_T S_T),  only column tiles J <= T
    P11 = M[:, :m]^T M[:, :m],  g = P11^-1 alpha_1,  alpha' = alpha_2 - M22^T (M21 g)

A larger m is cut into consecutive blocks of at most 16 rows.  Inert rows (a rejected append block:
zero input, zero weight, zero row and column of M) put a zero on the diagonal of M11 and P11, which
is treated as 1; among the kept rows they stay inert without special code.

Criterion, as for the append (tests/gp_append_ref.py): with e_full the worst error of a float64
full recompute of the kept rows (GaussianProcess.device_layout, the upload path) against the
np.longdouble reference (gp_append_ref.reference), a dropped GP's worst error must be at most
MARGIN_DROP e_full, per quantity.

R_MODEL.  The worst e_model / e_full of this model over CASES, the inert-row case and the sliding
window (both GPs; mean, variance and gradient), measured with tests/test_gp_drop_cpu.py -s:
R_MODEL = 11157 (mean, 17 - 16, gp1; gradient 7412 there).  MARGIN_DROP = ceil(4 R_MODEL) = 44628:
the factor 4 covers the MFMA summation order and the rounding carried from block to block (the
append's precedent: 8 over a model value of 1.6).

That figure is set by one case.  With one row left the yardstick is a 1 x 1 "factorisation", exact
to an ulp whatever the data (e_full 1e-17 .. 2e-16), while the dropped GP carries the rounding of
the 17-row factor it came from (e_model 1e-13, as in every other case): the ratio measures the
yardstick, not the update.  So the tests hold every state that keeps at least two rows to a second,
tighter margin as well: R_BULK = 31.4 is the model's worst ratio over those (variance, 120 - 7 - 16
- 3, gp0: e_model 5.5e-14; gradient 22.8 at 40 - 16 - 8, mean 20.9 with inert rows; 0.5 .. 9 in
the other cases, 6.9 after the sliding window's six rounds), MARGIN_BULK = ceil(4 R_BULK) = 126.
The ratios grow with the share of rows dropped: the kept rows inherit the rounding of the larger,
worse conditioned factor, and the recompute they are judged against factorises only the smaller one.
"""

from __future__ import annotations

import math

import numpy as np

import gp_ref as R

R_MODEL = 11157.0
MARGIN_DROP = float(math.ceil(4 * R_MODEL))
R_BULK = 31.4
MARGIN_BULK = float(math.ceil(4 * R_BULK))   # states that keep at least two rows


def margin(n_kept: int) -> float:
    return MARGIN_DROP if n_kept < 2 else MARGIN_BULK

SF2, SN2 = 1.0, 1e-3
NPTS = 64

# (name, rows, drops): each drop is one gpmpc_gp_drop_oldest call
CASES = [("a short block", 21, (5,)), ("a single dropped row", 33, (1,)), ("one row left", 17, (16,)),
         ("a full block", 48, (16,)), ("two separate drops", 40, (16, 8)), ("three blocks in one call", 64, (48,)),
         ("blocks unaligned to the tiles", 120, (7, 16, 3)), ("the headline N", 200, (16,)),
         ("npad 272 to 256", 272, (16,))]
CASE_IDS = [f"{n}-" + "-".join(str(m) for m in drops) for _, n, drops in CASES]


def targets(X):
    return np.sin(3.0 * X.sum(1)) + 0.5


def data(n, seed):
    """Per GP of quad2d (d = 1, 3): X (n, d), y (n,), ell, Z (NPTS, d); the setting of the append tests."""
    out = []
    for g, d in enumerate((1, 3)):
        gp = R.synthetic_gp(n, d, seed=seed + 17 * g, sf2=SF2, sn2=SN2)
        out.append(dict(X=gp["X"], y=targets(gp["X"]), ell=gp["ell"], Z=R.points(NPTS, d, seed=seed + 17 * g + 5), d=d))
    return out


def upload_state(X, y, ell, sf2=SF2, sn2=SN2):
    """(X, M, alpha) of the upload path: GaussianProcess.device_layout in float64."""
    import torch
    from gpmpc.gp import GaussianProcess

    gp = GaussianProcess(torch.tensor(np.asarray(X, dtype=np.float64)), torch.tensor(np.asarray(y, dtype=np.float64)))
    gp.set_hyperparameters(ell, sf2, sn2)
    lay = gp.device_layout("cpu")
    X = np.asarray(X, dtype=np.float64)
    return X.reshape(X.shape[0], -1).copy(), lay["Linv"].numpy().copy(), lay["alpha"].numpy().copy()


def with_inert(state, at, count):
    """The state with `count` inert rows inserted before row `at` (what a rejected append block leaves)."""
    X, M, alpha = state
    n = M.shape[0]
    live = np.r_[np.arange(at), np.arange(at, n) + count]
    Xn, Mn, an = np.zeros((n + count, X.shape[1])), np.zeros((n + count, n + count)), np.zeros(n + count)
    Xn[live], an[live] = X, alpha
    Mn[np.ix_(live, live)] = M
    return Xn, Mn, an


def _chol(A):
    """Lower Cholesky factor by columns and whether every pivot was finite and positive."""
    n = A.shape[0]
    L, ok = np.zeros_like(A), True
    for j in range(n):
        s = A[j:, j] - L[j:, :j] @ L[j, :j]
        good = bool(np.isfinite(s[0]) and s[0] > 0.0)
        ok = ok and good
        ljj = math.sqrt(s[0]) if good else 1.0
        L[j, j] = ljj
        L[j + 1:, j] = s[1:] / ljj
    return L, ok


def _inv_lower(L):
    n = L.shape[0]
    Li = np.zeros_like(L)
    for c in range(n):
        for i in range(c, n):
            Li[i, c] = ((1.0 if i == c else 0.0) - L[i, c:i] @ Li[c:i, c]) / L[i, i]
    return Li


def _spd_solve(Lc, b):
    """(Lc Lc^T)^-1 b, b (n,) or (n, k)."""
    y = np.zeros_like(b, dtype=np.float64)
    for i in range(Lc.shape[0]):
        y[i] = (b[i] - Lc[i, :i] @ y[:i]) / Lc[i, i]
    x = np.zeros_like(y)
    for i in range(Lc.shape[0] - 1, -1, -1):
        x[i] = (y[i] - Lc[i + 1:, i] @ x[i + 1:]) / Lc[i, i]
    return x


def drop_block(state, m, info=None):
    """One block of m <= 16 rows; returns (state', ok)."""
    X, M, alpha = state
    n = M.shape[0]
    assert 1 <= m <= 16 and m < n
    n2 = n - m
    M11 = M[:m, :m].copy()
    dz = np.diag(M11) == 0.0
    M11[dz, dz] = 1.0                                   # inert dropped rows
    ok = bool(np.all(np.isfinite(np.diag(M11)) & (np.diag(M11) > 0.0)))
    L11 = _inv_lower(M11)
    M21, B = M[m:, :m], M[m:, m:]
    V = -(M21 @ L11)
    P11 = M[:, :m].T @ M[:, :m]
    pz = np.diag(P11) == 0.0
    P11[pz, pz] = 1.0
    Lp, okp = _chol(P11)
    g = _spd_solve(Lp, alpha[:m])
    alpha2 = alpha[m:] - B.T @ (M21 @ g)
    ok = ok and okp
    Mn = np.zeros((n2, n2))
    G = np.eye(m)
    S = np.zeros((m, n2))
    condG = 1.0
    for lo in range(0, n2, 16):
        hi = min(lo + 16, n2)
        VT, BT = V[lo:hi], B[lo:hi]
        Lg, okg = _chol(G)
        E = _spd_solve(Lg, VT.T).T
        Lf, okf = _chol(np.eye(hi - lo) + E @ VT.T)
        D = _inv_lower(Lf)
        ok = ok and okg and okf
        condG = max(condG, float(np.linalg.cond(G)))
        # column tiles J <= T; the diagonal tile's upper triangle is written as exact zeros
        Mn[lo:hi, :hi] = np.tril(D @ (BT[:, :hi] - E @ S[:, :hi]), lo)
        S += VT.T @ BT
        G += VT.T @ VT
    if info is not None:
        info["condG"] = max(info.get("condG", 1.0), condG)
    return (X[m:].copy(), Mn, alpha2), ok


def drop_oldest(state, m, info=None):
    """gpmpc_gp_drop_oldest: consecutive blocks of at most 16 rows; returns (state', flags)."""
    flags = []
    for done in range(0, m, 16):
        state, ok = drop_block(state, min(16, m - done), info)
        flags.append(1 if ok else 0)
    return state, flags


def kernel64(X, ell, sf2, Z):
    q = ((Z[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    return sf2 * np.exp(-0.5 * q / ell ** 2)


def append_block(state, Xb, yb, ell, sf2=SF2, sn2=SN2):
    """The bordered update of csrc/gp_append.hip in float64 (an accepted block)."""
    X, M, alpha = state
    n, m = M.shape[0], len(yb)
    Xb = np.asarray(Xb, dtype=np.float64).reshape(m, -1)
    Kb = kernel64(X, ell, sf2, Xb).T                     # (n, m)
    W = M @ Kb
    Sc = kernel64(Xb, ell, sf2, Xb) + sn2 * np.eye(m) - W.T @ W
    Lb, ok = _chol(Sc)
    assert ok
    Lbi = _inv_lower(Lb)
    Rn = -Lbi @ (W.T @ M)
    beta = Lbi @ (np.asarray(yb, dtype=np.float64) - Kb.T @ alpha)
    Mn = np.zeros((n + m, n + m))
    Mn[:n, :n], Mn[n:, :n], Mn[n:, n:] = M, Rn, Lbi
    return np.vstack([X, Xb]), Mn, np.concatenate([alpha + Rn.T @ beta, Lbi.T @ beta])


def predict(state, ell, Z, sf2=SF2, sn2=SN2) -> dict:
    """mean, predictive variance and gradient at Z from a state, in float64."""
    X, M, alpha = state
    Z = np.asarray(Z, dtype=np.float64).reshape(len(Z), -1)
    k = kernel64(X, ell, sf2, Z)
    v = M @ k.T
    grad = np.stack([((k * alpha[None, :]) * (X[None, :, c] - Z[:, c, None])).sum(1) / ell ** 2
                     for c in range(X.shape[1])], axis=1)
    return dict(mean=k @ alpha, var=sf2 - (v * v).sum(0) + sn2, grad=grad)
