"""Float64 numpy model of gpmpc_gp_mll (csrc/gp_fit.hip), an np.longdouble recompute
of the same quantities, the tile edge cases the tests share (tests/test_gp_fit_model_cpu.py,
tests/test_gpu_gp_fit.py) and their margin.

Quantities: MLL / n and its gradient with respect to (lengthscale, outputscale, noise), n the number of
live rows (the ExactMarginalLogLikelihood convention of gpmpc.gp.exact_mll and oracle/gp_fit_oracle.py).

The model follows the kernels over the padded size npad = 16 nt, from the state a factorisation leaves
(M = L^-1 with an inert or padding row's row and column zero, alpha = M^T (M y) with zeros there):

    for I = 0 .. nt-1, J = 0 .. I                       one wave per lower tile
        Kinv_IJ = sum_{t >= I} linvT[I, t] linvT[J, t]^T    (linvT = M^T; column tiles before I are zeros)
        W = alpha_I alpha_J^T - Kinv_IJ, E = exp(-D2 / 2 ell^2)
        partial = (sum W E D2, sum W E, trace W on I == J), the first two doubled when J < I
    the partials are added in tile order
    log det Khat = -2 sum log M_ii, y^T alpha and the count n over the live rows

The state judged is a factorisation's, the one every iteration of the fit evaluates: the GPU test
refactorises the uploaded GP at its own hyperparameters first.  An upload's weights are K^-1 y from an
explicit inverse (GaussianProcess.device_layout); evaluated on that state (upload_state) this model's
d/d lengthscale is up to 116 yardstick errors off (33 rows, gp0) and the device's 102 (16 and 17 rows, gp0), which
is the upload's error and not the evaluation's.  Both tests print those figures without judging them.

Criterion on the edge cases (EDGE: ragged last tile, exactly one tile, two tiles with one real row in the
second, three tiles; both GPs of problem("quad2d", n) at the controller's lengthscales with sf2 = 1,
sn2 = 1e-3).  The reference is the longdouble recompute.  The yardstick is the parent's path on the same
case, exact_mll + autograd in float64, whose error e_yard per quantity is floored at 1e-14 (1 + |ref|).
An evaluation's error may be at most MARGIN_FIT e_yard.

R_MODEL.  The worst e_model / e_yard of this model over the edge cases and the four quantities, measured
with tests/test_gp_fit_model_cpu.py -s: R_MODEL = 2.65 (d/d lengthscale at 33 rows, gp0: e_model 7.7e-14
against e_yard 2.9e-14, which is the floor, on a value of 1.9; 2.60 and 2.26 for the same quantity at 17 and 16
rows, 0.04 .. 1.4 elsewhere).  MARGIN_FIT = ceil(4 R_MODEL) = 11: the factor 4
covers the MFMA summation order, as for the drop and the refactorisation.  The CPU test recomputes the
ratio and fails when it exceeds the constant stored here.
"""

from __future__ import annotations

import math

import numpy as np

import gp_ref as R
from gp_append_ref import chol_ld, solve_lower_ld

LD = R.LD
SF2, SN2 = 1.0, 1e-3
EDGE = [(5, 16), (16, 16), (17, 40), (33, 64)]   # (rows, capacity)
EDGE_IDS = [f"{n}-cap{c}" for n, c in EDGE]
QUANT = ("mll", "d_ell", "d_sf2", "d_sn2")
FLOOR = 1e-14

R_MODEL = 2.65
MARGIN_FIT = float(math.ceil(4 * R_MODEL))


def _sq(X):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    return X


def factor_state(X, y, ell, sf2, sn2, inert=None):
    """(Xp, M, alpha, live) over the padded size from a float64 Cholesky: what a factorisation leaves."""
    X = _sq(X)
    y = np.asarray(y, dtype=np.float64)
    n = X.shape[0]
    npad = (n + 15) // 16 * 16
    mask = np.ones(npad, dtype=bool)
    mask[:n] = False if inert is None else np.asarray(inert, dtype=bool)
    Xp = np.zeros((npad, X.shape[1]))
    Xp[:n] = X
    D2 = ((Xp[:, None, :] - Xp[None, :, :]) ** 2).sum(-1)
    A = sf2 * np.exp(-0.5 * D2 / ell**2)
    A[np.arange(npad), np.arange(npad)] = sf2 + sn2
    A[mask, :] = 0.0
    A[:, mask] = 0.0
    A[mask, mask] = 1.0
    L = np.linalg.cholesky(A)
    M = np.linalg.solve(L, np.eye(npad))
    M = np.tril(M)
    M[mask, :] = 0.0
    M[:, mask] = 0.0
    ym = np.zeros(npad)
    ym[:n][~mask[:n]] = y[~mask[:n]]
    alpha = M.T @ (M @ ym)
    alpha[mask] = 0.0
    return Xp, M, alpha, ~mask


def upload_state(X, y, ell, sf2, sn2):
    """(Xp, M, alpha, live) as an upload leaves them on the handle (gp_drop_ref.upload_state:
    GaussianProcess.device_layout, whose weights are K^-1 y from an explicit inverse), padded."""
    import gp_drop_ref as D

    Xs, M, alpha = D.upload_state(_sq(X), y, ell, sf2, sn2)
    n = Xs.shape[0]
    npad = (n + 15) // 16 * 16
    Xp, Mp, ap, live = np.zeros((npad, Xs.shape[1])), np.zeros((npad, npad)), np.zeros(npad), np.zeros(npad, dtype=bool)
    Xp[:n], Mp[:n, :n], ap[:n], live[:n] = Xs, M, alpha, True
    return Xp, Mp, ap, live


def tile_model(X, y, ell, sf2, sn2, inert=None, state=None):
    """The model: (MLL / n, gradient (3,)) as gp_fit_grad_kernel and gp_fit_finish_kernel form them."""
    Xp, M, alpha, live = factor_state(X, y, ell, sf2, sn2, inert) if state is None else state
    y = np.asarray(y, dtype=np.float64)
    npad = Xp.shape[0]
    nt = npad // 16
    linvT = np.ascontiguousarray(M.T)
    t = lambda i: slice(16 * i, 16 * i + 16)   # noqa: E731
    c = -0.5 / (ell * ell)
    tot = np.zeros(3)
    for I in range(nt):
        for J in range(I + 1):
            kinv = np.zeros((16, 16))
            for k in range(I, nt):
                kinv += linvT[t(I), t(k)] @ linvT[t(J), t(k)].T
            W = np.outer(alpha[t(I)], alpha[t(J)]) - kinv
            D2 = ((Xp[t(I), None, :] - Xp[None, t(J), :]) ** 2).sum(-1)
            WE = W * np.exp(c * D2)
            twice = 1.0 if I == J else 2.0
            tot += np.array([twice * (WE * D2).sum(), twice * WE.sum(), np.trace(W) if I == J else 0.0])
    n = len(y)
    rows = np.flatnonzero(live[:n])
    nl = float(len(rows))
    logm = np.log(np.diag(M)[rows]).sum()
    ya = float(y[rows] @ alpha[rows])
    val = (-0.5 * ya + logm - 0.5 * nl * math.log(2 * math.pi)) / nl
    h = 0.5 / nl
    return val, np.array([h * (sf2 / ell**3) * tot[0], h * tot[1], h * tot[2]])


def reference_ld(X, y, ell, sf2, sn2):
    """(MLL / n, gradient (3,)) as float64 roundings of an np.longdouble recompute on the live rows."""
    X = _sq(X)
    n = X.shape[0]
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    ell_l, sf2_l, sn2_l = LD(float(ell)), LD(float(sf2)), LD(float(sn2))
    E = R.kernel_ld(X, ell, 1.0, X)
    Xl = X.astype(LD)
    D2 = np.zeros((n, n), dtype=LD)
    for k in range(X.shape[1]):
        df = Xl[:, k, None] - Xl[None, :, k]
        D2 += df * df
    K = sf2_l * E + sn2_l * np.eye(n, dtype=LD)
    L = chol_ld(K)
    Linv = solve_lower_ld(L, np.eye(n, dtype=LD))
    Kinv = Linv.T @ Linv
    a = Kinv @ yl
    two_pi = LD(2) * np.arctan(LD(1)) * LD(4)
    val = (LD(-0.5) * (yl @ a) - np.log(np.diag(L)).sum() - LD(0.5) * n * np.log(two_pi)) / n
    W = np.outer(a, a) - Kinv
    g = np.array([(W * (sf2_l * E * D2 / ell_l**3)).sum(), (W * E).sum(), np.trace(W)], dtype=LD) * (LD(0.5) / n)
    return float(val), g.astype(np.float64)


def yardstick(X, y, ell, sf2, sn2):
    """The parent's path: gpmpc.gp.exact_mll + autograd in float64 on the CPU, the raw-parameter gradient
    divided by softplus' derivative.  Returns (MLL / n, gradient (3,), the hyperparameters the GP object
    holds: the ones every other evaluation of the case must use)."""
    import torch

    from gpmpc.gp import GaussianProcess, exact_mll

    gp = GaussianProcess(torch.tensor(_sq(X)), torch.tensor(np.asarray(y, dtype=np.float64)))
    gp.set_hyperparameters(ell, sf2, sn2)
    hyp = (gp.lengthscale, gp.outputscale, gp.noise)
    for p in gp.parameters():
        p.requires_grad_(True)
    m = exact_mll(gp)
    m.backward()
    g = np.array([float(p.grad) / float(torch.sigmoid(p.detach())) for p in gp.parameters()])
    return float(m.detach()), g, hyp


def errors(val, grad, ref):
    return np.abs(np.r_[val, grad] - np.r_[ref[0], ref[1]])


def ratios(val, grad, yard, ref):
    """Per quantity: (error, floored yardstick error, ratio)."""
    e = errors(val, grad, ref)
    ey = np.maximum(errors(yard[0], yard[1], ref), FLOOR * (1.0 + np.abs(np.r_[ref[0], ref[1]])))
    return e, ey, e / ey


def edge_data(n):
    """Per GP of quad2d: dict(X (n, d), y, ell, Z, d) of problem("quad2d", n) at the controller's lengthscale."""
    from helpers import problem

    _, data, hyp = problem("quad2d", n)
    out = []
    for g, (X, y) in enumerate(data):
        X = _sq(X)
        out.append(dict(X=X, y=np.asarray(y, dtype=np.float64), ell=hyp[g][0], Z=X[: min(n, 8)].copy(), d=X.shape[1]))
    return out
