"""Extended-precision exact-GP posterior for the append tests (tests/test_gpu_gp_append.py,
tests/test_gpu_online_learning.py), and their shared error criterion.

From float64 training data (X, y), hyperparameters and points Z, everything in np.longdouble:
K = k(X, X) + sn2 I (gp_ref.kernel_ld), L = chol(K), alpha = L^-T L^-1 y, v = L^-1 k(X, z):
  mean = k(z, X) alpha,   var = sf2 - |v|^2 + sn2 (predictive),   grad = d mean / d z.
The substitutions are done here in longdouble throughout: gp_ref.inv_lower_ld rounds the factor
it is given to float64 first, which would put an error of the size under test into the reference.

Criterion (`worst_ratio`).  The yardstick is the existing upload path, a float64 full recompute
(GaussianProcess.device_layout) fed to set_gps: its worst error over the points against this
reference is e_full.  The appended GP's worst error e_app must be at most 8 e_full: the numpy model
of the bordered update measured 1.6 against a float64 recompute; the margin allows for the MFMA's
summation order and the rounding carried from block to block.
"""

from __future__ import annotations

import numpy as np

import gp_ref as R

LD = R.LD
MARGIN = 8.0


def chol_ld(K):
    n = K.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        s = K[j, j] - L[j, :j] @ L[j, :j]
        assert s > 0
        L[j, j] = np.sqrt(s)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower_ld(L, b):
    x = np.zeros_like(b)
    for i in range(L.shape[0]):
        x[i] = (b[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def solve_upper_ld(U, b):
    x = np.zeros_like(b)
    for i in range(U.shape[0] - 1, -1, -1):
        x[i] = (b[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


def reference(X, y, ell, sf2, sn2, Z) -> dict:
    """mean (P,), predictive var (P,), grad (P, d) as float64 roundings of the longdouble values.
    Asserts var >= sn2 / 2 at every point (callers build the reference before any GPU call)."""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    X, Z = X.reshape(X.shape[0], -1), Z.reshape(Z.shape[0], -1)
    n = X.shape[0]
    K = R.kernel_ld(X, ell, sf2, X) + LD(float(sn2)) * np.eye(n, dtype=LD)
    L = chol_ld(K)
    alpha = solve_upper_ld(L.T, solve_lower_ld(L, np.asarray(y, dtype=np.float64).astype(LD)))
    kz = R.kernel_ld(X, ell, sf2, Z)                 # (P, n)
    v = solve_lower_ld(L, kz.T.copy())               # (n, P)
    var = LD(float(sf2)) - (v * v).sum(0) + LD(float(sn2))
    mean = kz @ alpha
    l2 = LD(float(ell)) ** 2
    grad = np.stack([((kz * alpha[None, :]) * (X[None, :, k].astype(LD) - Z[:, k, None].astype(LD))).sum(1) / l2
                     for k in range(X.shape[1])], axis=1)
    assert float(var.min()) >= 0.5 * sn2, float(var.min())
    return dict(mean=mean.astype(np.float64), var=var.astype(np.float64), grad=grad.astype(np.float64))


def worst_ratio(app, full, ref) -> tuple[float, float, float]:
    """(e_app, e_full, e_app / e_full) of one quantity over the points."""
    e_app = float(np.abs(np.asarray(app) - ref).max())
    e_full = float(np.abs(np.asarray(full) - ref).max())
    ratio = e_app / e_full if e_full > 0 else (0.0 if e_app == 0 else float("inf"))
    return e_app, e_full, ratio
