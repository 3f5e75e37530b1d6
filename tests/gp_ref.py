"""Synthetic GP operands and an extended-precision reference for the GP posterior kernels
(tests/test_gpu_gp_kernels.py; checked on the CPU by tests/test_gp_ref_cpu.py).

Operands.  Training rows and evaluation points are uniform in [-1, 1]^d and the lengthscale is
chosen so that every kernel value lies in [KMIN, 1] sf2; the weights alpha are O(1) with random
signs and the inverse Cholesky factor is a random dense lower-triangular matrix times a known
factor (`reference(frac=...)`).  Every (row, column) product of the contraction then contributes at the
same magnitude: a dropped row panel or column tile moves the variance by about 16/n of sf2, ten
or more orders above the bound below, whereas in a real fit with a short lengthscale most kernel
values are far below any tolerance.

Reference.  From the same float64 inputs, in np.longdouble (x87 80-bit, eps 1.1e-19):
  k_i = sf2 exp(-0.5 |z - x_i|^2 / ell^2),  s_j = sum_i k_i B_ij,
  var = sf2 - sum_j s_j^2 (+ sn2),          mean = sum_i alpha_i k_i
with B = (L^-1)^T, or B = R (n x r) for a LOVE root (var = sf2 - sf2^2 ||R^T e||^2 + sn2, k = sf2 e).

Bound.  A worst-case forward-error bound evaluated by the reference, not a constant:
  tol_var  = 4 (n + 128) eps64 (sf2 + sum_j (sum_i |k_i B_ij|)^2)
  tol_mean = 4 (n + 128) eps64 sum_i |alpha_i k_i|
n eps covers the length-n FMA / MFMA chains (any summation order), 128 eps the kernel value (exp
documented as 1 ulp, plus the rounding of its argument, |x| eps / 2 per operation at |x| <= ~50),
4 is margin.
"""

from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
KMIN = 0.05


def have_extended() -> bool:
    """np.longdouble is wider than float64 by at least 11 bits (x87 extended or better)."""
    return bool(np.finfo(LD).eps < 2e-19)


def lengthscale_for(d: int, kmin: float = KMIN) -> float:
    """ell with exp(-0.5 q / ell^2) >= kmin for every pair of points of [-1, 1]^d (q <= 4 d)."""
    return float(np.sqrt(2.0 * d / np.log(1.0 / kmin)))


def synthetic_gp(n: int, d: int, seed: int, sf2: float = 1.0, sn2: float = 1e-3, alpha_zero: bool = False) -> dict:
    """X (n, d), alpha (n,), Linv (n, n) lower triangular with entries in [-1, 1] (scale 1: see
    `reference`), ell, sf2, sn2."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, d))
    alpha = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    Linv = np.tril(rng.uniform(-1.0, 1.0, (n, n)))
    if alpha_zero:
        alpha = np.zeros(n)
    return dict(X=X, alpha=alpha, Linv=Linv, ell=lengthscale_for(d), sf2=float(sf2), sn2=float(sn2), n=n, d=d)


def synthetic_root(n: int, r: int, seed: int) -> np.ndarray:
    """A dense synthetic LOVE root R (n, r), entries in [-1, 1] (scale 1)."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, r))


def points(P: int, d: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (P, d))


def kernel_ld(X, ell, sf2, Z):
    """k (P, n) in longdouble from float64 X, ell, sf2, Z."""
    Xl, Zl = np.asarray(X, dtype=np.float64).astype(LD), np.asarray(Z, dtype=np.float64).astype(LD)
    q = np.zeros((Zl.shape[0], Xl.shape[0]), dtype=LD)
    for k in range(Xl.shape[1]):
        df = Zl[:, k, None] - Xl[None, :, k]
        q += df * df
    ell = LD(float(ell))
    return LD(float(sf2)) * np.exp(LD(-0.5) * q / (ell * ell))


def reference(X, ell, sf2, Z, alpha=None, B=None, frac=None) -> dict:
    """Extended-precision posterior at Z (P, d) and its error bounds (float64 arrays):
    ``mean`` / ``tol_mean`` when alpha is given, ``var`` (without noise; the kernels add sn2 in one
    more rounding, inside the bound's margin) / ``tol_var`` when B (n, c) is: B = Linv.T for the
    exact variance, B = R for a LOVE root.

    ``frac``: the variance terms are those of ``scale`` * B, where ``scale`` (returned) is the
    largest power of two that keeps sum_j s_j^2 <= frac * sf2 at every point, i.e. the reference
    variance >= (1 - frac) sf2.  A power of two, so the caller's float64 product scale * B is exact
    and is the operand this reference was computed from."""
    k = kernel_ld(X, ell, sf2, Z)
    n = k.shape[1]
    out = {}
    if alpha is not None:
        a = np.asarray(alpha).astype(LD)
        out["mean"] = (k @ a).astype(np.float64)
        out["tol_mean"] = (4.0 * (n + 128) * EPS64 * (np.abs(k) @ np.abs(a))).astype(np.float64)
    if B is not None:
        Bl = np.asarray(B).astype(LD)
        s = k @ Bl
        q = (s * s).sum(1)
        sa = np.abs(k) @ np.abs(Bl)
        qa = (sa * sa).sum(1)
        f = 1.0
        if frac is not None:
            f = float(2.0 ** np.floor(0.5 * np.log2(float(frac * sf2 / q.max()))))
            q, qa = q * LD(f * f), qa * LD(f * f)
        out["scale"] = f
        out["var"] = (LD(float(sf2)) - q).astype(np.float64)
        out["tol_var"] = (4.0 * (n + 128) * EPS64 * (LD(float(sf2)) + qa)).astype(np.float64)
    return out


def numpy64(X, ell, sf2, Z, alpha=None, B=None) -> dict:
    """The same posterior in plain float64 numpy (the bound must cover this evaluation's error)."""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    q = ((Z[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    k = sf2 * np.exp(-0.5 * q / ell**2)
    out = {}
    if alpha is not None:
        out["mean"] = k @ alpha
    if B is not None:
        s = k @ B
        out["var"] = sf2 - (s * s).sum(1)
    return out


def inv_lower_ld(L) -> np.ndarray:
    """Inverse of a lower-triangular float64 matrix by forward substitution in longdouble."""
    L = np.asarray(L, dtype=np.float64).astype(LD)
    n = L.shape[0]
    Li = np.zeros((n, n), dtype=LD)
    for i in range(n):
        Li[i, i] = LD(1) / L[i, i]
        if i:
            Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
    return Li
