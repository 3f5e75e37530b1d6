"""Numpy model of the IPM corrector solved as a delta system (gp-mpc_amd/csrc/sqp_kernel.hip,
SqpKernel kCorrDelta: qp_ipm, mfma4_vector_backward, acl_phase<false>) against the full re-solve
and the dense KKT solve of the Newton system (CPU, no GPU).

The predictor and the corrector of one IPM iteration solve
    min sum_k 1/2 w_k' diag(h_k) w_k + g_k' w_k,   x_{k+1} = A_k x_k + B_k u_k + c_k,   x_0 = 0
with the same h, A, B, c and two gradients g (predictor) and g' (corrector).  One Riccati
factorisation serves both.  The full corrector runs the vector passes with (g', c):
    t_k = P_{k+1} c_k,  vt_k = q_k + K_k' r_k + Acl_k' t_k,  p_k = vt_k + Acl_k' p_{k+1},
    kff_k = -Ru_k^-1 (r_k + B_k' (t_k + p_{k+1})),  affine column B_k kff_k + c_k.
The delta corrector runs them with (g' - g, 0), where t_k = 0 and the terms above that carry t_k
or c_k are not computed at all, and adds the result (dx, du and the dynamics multipliers dpi) to
the predictor's.  Both must agree with the dense KKT solve of (g', c) at the tolerance
tests/test_segment_model_cpu.py uses for its dense-KKT comparison: atol 1e-9 (1 + max |ref|).
"""

import numpy as np
import pytest


def _problem(rng, H, nx, nu):
    A = [np.eye(nx) + 0.1 * rng.standard_normal((nx, nx)) for _ in range(H)]
    B = [0.3 * rng.standard_normal((nx, nu)) for _ in range(H)]
    c = [0.05 * rng.standard_normal(nx) for _ in range(H)]
    h = [np.concatenate([rng.uniform(0.5, 3.0, nx), rng.uniform(0.1, 1.0, nu)]) for _ in range(H + 1)]
    g = [0.2 * rng.standard_normal(nx + nu) for _ in range(H + 1)]
    g2 = [gi + 0.1 * rng.standard_normal(gi.shape) for gi in g]
    return A, B, c, h, g, g2


def _kkt(A, B, c, h, g, H, nx, nu):
    """Dense KKT solve with x_0 = 0: x (H+1, nx), u (H, nu) and the multipliers pi (H, nx) of
    x_{k+1} - A_k x_k - B_k u_k = c_k (Lagrangian ... + pi_k' (x_{k+1} - A_k x_k - B_k u_k - c_k))."""
    nb = nx + nu
    nv, ne = (H + 1) * nb, (H + 1) * nx
    K = np.zeros((nv + ne, nv + ne))
    rhs = np.zeros(nv + ne)
    for k in range(H + 1):
        K[k * nb:(k + 1) * nb, k * nb:(k + 1) * nb] = np.diag(h[k])
        rhs[k * nb:(k + 1) * nb] = -g[k]
    for i in range(nx):
        K[nv + i, i] = K[i, nv + i] = 1.0
    for k in range(H):
        r0 = nv + (k + 1) * nx
        rows = np.zeros((nx, nv))
        rows[:, (k + 1) * nb:(k + 1) * nb + nx] = np.eye(nx)
        rows[:, k * nb:k * nb + nx] = -A[k]
        rows[:, k * nb + nx:(k + 1) * nb] = -B[k]
        K[r0:r0 + nx, :nv] = rows
        K[:nv, r0:r0 + nx] = rows.T
        rhs[r0:r0 + nx] = c[k]
    sol = np.linalg.solve(K, rhs)
    w = sol[:nv].reshape(H + 1, nb)
    return w[:, :nx], w[:H, nx:], sol[nv + nx:].reshape(H, nx)


def _factor(A, B, h, H, nx, nu):
    """P_k (k = 0..H), K_k, Ru_k^-1, Acl_k = A_k + B_k K_k."""
    P = [None] * (H + 1)
    K, Rui, Acl = [None] * H, [None] * H, [None] * H
    P[H] = np.diag(h[H][:nx])
    for k in range(H - 1, -1, -1):
        Ru = np.diag(h[k][nx:]) + B[k].T @ P[k + 1] @ B[k]
        Rui[k] = np.linalg.inv(Ru)
        K[k] = -Rui[k] @ (B[k].T @ P[k + 1] @ A[k])
        Acl[k] = A[k] + B[k] @ K[k]
        Pk = np.diag(h[k][:nx]) + A[k].T @ P[k + 1] @ Acl[k]
        P[k] = 0.5 * (Pk + Pk.T)
    return P, K, Rui, Acl


def _sweep(fac, B, aff, p, kff, H, nx):
    """Forward sweep from dx_0 = 0 with affine columns aff_k, and the step recovery."""
    P, K, _, Acl = fac
    x = np.zeros((H + 1, nx))
    u = np.zeros((H, kff[0].shape[0]))
    pi = np.zeros((H, nx))
    for k in range(H):
        u[k] = K[k] @ x[k] + kff[k]
        x[k + 1] = Acl[k] @ x[k] + aff[k]
        pi[k] = -(P[k + 1] @ x[k + 1] + p[k + 1])
    return x, u, pi


def _solve_full(fac, B, c, g, H, nx):
    """The vector passes of the full solve with gradient g and dynamics residual c."""
    P, K, Rui, Acl = fac
    p = [None] * (H + 1)
    kff, aff = [None] * H, [None] * H
    p[H] = g[H][:nx].copy()
    for k in range(H - 1, -1, -1):
        q, r = g[k][:nx], g[k][nx:]
        t = P[k + 1] @ c[k]
        vt = q + K[k].T @ r + Acl[k].T @ t
        p[k] = vt + Acl[k].T @ p[k + 1]
        kff[k] = -Rui[k] @ (r + B[k].T @ (t + p[k + 1]))
        aff[k] = B[k] @ kff[k] + c[k]
    return _sweep(fac, B, aff, p, kff, H, nx)


def _solve_delta(fac, B, dg, H, nx):
    """The same passes for the gradient change dg with no dynamics residual: no t_k anywhere."""
    _, K, Rui, Acl = fac
    p = [None] * (H + 1)
    kff, aff = [None] * H, [None] * H
    p[H] = dg[H][:nx].copy()
    for k in range(H - 1, -1, -1):
        q, r = dg[k][:nx], dg[k][nx:]
        vt = q + K[k].T @ r
        p[k] = vt + Acl[k].T @ p[k + 1]
        kff[k] = -Rui[k] @ (r + B[k].T @ p[k + 1])
        aff[k] = B[k] @ kff[k]
    return _sweep(fac, B, aff, p, kff, H, nx)


def _close(got, ref):
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9 * (1 + np.abs(ref).max()))


@pytest.mark.parametrize("nx,nu,H", [(6, 2, 3), (6, 2, 30), (4, 1, 11)])
def test_delta_corrector_matches_full_solve_and_dense_kkt(nx, nu, H):
    rng = np.random.default_rng(1000 * H + 10 * nx + nu)
    A, B, c, h, g, g2 = _problem(rng, H, nx, nu)
    fac = _factor(A, B, h, H, nx, nu)          # one factorisation per case
    aff = _solve_full(fac, B, c, g, H, nx)     # predictor
    full = _solve_full(fac, B, c, g2, H, nx)   # corrector, re-solved
    dlt = _solve_delta(fac, B, [b - a for a, b in zip(g, g2)], H, nx)
    comb = tuple(a + d for a, d in zip(aff, dlt))
    ref = _kkt(A, B, c, h, g2, H, nx, nu)
    ref_aff = _kkt(A, B, c, h, g, H, nx, nu)
    assert max(np.abs(d).max() for d in dlt) > 1e-3   # (the change is not a rounding-level one)
    for name, a, f, cb, r, ra in zip(("dx", "du", "dpi"), aff, full, comb, ref, ref_aff):
        print(f"nx={nx} nu={nu} H={H} {name}: |full - kkt| {np.abs(f - r).max():.3e}, "
              f"|affine + delta - kkt| {np.abs(cb - r).max():.3e}, |affine + delta - full| {np.abs(cb - f).max():.3e}, "
              f"scale {np.abs(r).max():.3e}")
        _close(a, ra)
        _close(f, r)
        _close(cb, r)
        _close(cb, f)
