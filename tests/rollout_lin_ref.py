"""CPU reference of gpmpc_rollout_lin, built on rollout_ref.py and the oracle: the per-step Jacobians of the RK4 step
(oracle/gpmpc_oracle.py Dynamics.rk4, the exact tangent recursion) and the covariance recursion
  S_{k+1} = Phi_k S_k Phi_k^T + Bd diag(q_k) Bd^T,  Phi_k = A_k + B_k K  (K None: A_k),
  q_k[j] = dt^2 sum_g W_{j,g}(z_k) (var_{g,k} + noise_g)
with O.variance_weights and spec["unc_dims"]: the tightening's recursion (O.propagate_constraint_limits) in its
closed-loop form, fed per-step matrices."""

import numpy as np

from helpers import O


def jacobians(spec, gps, x, u):
    """x+ [P][nx], A [P][nx][nx], B [P][nx][nu] of one RK4 step from x [P][nx] under u [P][nu]."""
    dyn = O.Dynamics(spec.to_dict(), gps)
    out = [dyn.rk4(np.asarray(xi, dtype=np.float64), np.asarray(ui, dtype=np.float64)) for xi, ui in zip(x, u)]
    return tuple(np.array([o[i] for o in out]) for i in range(3))


def process_noise(spec, x, u, var, noise=None):
    """q [T][n_unc] at the T points z_k = [x_k; u_k] (x [T][nx], u [T][nu]) from var [T][n_gp] and noise [n_gp] or None."""
    sd = spec.to_dict()
    W = O.variance_weights(sd, np.hstack([x, u]))
    v = np.asarray(var, dtype=np.float64) + (0.0 if noise is None else np.asarray(noise, dtype=np.float64)[None, :])
    return np.einsum("tjg,tg->tj", W, v) * sd["dt"] ** 2


def bd(spec):
    return np.eye(spec.nx)[:, spec.to_dict()["unc_dims"]]


def cov_step(spec, S, A, B, K, q):
    """S_{k+1} of one step, and the entrywise sum of the absolute terms |Phi||S||Phi|^T + |Q|."""
    Phi = A if K is None else A + B @ K
    Bd = bd(spec)
    Q = Bd @ np.diag(q) @ Bd.T
    return Phi @ S @ Phi.T + Q, np.abs(Phi) @ np.abs(S) @ np.abs(Phi).T + np.abs(Q)


def cov_recursion(spec, A, B, K, q, cov0=None):
    """S [T+1][nx][nx] of one trajectory from A [T][nx][nx], B [T][nx][nu], q [T][n_unc]."""
    T = len(A)
    S = np.zeros((T + 1, spec.nx, spec.nx))
    if cov0 is not None:
        S[0] = cov0
    for k in range(T):
        S[k + 1] = cov_step(spec, S[k], A[k], B[k], K, q[k])[0]
    return S
