"""CPU reference of gpmpc_rollout: the oracle's RK4 (oracle/gpmpc_oracle.py Dynamics.rk4, the reference's
`gpmpc/gpmpc.py:204-209` over the residual dynamics of `:171-199`) chained over a horizon, and the exact posterior
variance of every GP along the trajectory.

`gps` is a list of oracle GPs (helpers.oracle_gps; with a FITC mean helpers.fitc_oracle_gps for the mean and the
exact GPs for the variance) or None for the prior alone."""

import numpy as np

from helpers import O


def one_step(spec, gps, x, u):
    """x+ [P][nx] of one RK4 step from x [P][nx] under u [P][nu]."""
    dyn = O.Dynamics(spec.to_dict(), gps)
    return np.array([dyn.rk4(np.asarray(xi, dtype=np.float64), np.asarray(ui, dtype=np.float64))[0] for xi, ui in zip(x, u)])


def rollout(spec, gps, x0, u):
    """x [P][T+1][nx]: row 0 is x0, row k+1 one RK4 step from (x_k, u_k)."""
    x0 = np.asarray(x0, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    P, T = u.shape[:2]
    x = np.empty((P, T + 1, spec.nx))
    x[:, 0] = x0
    for k in range(T):
        x[:, k + 1] = one_step(spec, gps, x[:, k], u[:, k])
    return x


def gp_points(spec, x, u):
    """Per GP the inputs z_k[gp_src_g], z_k = [x_k; u_k], k = 0 .. T-1, along x [P][T+1][nx], u [P][T][nu]: [P][T][d_g]."""
    z = np.concatenate([x[:, :-1], u], axis=-1)
    return [z[..., list(idx)] for idx in spec.to_dict()["gp_inputs"]]


def means(spec, gps, x, u):
    """[P][T][n_gp]: the GP means at the trajectory's points."""
    pts = gp_points(spec, x, u)
    return np.stack([np.asarray(gp.mean(Z.reshape(-1, Z.shape[-1]))).reshape(Z.shape[:2]) for gp, Z in zip(gps, pts)], axis=-1)


def variances(spec, exact_gps, x, u):
    """[P][T][n_gp]: the exact posterior variance without likelihood noise at the trajectory's points."""
    pts = gp_points(spec, x, u)
    return np.stack([gp.var(Z.reshape(-1, Z.shape[-1]), with_noise=False).reshape(Z.shape[:2])
                     for gp, Z in zip(exact_gps, pts)], axis=-1)
