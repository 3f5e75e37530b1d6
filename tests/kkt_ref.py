"""KKT certificate of a solved horizon, independent of any interior-point method.

Given a trajectory (x, u), the stage bounds of ``O.stage_bounds``, the reference window and an
``O.Dynamics``, ``certificate`` measures how far (x, u) is from a KKT point of

    min  sum_k dt/2 |[x_k; u_k] - [xr_k; u_eq]|^2_W + 1/2 |x_H - xr_H|^2_Q
    s.t. x_{k+1} = F(x_k, u_k),  x_0 given,  lb <= [u_0, x_1, ..., u_{H-1}, x_H] <= ub

without using any solver's multipliers:

* ``eq``    max |F(x_k, u_k) - x_{k+1}|, F the oracle's RK4 map;
* ``viol``  the largest bound violation (with ``x0``: also |x0 - x_0| and the stage-0 state rows,
            the terms ``SQPSolver.solve`` adds to its inequality residual);
* ``stat``  min over pi free, lam >= 0 of |g + C' pi + E' lam|_2: g the LINEAR_LS gradient
            (dt-scaled stages, unscaled terminal), C the constraint Jacobian from the RK4 tangent maps
            at (x, u), E the rows of the bounds within ``active_tol`` (-e_i for a lower bound, +e_i for
            an upper one).  Solved as a non-negative least-squares problem with pi = pi+ - pi-.

A solver whose inf-norm stationarity residual is <= tol with multipliers that vanish off the active
set has stat <= sqrt(n) tol, n = H (nx + nu); the tests allow 2 sqrt(n) tol.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.optimize

ACTIVE_TOL = 1e-6


@dataclass
class Certificate:
    eq: float
    viol: float
    stat: float
    act_lo: np.ndarray     # (n,) bool, d layout [u_0, x_1, ..., u_{H-1}, x_H]
    act_hi: np.ndarray


def pack(x, u):
    """[u_0, x_1, u_1, ..., u_{H-1}, x_H] from x (H+1, nx), u (H, nu) (the oracle's layout)."""
    return np.concatenate([np.concatenate([u[k], x[k + 1]]) for k in range(u.shape[0])])


def is_state(nx, nu, H):
    """(n,) bool: which entries of the packed layout are states."""
    return np.tile(np.concatenate([np.zeros(nu, bool), np.ones(nx, bool)]), H)


def active_sets(x, u, lbx, ubx, lbu, ubu, active_tol=ACTIVE_TOL):
    H = u.shape[0]
    w = pack(x, u)
    lbw, ubw = pack(lbx[:H + 1], lbu), pack(ubx[:H + 1], ubu)
    return w - lbw <= active_tol, ubw - w <= active_tol


def certificate(sd, dyn, x, u, lbx, ubx, lbu, ubu, win, x0=None, active_tol=ACTIVE_TOL) -> Certificate:
    """sd: ``spec.to_dict()``; win: reference window (nx, H+1); x (H+1, nx), u (H, nu)."""
    x, u = np.asarray(x, float), np.asarray(u, float)
    H, nx, nu = u.shape[0], sd["nx"], sd["nu"]
    nb, n, m = nx + nu, H * (nx + nu), H * nx
    dt = sd["dt"]
    Q, R = np.asarray(sd["q_diag"], float), np.asarray(sd["r_diag"], float)
    w = pack(x, u)
    yref = pack(win.T, np.tile(np.asarray(sd["u_eq"], float), (H, 1)))
    hd = np.concatenate([np.concatenate([dt * R, Q if k == H - 1 else dt * Q]) for k in range(H)])
    g = hd * (w - yref)
    C = np.zeros((m, n))
    eq = 0.0
    for k in range(H):
        F, A, B = dyn.rk4(x[k], u[k])
        eq = max(eq, np.abs(F - x[k + 1]).max())
        rows = slice(k * nx, (k + 1) * nx)
        C[rows, k * nb + nu:(k + 1) * nb] = np.eye(nx)
        C[rows, k * nb:k * nb + nu] = -B
        if k > 0:
            C[rows, (k - 1) * nb + nu:k * nb] = -A
    lbw, ubw = pack(lbx[:H + 1], lbu), pack(ubx[:H + 1], ubu)
    viol = max(0.0, (lbw - w).max(), (w - ubw).max())
    if x0 is not None:
        viol = max(viol, np.abs(x0 - x[0]).max(), (lbx[0] - x[0]).max(), (x[0] - ubx[0]).max())
    act_lo, act_hi = w - lbw <= active_tol, ubw - w <= active_tol
    il, ih = np.flatnonzero(act_lo), np.flatnonzero(act_hi)
    E = np.zeros((n, len(il) + len(ih)))
    E[il, np.arange(len(il))] = -1.0
    E[ih, len(il) + np.arange(len(ih))] = 1.0
    _, stat = scipy.optimize.nnls(np.hstack([C.T, -C.T, E]), -g, maxiter=50 * (2 * m + E.shape[1]))
    return Certificate(float(eq), float(viol), float(stat), act_lo, act_hi)
