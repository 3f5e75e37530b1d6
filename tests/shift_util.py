"""Shared pieces of the shifted-warm-start tests (test_shift_cpu.py, test_gpu_shift.py).

The C++ CPU restatement keeps an instance's iterate and multipliers as numpy arrays between steps
(``CpuRef.x, u, pi, ll, lu``), so the one-stage shift of ``GPMPC_TUNE_SHIFT`` is restated here on
those arrays: stage k takes stage min(k + 1, last).  In the restatement's d layout (H blocks
``[u_k, x_{k+1}]``) that is "block k <- block k + 1, last block kept" for ``ll`` / ``lu``, and the
same for ``pi``.  Valid with the restatement's tightening off only: it tightens at the arrays it is
handed, while the product tightens at the unshifted stored solution.

Every closed loop here is computed once per shape and shared (``oracle_loop`` is cached); callers
must not modify what it returns.
"""

from __future__ import annotations

import functools

import numpy as np

from helpers import O, initial_states, lqr, oracle_gps, problem

# (model, training rows, horizon, batch, closed-loop steps)
SMALL = [("quad2d", 60, 5, 8, 5), ("cartpole", 40, 11, 8, 5), ("quad3d", 60, 6, 4, 4)]
HEADLINE = ("quad2d", 200, 30, 12, 4)
TOL, QP_TOL, QP_MAX_ITER = 1e-9, 1e-11, 100


def shift_cpuref(ref, mask):
    """Move instances ``mask`` of ``ref`` (a CpuRef) up one stage, in place."""
    m = np.asarray(mask, dtype=bool)
    B, H, nb = ref.B, ref.H, ref.spec.nx + ref.spec.nu
    ref.x[m, :-1] = ref.x[m, 1:].copy()      # x_k <- x_{k+1}, x_H kept
    ref.u[m, :-1] = ref.u[m, 1:].copy()      # u_k <- u_{k+1}, u_{H-1} kept
    ref.pi[m, :-1] = ref.pi[m, 1:].copy()
    for lam in (ref.ll, ref.lu):
        blk = lam.reshape(B, H, nb)          # a view: the blocks [u_k, x_{k+1}]
        blk[m, :-1] = blk[m, 1:].copy()


def rel_gap(a, b):
    """max |a - b| / (1 + |b|), elementwise."""
    return float((np.abs(a - b) / (1.0 + np.abs(b))).max())


@functools.lru_cache(maxsize=None)
def oracle_loop(name, N, H, B, steps, max_iter=25, tighten=False, shift=False, obs_from=None):
    """Closed loop of the C++ restatement at KKT 1e-9.  ``obs_from``: the key (a tuple of this
    function's arguments) of the loop whose observations drive this one; None: its own plant.
    Returns obs (steps, B, nx), x (steps, B, H+1, nx), u (steps, B, H, nu), status, sqp_iter (steps, B)."""
    from oracle import cpu_ref

    spec, data, hyp = problem(name, N)
    ref = cpu_ref.CpuRef(spec, H, B, gps=oracle_gps(data, hyp), lqr_mats=lqr(spec) if tighten else None, tol=TOL,
                         qp_tol=QP_TOL, qp_max_iter=QP_MAX_ITER, max_iter=max_iter)
    assert not (shift and tighten), "the numpy shift is valid with the restatement's tightening off only"
    traj = spec.reference_trajectory()
    x0, phase = initial_states(spec, traj, B)
    x0 = x0.copy()
    obs_in = None if obs_from is None else oracle_loop(*obs_from)["obs"]
    plant = O.Dynamics(spec.to_dict(), None, params=spec.true_params)
    out = {k: [] for k in ("obs", "x", "u", "status", "sqp_iter")}
    for s in range(steps):
        if obs_in is not None:
            x0 = obs_in[s].copy()
        if shift and s > 0:
            shift_cpuref(ref, np.isin(out["status"][-1], (0, 2)))
        u0 = ref.step(x0, phase + s, threads=4).copy()
        out["obs"].append(x0.copy())
        for k, v in (("x", ref.x), ("u", ref.u), ("status", ref.status), ("sqp_iter", ref.sqp_iter)):
            out[k].append(v.copy())
        if obs_in is None:
            for b in range(B):
                x0[b] = plant.rk4(x0[b], u0[b])[0]
    res = {k: np.stack(v) for k, v in out.items()}
    res["phase"] = phase
    for v in res.values():
        v.setflags(write=False)
    return res
