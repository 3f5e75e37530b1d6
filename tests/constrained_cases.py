"""Closed loops that start off the reference so that bounds are ACTIVE at the solutions: one table
for the CPU test (tests/test_constrained_cpu.py: numpy oracle vs C++ restatement vs KKT certificate)
and the GPU test (tests/test_gpu_constrained.py).

``initial_states()`` starts every instance on the reference plus N(0, 0.05^2); at those starts no
bound is ever active and every bound multiplier stays ~1e-13, so none of the IPM's multiplier terms
is exercised.  Each case here is one batch: a model, a bounds modifier applied to a ``get_spec()``
copy before it reaches ``BatchSolver``, ``CpuRef`` and ``to_dict()``, the tightening's variance input
map, and instances (phase0, offset from the reference at phase0).  ``kinds`` declares which kinds of
bound (x lower "xl", x upper "xu", u lower "ul", u upper "uu") are active, within 1e-6, at some
solution of that instance; the last instance of every case is nominal (none), so each batch mixes
both.  tests/test_constrained_cpu.py checks the declarations.

Shapes stay at N <= 60, H <= 12, B <= 8 and at most 4 steps.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from helpers import O, lqr, oracle_gps, oracle_step, problem

TOL, QP_TOL, QP_MAX_ITER, PROB = 1e-9, 1e-11, 100, 0.95


@dataclass(frozen=True)
class Instance:
    label: str
    phase0: int
    offset: tuple
    kinds: frozenset = frozenset()
    # steps at which the numpy oracle's own solution stops short of strict complementarity: its IPM ends
    # on the MEAN complementarity, and leaves one bound at a slack above 1e-6 with a multiplier far above
    # tol (their product still under tol).  That solution is itself a few 1e-6 from the KKT point, so at
    # such a step it is no reference: the tests check that this is so, and hold the C++ restatement's
    # solution (CPU test) and the GPU's (GPU test) to the certificate and to each other instead.
    oracle_weak_steps: tuple = ()


@dataclass(frozen=True)
class Case:
    id: str
    model: str
    N: int
    H: int
    bounds: tuple            # ((field, index, value), ...) on x_lo / x_hi / u_lo / u_hi
    var_map: str             # "reference": spec.var_inputs as shipped; "dynamics": = spec.gp_inputs
    instances: tuple
    steps: int = 3

    @property
    def B(self):
        return len(self.instances)


def _k(*names):
    return frozenset(names)


def _box(field, idx, v):
    return ((field + "_lo", idx, -v), (field + "_hi", idx, v))


_Q3 = (0.5, 0, -0.5, 0, -0.3, 0) + (0,) * 6

CASES = (
    # cartpole: force box +-1 and cart speed box +-0.3; the cart starts 0.3 off the reference
    Case("cartpole_u_vx", "cartpole", 40, 11, _box("u", 0, 1.0) + _box("x", 1, 0.3), "reference", (
        Instance("A", 490, (-0.3, 0, 0.05, 0), _k("xu", "uu")),           # window wraps past traj_len
        Instance("B", 240, (0.3, 0, -0.08, 0), _k("xl", "ul")),
        Instance("nominal", 120, (0.01, 0, 0.0, 0)))),
    # quad2d, stock bounds: both inputs saturate on the way back
    Case("quad2d_inputs", "quad2d", 60, 12, (), "reference", (
        Instance("D", 493, (0.6, 0, -0.4, 0, 0, 0), _k("ul", "uu")),      # wraps
        Instance("nominal", 60, (0.02, 0, -0.02, 0, 0, 0)))),
    # quad2d with a pitch box of +-0.12
    Case("quad2d_theta", "quad2d", 60, 12, _box("x", 4, 0.12), "reference", (
        Instance("C2-", 493, (-0.4, 0, 0.3, 0, 0, 0), _k("ul", "uu")),    # wraps
        Instance("C2+", 493, (0.4, 0, 0.3, 0, 0, 0), _k("ul", "uu")),
        Instance("nominal", 60, (0.02, 0, -0.02, 0, 0, 0)))),
    # quad3d, stock bounds, the reference's variance input map
    Case("quad3d_inputs", "quad3d", 60, 8, (), "reference", (
        Instance("F", 0, _Q3, _k("ul", "uu")),
        Instance("nominal", 30, (0.02, 0, -0.02, 0, 0.01, 0) + (0,) * 6))),
    # quad2d with vx <= 0.7: at step 1 the speed bound is active while a slack falls to 1e-14 with the
    # other QP residuals still above 1e-11; before the IPM floored its slacks (kSlackMin) the Riccati
    # recursion lost definiteness there and the feasible QP ended as status 4.  V is the start at which
    # this was found; at its step 1 the oracle leaves the last stage's speed bound at slack 2.9e-6 with
    # multiplier 9.1e-5 (2.9e-6 off in u_11), so V' (1 cm closer, the same failure before the floor)
    # carries every comparison with the oracle at every step.
    Case("quad2d_vx", "quad2d", 60, 12, (("x_hi", 1, 0.7),), "reference", (
        Instance("V", 493, (-0.4, 0, 0.3, 0, 0, 0), _k("xu", "ul", "uu"), oracle_weak_steps=(1,)),   # wraps
        Instance("V'", 493, (-0.39, 0, 0.3, 0, 0, 0), _k("xu", "ul", "uu")),
        Instance("nominal", 125, (0.02, 0, -0.02, 0, 0, 0)))),
    # quad2d with a climb-rate box of +-0.5: a state bound active over most of the horizon, tightened
    Case("quad2d_vz", "quad2d", 60, 12, _box("x", 3, 0.5), "reference", (
        Instance("S+", 60, (0, 0, -0.4, 0, 0, 0), _k("xu", "ul", "uu")),
        Instance("S-", 60, (0, 0, 0.4, 0, 0, 0), _k("xl", "ul")),
        Instance("nominal", 60, (0.02, 0, -0.02, 0, 0, 0)))),
    # quad3d with a climb-rate box of +-0.4; the variance map of the dynamics (with the reference's map
    # the quad3d tightening is 0.53 and empties a narrow box)
    Case("quad3d_vz", "quad3d", 60, 8, _box("x", 5, 0.4), "dynamics", (
        Instance("G+", 0, (0, 0, 0, 0, -0.3, 0) + (0,) * 6, _k("xu", "uu")),
        Instance("G-", 0, (0, 0, 0, 0, 0.3, 0) + (0,) * 6, _k("xl", "ul")),
        Instance("nominal", 30, (0.02, 0, -0.02, 0, 0.01, 0) + (0,) * 6))),
)

BY_ID = {c.id: c for c in CASES}


def case_spec(case: Case):
    spec, data, hyp = problem(case.model, case.N)
    for field, idx, v in case.bounds:
        getattr(spec, field)[idx] = v
    if case.var_map == "dynamics":
        spec.var_inputs = spec.gp_inputs
    return spec, data, hyp


def case_starts(case: Case, spec):
    traj = spec.reference_trajectory()
    phase = np.array([i.phase0 for i in case.instances], dtype=np.int32)
    x0 = traj[:, phase].T + np.array([i.offset for i in case.instances], dtype=np.float64)
    return x0, phase


@dataclass
class OracleStep:
    x0: np.ndarray          # (nx,) the observation
    status: int
    sqp_iter: int
    x: np.ndarray           # (H+1, nx)
    u: np.ndarray           # (H, nu)
    ll: np.ndarray          # (n,) the oracle's bound multipliers, d layout
    lu: np.ndarray
    res: tuple
    sc: np.ndarray          # tightening (2 nx, H+1), (2 nu, H) as propagate_constraint_limits returns it
    ic: np.ndarray
    bounds: tuple           # (lbx, ubx, lbu, ubu) of stage_bounds


def oracle_options(tol=TOL, qp_tol=QP_TOL, max_iter=25):
    return O.SQPOptions(max_iter=max_iter, tol_stat=tol, tol_eq=tol, tol_ineq=tol, tol_comp=tol, qp_tol=qp_tol,
                        qp_max_iter=QP_MAX_ITER)


def oracle_run(case_id: str, tol: float = TOL, qp_tol: float = QP_TOL, max_iter: int = 25, steps: int | None = None):
    """The numpy oracle's closed loop of a case: [step][instance] -> OracleStep.  The plant moves with
    the oracle's u0.  Computed once per session and shared; callers must not modify it."""
    return _oracle_run(case_id, tol, qp_tol, max_iter, BY_ID[case_id].steps if steps is None else steps)


@functools.lru_cache(maxsize=None)
def _oracle_run(case_id, tol, qp_tol, max_iter, steps):
    case = BY_ID[case_id]
    spec, data, hyp = case_spec(case)
    gpo = oracle_gps(data, hyp)
    mats = lqr(spec)
    sd = spec.to_dict()
    H = case.H
    orc = [O.SQPSolver(sd, O.Dynamics(sd, gpo), H, oracle_options(tol, qp_tol, max_iter)) for _ in range(case.B)]
    plant = O.Dynamics(sd, None, params=spec.true_params)
    traj = spec.reference_trajectory()
    x0, phase = case_starts(case, spec)
    prev = [None] * case.B
    out = []
    for s in range(steps):
        row = []
        for b in range(case.B):
            st, sc, ic = oracle_step(spec, orc[b], gpo, x0[b], int(phase[b]) + s, H, traj, prev[b], prob=PROB,
                                     lqr_mats=mats)
            o = orc[b]
            row.append(OracleStep(x0[b].copy(), st, o.sqp_iter, o.x.copy(), o.u.copy(), o.ll.copy(), o.lu.copy(),
                                  o.res, sc, ic, O.stage_bounds(sd, sc, ic, -1e-8)))
            prev[b] = (o.x.T.copy(), o.u.T.copy())
            x0[b] = plant.rk4(x0[b], o.u[0])[0]
        out.append(row)
    return out


def cpu_ref_built() -> bool:
    from oracle import cpu_ref

    return cpu_ref.LIB_PATH.exists()


def cpp_run(case_id: str, tol: float = TOL, qp_tol: float = QP_TOL, max_iter: int = 25, steps: int | None = None):
    """The C++ restatement (oracle/cpu_ref.cpp) on the oracle's observations of ``oracle_run``:
    [step] -> (status (B,), sqp_iter (B,), x (B, H+1, nx), u (B, H, nu)).  Shared like ``oracle_run``."""
    return _cpp_run(case_id, tol, qp_tol, max_iter, BY_ID[case_id].steps if steps is None else steps)


@functools.lru_cache(maxsize=None)
def _cpp_run(case_id, tol, qp_tol, max_iter, steps):
    from oracle import cpu_ref

    case = BY_ID[case_id]
    spec, data, hyp = case_spec(case)
    ref = cpu_ref.CpuRef(spec, case.H, case.B, gps=oracle_gps(data, hyp), lqr_mats=lqr(spec), prob=PROB, tol=tol,
                         qp_tol=qp_tol, qp_max_iter=QP_MAX_ITER, max_iter=max_iter)
    _, phase = case_starts(case, spec)
    out = []
    for s, row in enumerate(_oracle_run(case_id, tol, qp_tol, max_iter, steps)):
        ref.step(np.array([o.x0 for o in row]), phase + s, threads=2)
        out.append((ref.status.copy(), ref.sqp_iter.copy(), ref.x.copy(), ref.u.copy()))
    return out
