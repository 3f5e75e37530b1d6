"""Solves that FAIL inside the SQP loop: one script for the CPU test (tests/test_failure_exits_cpu.py:
the C++ restatement's verdicts, which are conditions on these inputs) and the GPU test
(tests/test_gpu_failure_exits.py: every compiled variant of the SQP kernel against the restatement
and against a twin handle that gets the clean inputs).

Per shape, B = 8 instances from ``initial_states()``, GPs and tightening on.  ``drive`` runs

    0, 1   two clean warm-up solves (tstep, tstep + 1)
    plant  set_iterate(stored solution, with the NaNs of cases C and D)       [whole batch]
    2      the failing solve (inputs below)
    3      the next solve, clean inputs: A and B+- recover, C and D still hold their NaN
    heal   set_iterate(stored solution, rows of C and D from before the plant) [whole batch]
    4      a clean solve: every instance solves

``set_iterate`` is a whole-batch call that zeroes every instance's multipliers, so the clean run
(the twin) makes the same two calls with its own stored solution unchanged.  Instances 0, 6 and 7
are clean in every run.  The failing solve's inputs:

    A   inst 1  obs[2] = x_hi[2] + 0.1: outside the stage-0 box, refused before the SQP loop
    B+  inst 2  px = x_hi[0] - 1e-3 moving outwards at vx = 0.5 x_hi[1]: the first QP is infeasible
    B-  inst 3  px = x_lo[0] + 1e-3, vx = 0.5 x_lo[1]
                cartpole: the pole angle 1e-3 (B+) and 1e-2 (B-) inside its LOWER bound, falling at 0.7
                of the rate bound.  On the cart position the IPM of the infeasible QP diverges so slowly
                that the iteration at which it is refused hangs on rounding, on the restatement (a change
                of tolerance moves it from 35 to past 200) as on the device (33 to past 200 across the
                launch shapes), and past the IPM limit the step is accepted and the failure moves to a
                later SQP iteration.  The pole's upper bound behaves the same.  These two inputs are the
                ones of a grid (lower bound, 1e-2 / 1e-3 / 1e-4 inside, 0.3 to 0.9 of the rate bound) that
                the restatement and every launch shape of the device refuse in the first QP, at instance 2
                and 3 respectively (profiles/r23/README.md).  Case E keeps the cart position
                (``Options.b_state = 0``): it is about that slow divergence.
    C   inst 4  NaN in the stored u[H // 2]; obs and tstep one step on
    D   inst 5  NaN in the converged stored iterate (``plant``: u_0, u_{H-1} or x_H) and the SAME
                solve again (obs and tstep of solve 1): every finite residual term is converged

The observations are those of the restatement's clean closed loop (its plant moves with its u0);
every backend is driven on them, so no run depends on another's rounding.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from helpers import O, initial_states, lqr, oracle_gps, problem

B = 8
CLEAN = (0, 6, 7)
A, BP, BM, C, D = 1, 2, 3, 4, 5
FAILING, NEXT, HEALED = 2, 3, 4       # indices into what ``drive`` returns
PLANTS = ("u0", "uH", "xH")
# (model, training rows, horizon): H = 32 is the first horizon past the split-lane IPM layout (H + 1 <= 32)
SHAPES = (("quad2d", 60, 5), ("quad2d", 60, 32), ("cartpole", 40, 4), ("cartpole", 40, 32), ("quad3d", 60, 4))
CASE_E_SHAPE = ("cartpole", 40, 32)


@dataclass(frozen=True)
class Options:
    tol: float = 1e-6                 # the shipped NLP tolerance
    qp_tol: float | None = 1e-11      # QPs solved tightly, so that SQP iteration counts do not hang on rounding
    qp_max_iter: int = 200            # out of reach of the failing IPM iteration of B+-
    max_iter: int = 25
    b_state: int | None = None        # of the script, not the solver: see failing_inputs

    def kw(self):
        return dict(tol=self.tol, qp_tol=self.qp_tol, qp_max_iter=self.qp_max_iter, max_iter=self.max_iter)


OPTS = Options()
OPTS_50 = Options(qp_max_iter=50)             # B+- fail at the same IPM iteration as with 200
OPTS_E = Options(qp_max_iter=50, max_iter=5, b_state=0)   # case E: every QP of B+- ends at the IPM limit


def shape_id(shape):
    return f"{shape[0]}-H{shape[2]}"


def plant_nan(x, u, plant):
    """Copies of the stored solution (B, H+1, nx), (B, H, nu) with the NaNs of cases C and D (a batch
    larger than 8 repeats the pattern: instance i plays instance i % 8)."""
    x, u = x.copy(), u.copy()
    H = u.shape[1]
    u[C::B, H // 2, 0] = np.nan
    if plant == "u0":
        u[D::B, 0, 0] = np.nan
    elif plant == "uH":
        u[D::B, H - 1, -1] = np.nan
    elif plant == "xH":
        x[D::B, H, 0] = np.nan
    else:
        raise ValueError(plant)
    return x, u


def failing_inputs(spec, obs_prev, obs_now, t_now, b_state=None):
    """(obs, tstep) of a failing solve from the clean observations of the solve before and of this one.
    ``b_state``: the position state B+- push against its bounds (None: the module docstring's)."""
    o, t = obs_now.copy(), t_now.copy()
    o[A::B, 2] = spec.x_hi[2] + 0.1
    if b_state is None and spec.name == "cartpole":
        o[BP::B, 2], o[BP::B, 3] = spec.x_lo[2] + 1e-3, 0.7 * spec.x_lo[3]
        o[BM::B, 2], o[BM::B, 3] = spec.x_lo[2] + 1e-2, 0.7 * spec.x_lo[3]
    else:
        i = b_state or 0
        o[BP::B, i], o[BP::B, i + 1] = spec.x_hi[i] - 1e-3, 0.5 * spec.x_hi[i + 1]
        o[BM::B, i], o[BM::B, i + 1] = spec.x_lo[i] + 1e-3, 0.5 * spec.x_lo[i + 1]
    o[D::B] = obs_prev[D::B]
    t[D::B] -= 1
    return o, t


def pattern(b, n):
    """The instances of a batch of n that play instance b of the eight."""
    return np.arange(b, n, B)


class CpuBackend:
    """The C++ restatement behind the three calls ``drive`` makes."""

    def __init__(self, shape, opts=OPTS, tighten=True):
        from oracle import cpu_ref

        name, N, H = shape
        self.spec, data, hyp = problem(name, N)
        self.ref = cpu_ref.CpuRef(self.spec, H, B, gps=oracle_gps(data, hyp), lqr_mats=lqr(self.spec) if tighten else None,
                                  **opts.kw())

    def solve(self, obs, tstep):
        r = self.ref
        r.step(obs, tstep, threads=4)
        return {k: getattr(r, k).copy() for k in ("u0", "status", "sqp_iter", "qp_iter", "x", "u", "pi", "ll", "lu", "has_prev")}

    def iterate(self):
        return self.ref.x.copy(), self.ref.u.copy()

    def set_iterate(self, x, u):
        """gpmpc_set_iterate: the iterate of every instance, multipliers zeroed, has_prev kept."""
        r = self.ref
        r.x[:], r.u[:] = x, u
        for m in (r.pi, r.ll, r.lu):
            m[:] = 0.0


def drive(backend, spec, obs, phase, plant=None, b_state=None):
    """The script of the module docstring on ``backend``; ``plant=None`` is the clean run.  ``obs``:
    the five clean observations, or None to generate them (the clean run on the restatement, whose
    plant is the true model).  Returns the five solves' outputs, the iterate handed to the plant call
    under "before" of the failing solve, and (generating) the observations."""
    gen = obs is None
    if gen:
        assert plant is None
        sim = O.Dynamics(spec.to_dict(), None, params=spec.true_params)
        obs = [initial_states(spec, spec.reference_trajectory(), B)[0].copy()]
    out = []

    def step(o, t):
        out.append(backend.solve(np.ascontiguousarray(o), np.ascontiguousarray(t, dtype=np.int32)))
        if gen:
            obs.append(np.stack([sim.rk4(o[b], out[-1]["u0"][b])[0] for b in range(len(o))]))

    step(obs[0], phase)
    step(obs[1], phase + 1)
    x1, u1 = backend.iterate()
    xp, up = plant_nan(x1, u1, plant) if plant else (x1, u1)
    backend.set_iterate(xp, up)
    step(*(failing_inputs(spec, obs[1], obs[2], phase + 2, b_state) if plant else (obs[2], phase + 2)))
    out[-1]["before"] = (xp, up)
    step(obs[3], phase + 3)
    x3, u3 = backend.iterate()
    if plant:
        for b in (C, D):
            x3[b::B], u3[b::B] = x1[b::B], u1[b::B]
    backend.set_iterate(x3, u3)
    out[-1]["before_heal"] = (x3, u3)
    step(obs[4], phase + 4)
    return (out, obs) if gen else out


def cpu_ref_built() -> bool:
    from oracle import cpu_ref

    return cpu_ref.LIB_PATH.exists()


@functools.lru_cache(maxsize=None)
def clean_run(shape, opts=OPTS, tighten=True):
    """The restatement's clean closed loop of a shape: (outputs of the five solves, observations (5, B, nx),
    phase).  Computed once and shared; callers must not modify it."""
    be = CpuBackend(shape, opts, tighten)
    phase = initial_states(be.spec, be.spec.reference_trajectory(), B)[1].astype(np.int32)
    out, obs = drive(be, be.spec, None, phase)
    return out, np.stack(obs[:5]), phase


@functools.lru_cache(maxsize=None)
def planted_run(shape, plant="u0", opts=OPTS, tighten=True):
    """The restatement's verdicts on the planted script, on the clean run's observations.  Shared."""
    _, obs, phase = clean_run(shape, opts, tighten)
    be = CpuBackend(shape, opts, tighten)
    return drive(be, be.spec, obs, phase, plant, opts.b_state)
