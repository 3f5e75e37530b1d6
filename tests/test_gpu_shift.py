"""The one-stage shifted warm start (gpmpc_set_tuning GPMPC_TUNE_SHIFT, ``set_tuning(shift=1)``) on
the MI355X, against the C++ CPU restatement with the same shift restated in numpy
(shift_util.shift_cpuref) and against a handle with the option off.

Every shape recomputes the first linearisation of a shifted solve (the cache has no row for the
duplicated last stage), so the cache test lists every shape as a fallback shape.
"""

import numpy as np
import pytest

from helpers import initial_states, lqr, problem, product_gps
from shift_util import HEADLINE, QP_MAX_ITER, QP_TOL, SMALL, TOL, oracle_loop, rel_gap

pytestmark = pytest.mark.gpu

# shapes whose shifted solves recompute their first linearisation instead of reading cached rows
CACHE_FALLBACK = {("quad2d", 5), ("quad2d", 30), ("cartpole", 11), ("quad3d", 6)}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import cpu_ref

    if not cpu_ref.LIB_PATH.exists():
        pytest.skip("oracle/lib/libcpuref.so not built (make -C oracle)")
    return torch


def _solver(name, N, H, B, tighten, launch=None, **kw):
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem(name, N)
    gs = BatchSolver(spec, H, B, **kw)
    gs.set_gps(product_gps(data, hyp))
    if tighten:
        gs.set_tightening(True, 0.95, *lqr(spec))
    if launch is not None:
        gs.set_launch(launch[0])
        gs.set_tuning(seg=launch[1])
    gs.reset(reset_iterate=True)
    return spec, gs


def _outputs(gs):
    """Everything a solve writes, on the host."""
    x, u, t = gs.solution()
    return {k: v.cpu().numpy().copy() for k, v in dict(x=x, u=u, tight=t, u0=gs.u0, status=gs.status, sqp_iter=gs.sqp_iter,
                                                          qp_iter=gs.qp_iter, res=gs.res).items()}


def _solve(torch, gs, obs, tstep):
    gs.solve(torch.tensor(np.ascontiguousarray(obs), device="cuda"),
             torch.tensor(np.asarray(tstep), dtype=torch.int32, device="cuda"))
    return _outputs(gs)


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(a[k][rows], b[k][rows], equal_nan=True) for k in a)


def _assert_same(a, b, what, rows=slice(None)):
    for k in a:
        np.testing.assert_array_equal(a[k][rows], b[k][rows], err_msg=f"{what}: {k}")


def _driven(torch, gs, loop, steps):
    """Solve `steps` steps on the observations of an oracle loop; the outputs of every step."""
    return [_solve(torch, gs, loop["obs"][s], loop["phase"] + s) for s in range(steps)]


LAUNCHES = [(1, 0), (2, 1), (4, 1)]
PATH_CASES = [(s, l) for s in SMALL[:2] + [HEADLINE] for l in LAUNCHES] + [(SMALL[2], None)]


@pytest.mark.parametrize("shape,launch", PATH_CASES, ids=[f"{s[0]}-H{s[2]}-{'auto' if l is None else f'w{l[0]}'}"
                                                          for s, l in PATH_CASES])
def test_same_start_same_path(shape, launch):
    """One SQP iteration (max_iter = 1: one QP from the start point, status 2), tightening off, GPs
    on: the GPU with shift = 1 lands where the restatement with the numpy shift lands, within the
    project's bound for agreeing solves, 1e-6 (1 + |.|), and at least 1e-3 away from the unshifted
    restatement at every step >= 1 (what fails when the shift is silently not applied).

    Today's behaviour at one iteration, shift = 0 against the unshifted restatement, measured on an
    MI355X over these cases: at most 5.5e-10, so the 1e-6 bound stands."""
    torch = _torch()
    name, N, H, B, steps = shape
    want = oracle_loop(*shape, max_iter=1, shift=True, obs_from=shape)
    plain = oracle_loop(*shape, max_iter=1, obs_from=shape)
    _, gs = _solver(name, N, H, B, False, launch, tol=TOL, qp_tol=QP_TOL, qp_max_iter=QP_MAX_ITER, max_iter=1)
    gs.set_tuning(shift=1)
    got = _driven(torch, gs, want, steps)
    for s in range(steps):
        np.testing.assert_array_equal(got[s]["status"], want["status"][s])
        gap = max(rel_gap(got[s]["x"], want["x"][s]), rel_gap(got[s]["u"], want["u"][s]))
        away = max(rel_gap(got[s]["x"], plain["x"][s]), rel_gap(got[s]["u"], plain["u"][s]))
        print(f"{name} H={H} launch={launch} step {s}: vs shifted oracle {gap:.3e}, vs unshifted oracle {away:.3e}")
        assert gap <= 1e-6, (s, gap)
        if s >= 1:
            assert away >= 1e-3, (s, away)


@pytest.mark.parametrize("shape", SMALL, ids=[s[0] for s in SMALL])
def test_same_nlp(shape):
    """Tightening on, KKT 1e-9: only the start point moves, so the GPU with shift = 1 converges to
    the solution of the *unshifted* restatement (which tightens at the unshifted stored solution,
    as the product does): identical statuses (all 0), x and u within 1e-6 (1 + |.|)."""
    torch = _torch()
    name, N, H, B, steps = shape
    want = oracle_loop(*shape, tighten=True)
    _, gs = _solver(name, N, H, B, True, tol=TOL, qp_tol=QP_TOL, qp_max_iter=QP_MAX_ITER)
    gs.set_tuning(shift=1)
    got = _driven(torch, gs, want, steps)
    for s in range(steps):
        np.testing.assert_array_equal(got[s]["status"], want["status"][s])
        assert (got[s]["status"] == 0).all(), (s, got[s]["status"])
        gap = max(rel_gap(got[s]["x"], want["x"][s]), rel_gap(got[s]["u"], want["u"][s]))
        print(f"{name} step {s}: shift=1 vs unshifted oracle {gap:.3e}, sqp_iter {got[s]['sqp_iter'].tolist()} "
              f"(oracle {want['sqp_iter'][s].tolist()})")
        assert gap <= 1e-6, (s, gap)


def test_eligibility():
    """Only a solve that follows the instance's last good solve by one reference index is shifted:
    everything else is bit-identical to a handle with the option off."""
    torch = _torch()
    name, N, H, B = "quad2d", 60, 5, 8
    spec, on = _solver(name, N, H, B, True)
    _, off = _solver(name, N, H, B, True)
    on.set_tuning(shift=1)
    off.set_tuning(shift=0)
    traj = spec.reference_trajectory()
    L = traj.shape[1]
    x0, ph = initial_states(spec, traj, B)

    def both(obs, t):
        return _solve(torch, on, obs, t), _solve(torch, off, obs, t)

    _assert_same(*both(x0, ph), "first solve after reset")
    _assert_same(*both(x0, ph), "second solve at the same tstep")
    _assert_same(*both(x0, ph + 2), "tstep jumps by 2")
    guess = on.solution()
    for gs in (on, off):
        gs.set_iterate(guess[0], guess[1])
    _assert_same(*both(x0, ph + 3), "the solve after set_iterate")
    bad = x0.copy()
    bad[1, 2] = spec.x_hi[2] + 0.1   # outside the stage-0 box: status 4
    a, b = both(bad, ph + 5)
    assert a["status"][1] == 4 and (np.delete(a["status"], 1) != 4).all(), a["status"]
    _assert_same(a, b, "tstep jumps by 2, one instance failing")
    a, b = both(x0, ph + 6)          # an ordinary + 1 step for every instance but the failed one
    _assert_same(a, b, "the solve after a failed solve", rows=slice(1, 2))
    assert np.isin(a["status"], (0, 2)).all() and np.isin(b["status"], (0, 2)).all()
    for i in [i for i in range(B) if i != 1]:
        assert not np.array_equal(a["x"][i], b["x"][i]), f"instance {i}: an ordinary + 1 step was not shifted"

    # a tstep wrapping from traj_len - 1 to 0 counts as + 1
    for gs in (on, off):
        gs.reset(reset_iterate=True)
    last, first = np.full(B, L - 1), np.zeros(B, dtype=int)
    _assert_same(*both(x0, last), "first solve after reset (at traj_len - 1)")
    a, b = both(x0, first)
    assert np.isin(a["status"], (0, 2)).all() and np.isin(b["status"], (0, 2)).all()
    for i in range(B):
        assert not np.array_equal(a["x"][i], b["x"][i]), f"instance {i}: the wrapping step was not shifted"


CACHE_SHAPES = [("quad2d", 60, 5, 8), ("quad2d", 200, 30, 12), ("cartpole", 40, 11, 8), ("quad3d", 60, 6, 4)]


@pytest.mark.parametrize("name,N,H,B", CACHE_SHAPES, ids=[f"{s[0]}-H{s[2]}" for s in CACHE_SHAPES])
def test_cache_honesty(name, N, H, B):
    """shift = 1 with the linearisation cache on against off over a 5-step closed loop: every output
    bit-identical (a shifted first iteration never reads rows of another iterate), and stats slot 9
    (linearisations computed) tells the truth: every shape is a fallback shape (CACHE_FALLBACK), so
    the two totals are equal."""
    torch = _torch()
    runs, slot9 = [], []
    obs = None
    for cache in (1, 0):
        spec, gs = _solver(name, N, H, B, True)
        gs.set_tuning(shift=1, lin_cache=cache)
        stats = torch.zeros(B, gs.STATS_SLOTS, dtype=torch.int64, device="cuda")
        gs.set_stats(stats)
        x0, ph = initial_states(spec, spec.reference_trajectory(), B)
        x = torch.tensor(x0, device="cuda")
        out = []
        for s in range(5):
            out.append(_solve(torch, gs, x.cpu().numpy(), ph + s))
            x = gs.plant_step(x, gs.u0)
        runs.append(out)
        slot9.append(int(stats[:, 9].sum()))
        total = int(stats[:, 0].sum()) + 5 * B   # an SQP solve of `it` iterations linearises it + 1 times
        if cache == 0:
            assert slot9[-1] == total, (slot9, total)
    for s in range(5):
        _assert_same(runs[0][s], runs[1][s], f"step {s}")
    assert (name, H) in CACHE_FALLBACK
    assert slot9[0] == slot9[1], slot9


def test_default_and_validation():
    """shift = 0 is bit-identical to a handle on which the option was never set; any value other
    than 0 or 1 is refused."""
    torch = _torch()
    from gpmpc import _lib

    name, N, H, B = "quad2d", 60, 5, 8
    spec, never = _solver(name, N, H, B, True)
    _, zero = _solver(name, N, H, B, True)
    zero.set_tuning(shift=1)
    zero.set_tuning(shift=0)
    with pytest.raises(_lib.GPMPCError):
        zero.set_tuning(shift=2)
    with pytest.raises(_lib.GPMPCError):
        zero.set_tuning(shift=-1)
    x0, ph = initial_states(spec, spec.reference_trajectory(), B)
    x = torch.tensor(x0, device="cuda")
    for s in range(4):
        a = _solve(torch, never, x.cpu().numpy(), ph + s)
        b = _solve(torch, zero, x.cpu().numpy(), ph + s)
        _assert_same(a, b, f"step {s}")
        x = never.plant_step(x, never.u0)


def test_constructor_keyword_reaches_the_solver():
    """``warm_start_shift=True`` through BatchSolver and through GPMPC's solver keywords is
    ``set_tuning(shift=1)``: bit-identical outputs over a short closed loop, and not those of the default."""
    torch = _torch()
    from gpmpc.gpmpc import GPMPC
    from gpmpc.solver import BatchSolver

    name, N, H, B = "quad2d", 60, 5, 4
    spec, data, hyp = problem(name, N)
    mats = lqr(spec)
    handles = []
    for kw, tune in (({"warm_start_shift": True}, None), ({}, 1), ({}, None)):
        gs = BatchSolver(spec, H, B, **kw)
        gs.set_gps(product_gps(data, hyp))
        gs.set_tightening(True, 0.95, *mats)
        if tune is not None:
            gs.set_tuning(shift=tune)
        gs.reset(reset_iterate=True)
        handles.append(gs)
    x0, ph = initial_states(spec, spec.reference_trajectory(), B)
    x = torch.tensor(x0, device="cuda")
    differs = False
    for s in range(3):
        a, b, c = (_solve(torch, gs, x.cpu().numpy(), ph + s) for gs in handles)
        _assert_same(a, b, f"step {s}")
        differs = differs or not _same(a, c)
        x = handles[0].plant_step(x, handles[0].u0)
    assert differs
    ctrl = GPMPC(name, horizon=H, prob=0.95, batch=1, warm_start_shift=True)
    assert ctrl.solver.tuning.get("shift") == 1 and ctrl.prior_ctrl.solver.tuning.get("shift") == 1
    assert GPMPC(name, horizon=H, prob=0.95, batch=1).solver.tuning.get("shift") is None


def test_fewer_sqp_iterations():
    """What the option is for: quad2d N=200 H=30 B=64, 25 closed-loop steps at the shipped
    tolerances.  Every solve ends with status 0 or 2 and the shifted loop runs strictly fewer SQP
    iterations in total (the C++ restatement: 3.02 -> 2.63 per solve)."""
    torch = _torch()
    name, N, H, B, steps = "quad2d", 200, 30, 64, 25
    totals = []
    for shift in (0, 1):
        spec, gs = _solver(name, N, H, B, True)
        gs.set_tuning(shift=shift)
        x0, ph = initial_states(spec, spec.reference_trajectory(), B)
        x = torch.tensor(x0, device="cuda")
        t = torch.tensor(ph, dtype=torch.int32, device="cuda")
        its = torch.zeros(B, dtype=torch.int64, device="cuda")
        ok = torch.ones(B, dtype=torch.bool, device="cuda")
        for s in range(steps):
            gs.solve(x, t)
            its += gs.sqp_iter
            ok &= (gs.status == 0) | (gs.status == 2)
            x = gs.plant_step(x, gs.u0, t)
        assert bool(ok.all())
        totals.append(int(its.sum()))
    print(f"SQP iterations over {steps} x {B} solves: shift=0 {totals[0]} ({totals[0] / steps / B:.3f} per solve), "
          f"shift=1 {totals[1]} ({totals[1] / steps / B:.3f})")
    assert totals[1] < totals[0], totals
