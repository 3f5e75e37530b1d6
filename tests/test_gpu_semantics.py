"""Semantics of the drop-in surface on the MI355X (through the C ABI):

* stage-0 state rows: an obs outside the box is status 4 (`gpmpc/gpmpc.py:288,296,309-310`),
  on the bound (within the tolerance) it solves; a failed instance keeps its previous iterate,
  returns its first input and recovers on the next step (no NaN poisoning); the drop-in
  ``GPMPC.select_action`` asserts on it like the reference (`gpmpc/gpmpc.py:365`);
* ``GPMPC.reset`` after new GPs starts from a fresh iterate, as the reference's new
  ``AcadosOcpSolver`` (`gpmpc/gpmpc.py:97-108`); with unchanged GPs it keeps the warm start;
* ``MPC(q_mpc, r_mpc)`` solves the OCP with those weights (`gpmpc/mpc.py:42-45`).
"""

import numpy as np
import pytest

from helpers import O, initial_states, lqr, oracle_gps, oracle_step, problem, product_gps

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def test_infeasible_and_nan_obs_fail_without_poisoning():
    torch = _torch()
    from oracle import cpu_ref
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem("quad2d", 60)
    H, B = 12, 4
    mats = lqr(spec)
    gs = BatchSolver(spec, H, B)
    gs.set_gps(product_gps(data, hyp))
    gs.set_tightening(True, 0.95, *mats)
    gs.reset(reset_iterate=True)
    have_ref = cpu_ref.LIB_PATH.exists()
    ref = cpu_ref.CpuRef(spec, H, B, gps=oracle_gps(data, hyp), lqr_mats=mats) if have_ref else None
    traj = spec.reference_trajectory()
    x0, ph = initial_states(spec, traj, B)

    def solve(x, k):
        u = gs.solve(torch.tensor(x, device="cuda"), torch.tensor(ph + k, dtype=torch.int32, device="cuda"))
        if ref is not None:
            ref.step(x, ph + k)
        return u.cpu().numpy(), gs.status.cpu().numpy()

    u, st = solve(x0, 0)
    assert (st == 0).all()
    xp, up, _ = (t.cpu().numpy() for t in gs.solution())
    bad = x0.copy()
    bad[1, 2] = spec.x_hi[2] + 0.1                    # z above the box: infeasible stage-0 row
    bad[2, 0] = np.nan                                # NaN observation
    bad[3, 4] = spec.x_hi[4] - 1e-8                   # theta exactly on its stage-0 bound: feasible
    bad[3, 5] = 0.0                                   # (at rest, so the next stages can stay inside)
    u, st = solve(bad, 1)
    assert st[0] == 0 and st[1] == 4 and st[2] == 4 and st[3] in (0, 2), st
    if ref is not None:
        np.testing.assert_array_equal(st, ref.status)
    x1, u1, _ = (t.cpu().numpy() for t in gs.solution())
    np.testing.assert_array_equal(x1[1:3], xp[1:3])     # failed instances keep the previous iterate
    np.testing.assert_array_equal(u[1:3], up[1:3, 0])   # ... and return its first input
    assert np.isfinite(x1).all() and np.isfinite(u).all()
    u, st = solve(x0, 2)
    assert (st == 0).all() and np.isfinite(u).all(), st
    if ref is not None:
        np.testing.assert_array_equal(st, ref.status)
        x2 = gs.solution()[0].cpu().numpy()
        err = np.abs(x2 - ref.x).max() / (1 + np.abs(ref.x).max())
        assert err <= 1e-5, err


def test_gpmpc_select_action_asserts_on_infeasible_obs():
    _torch()
    from gpmpc.gpmpc import GPMPC

    spec, data, hyp = problem("quad2d", 40)
    ctrl = GPMPC("quad2d", horizon=10, prob=0.95)
    ctrl.set_gaussian_processes(product_gps(data, hyp))
    ctrl.reset()
    x = initial_states(spec, spec.reference_trajectory(), 1)[0][0]
    ctrl.select_action(x)
    bad = x.copy()
    bad[0] = spec.x_hi[0] + 1.0
    with pytest.raises(AssertionError, match="status 4"):
        ctrl.select_action(bad)
    ctrl.select_action(x)   # the controller is usable again


def test_gpmpc_reset_after_new_gps_restarts_the_iterate():
    torch = _torch()
    from gpmpc.gpmpc import GPMPC

    spec, data, hyp = problem("quad2d", 50)
    x = initial_states(spec, spec.reference_trajectory(), 1)[0][0]
    gps = product_gps(data, hyp)

    def run(ctrl, steps):
        out = []
        for _ in range(steps):
            out.append(ctrl.select_action(x))
        return out, int(ctrl.solver.sqp_iter[0])

    fresh = GPMPC("quad2d", horizon=10, prob=0.95)
    fresh.set_gaussian_processes(gps)
    fresh.reset()
    (u_fresh,), it_fresh = run(fresh, 1)

    ctrl = GPMPC("quad2d", horizon=10, prob=0.95)
    ctrl.set_gaussian_processes(gps)
    ctrl.reset()
    run(ctrl, 3)                                     # the iterate now holds a converged solution
    ctrl.set_gaussian_processes(gps)                 # "retrained": the reference rebuilds its solver
    ctrl.reset()
    (u_new,), it_new = run(ctrl, 1)
    np.testing.assert_array_equal(u_new, u_fresh)    # bitwise: same inputs from a zero iterate
    assert it_new == it_fresh
    ctrl.reset()                                     # same GPs: acados keeps its memory
    (u_warm,), it_warm = run(ctrl, 1)
    assert it_warm < it_fresh                        # warm-started from the last solution


def test_mpc_q_r_weights_change_the_solution():
    _torch()
    from gpmpc.mpc import MPC

    spec, _, _ = problem("cartpole", 10)
    H = 10
    traj = spec.reference_trajectory()
    x = initial_states(spec, traj, 1)[0][0]
    q2 = np.array([5.0, 0.5, 2.0, 0.2])
    r2 = np.array([0.02])
    u = {}
    for name, (q, r) in {"default": (spec.q_diag, spec.r_diag), "custom": (q2, r2)}.items():
        ctrl = MPC("cartpole", q_mpc=list(q), r_mpc=list(r), horizon=H)
        ctrl.reset()
        u[name] = ctrl.select_action(x)
        sd = spec.to_dict()
        sd["q_diag"], sd["r_diag"] = np.asarray(q), np.asarray(r)
        orc = O.SQPSolver(sd, O.Dynamics(sd, None), H, O.SQPOptions(qp_tol=1e-10, qp_max_iter=100))
        sp = spec.copy()
        sp.q_diag, sp.r_diag = np.asarray(q), np.asarray(r)
        st, _, _ = oracle_step(sp, orc, None, x, 0, H, traj, None, tighten=False, uh=1e-8)
        assert st == 0
        assert np.abs(u[name] - orc.u[0]).max() <= 1e-4 * (1 + np.abs(orc.u).max()), (name, u[name], orc.u[0])
    assert np.abs(u["default"] - u["custom"]).max() > 1e-3


@pytest.mark.parametrize("model,H,n", [("quad2d", 30, 200), ("quad3d", 15, 60), ("quad2d", 33, 60), ("cartpole", 63, 40)])
def test_linearisation_cache_is_bit_exact(model, H, n):
    """The first SQP iteration of a step reads the stored iterate's linearisation (written by the
    step that produced the iterate) instead of recomputing it.  Against a solver with the cache off
    (gpmpc_set_tuning(GPMPC_TUNE_LIN_CACHE, 0)) every output is bit-identical over a closed loop that also re-uploads the
    GPs without a reset, switches the GPs off and on, changes the prior model's parameters, re-uploads
    with a reset, sets the iterate from outside and resets the multipliers (each of which must
    invalidate the cache or leave it valid).  quad2d H = 30 reads the cached rows early, under the
    tightening (the split kernels, H <= 31); quad2d H = 33 and cartpole H = 63 are the non-split
    single-tile kernels, which load them at the first linearisation."""
    torch = _torch()
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem(model, n)
    _, data2, hyp2 = problem(model, n, seed=2)
    B = 16
    mats = lqr(spec)

    def make():
        s = BatchSolver(spec, H, B)
        s.set_gps(product_gps(data, hyp))
        s.set_tightening(True, 0.95, *mats)
        s.reset(reset_iterate=True)
        return s

    on = make()
    off = make()
    off.set_tuning(lin_cache=0)
    traj = spec.reference_trajectory()
    census = (model, H, n) == ("quad2d", 30, 200)   # the loop whose statuses are pinned below
    n_maxiter = []
    x0, ph = initial_states(spec, traj, B)
    x = torch.tensor(x0, device="cuda")
    ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
    for k in range(12):
        if k == 1:
            for s in (on, off):   # new GPs, iterate kept (the cached rows used the old GPs)
                s.set_gps(product_gps(data2, hyp2))
        if k == 2:
            for s in (on, off):   # prior-only model (gpmpc_use_gp(0))
                s.set_gps(None)
        if k == 8:
            for s in (on, off):   # GPs back on
                s.set_gps(product_gps(data, hyp))
        if k == 10:
            for s in (on, off):   # prior model parameters changed (gpmpc_set_model)
                s.set_prior({key: 1.05 * v for key, v in spec.prior.items()})
        if k == 3:
            for s in (on, off):   # new GPs (GPMPC.reset after train_gp)
                s.set_gps(product_gps(data2, hyp2))
                s.reset(reset_iterate=True)
        if k == 5:
            xi, ui, _ = on.solution()
            for s in (on, off):
                s.set_iterate(xi * 0.5, ui)
        if k == 7:
            for s in (on, off):
                s.reset(reset_iterate=False)
        outs = []
        for s in (on, off):
            u = s.solve(x, ts + k).clone()
            outs.append((u, s.status.clone(), s.sqp_iter.clone(), s.qp_iter.clone(), s.res.clone(), *s.solution()[:2]))
        for a, b in zip(*outs):
            assert torch.equal(a, b), k
        if census:
            # a healthy closed loop: every solve ends at status 0 or at the SQP iteration limit (2,
            # accepted by the reference, gpmpc.py:365) -- the latter after the perturbations above, where
            # QPs solved to the NLP tolerance (acados' default) leave a residual just above it
            st = outs[0][1]
            assert ((st == 0) | (st == 2)).all(), (k, st)
            n_maxiter.append(int((st == 2).sum()))
        x = on.plant_step(x, outs[0][0])
    if census:
        # status census of this closed loop at the default tolerances (NLP 1e-6, QP tol = NLP tol):
        # the instance-steps stopped at the SQP iteration limit, pinned exactly: two, both at step 2
        # right after the GPs were switched off (profiles/r5/census_lincache.log)
        print("status-2 instance-steps per step:", n_maxiter)
        assert n_maxiter == LINCACHE_MAXITER_STEPS, n_maxiter


# status-2 (SQP iteration limit) instance-steps per step of test_linearisation_cache_is_bit_exact's
# quad2d loop at the default tolerances
LINCACHE_MAXITER_STEPS = [0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def test_variance_readback_only_after_a_variance_launch():
    """gpmpc_get_variance returns what the last tightening used, or refuses: after a reset (first
    step, no previous solution) the solve runs no variance launch and there is nothing to return;
    after the next step it returns the launch's values (likelihood noise included, so > 0)."""
    torch = _torch()
    from gpmpc import _lib
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem("quad2d", 40)
    H, B = 10, 3
    gs = BatchSolver(spec, H, B)
    gs.set_gps(product_gps(data, hyp))
    gs.set_tightening(True, 0.95, *lqr(spec))
    gs.reset(reset_iterate=True)
    x0, ph = initial_states(spec, spec.reference_trajectory(), B)
    obs = torch.tensor(x0, device="cuda")
    ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.GPMPCError):
        gs.variance()                       # nothing solved yet
    u = gs.solve(obs, ts)                   # first step: no previous solution, no variance launch
    with pytest.raises(_lib.GPMPCError):
        gs.variance()
    gs.plant_step(obs, u, ts, out=obs)
    gs.solve(obs, ts)                       # variance launch at the previous solution
    v = gs.variance().cpu().numpy()
    assert v.shape == (B, H, spec.n_gp) and (v > 0).all()
    gs.reset(reset_iterate=False)
    with pytest.raises(_lib.GPMPCError):
        gs.variance()


@pytest.mark.parametrize("model,H,n,B", [("quad2d", 30, 200, 1100), ("cartpole", 20, 50, 1100), ("quad3d", 12, 60, 300)])
def test_overlapped_step_is_bit_exact(model, H, n, B):
    """A step whose SQP launch needs more than one round of workgroups (more instances than the
    device holds at once: 4 per CU for the one-wave models here, 1 for quad3d) runs as two
    cost-ranked halves, the second half's variance and SQP launches on a side stream beside the
    first half's SQP launch (gpmpc_solve).
    Against a solver with the overlap off (GPMPC_TUNE_OVERLAP 0: one variance launch, then one SQP
    launch) every output, the iterate and the tightening variances are bit-identical over a closed
    loop (the ranking changes from step to step with the instances' costs)."""
    torch = _torch()
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem(model, n)
    mats = lqr(spec)

    def make():
        s = BatchSolver(spec, H, B)
        s.set_gps(product_gps(data, hyp))
        s.set_tightening(True, 0.95, *mats)
        s.reset(reset_iterate=True)
        return s

    on = make()
    off = make()
    off.set_tuning(overlap=0)
    assert on.launch_info()["overlapped"] and not off.launch_info()["overlapped"]
    x0, ph = initial_states(spec, spec.reference_trajectory(), B)
    x = torch.tensor(x0, device="cuda")
    ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
    for k in range(5):
        outs = []
        for s in (on, off):
            u = s.solve(x, ts + k).clone()
            outs.append((u, s.status.clone(), s.sqp_iter.clone(), s.qp_iter.clone(), s.res.clone(), *s.solution()[:2]))
            if k >= 1:
                outs[-1] = outs[-1] + (s.variance().clone(),)
        for a, b in zip(*outs):
            assert torch.equal(a, b), k
        x = on.plant_step(x, outs[0][0], ts + k)
