"""The SQP/IPM kernel with ACTIVE bounds against both CPU references and a KKT certificate (MI355X only).

Every other solver test starts on the reference trajectory, where no bound is active and every bound
multiplier stays ~1e-13.  The batches of tests/constrained_cases.py start off the reference so that
state and input bounds, lower and upper, tightened and wrapped past the reference's end, are active at
the solutions (tests/test_constrained_cpu.py proves that on the CPU), next to a nominal instance in
the same batch.  Per launch shape and step the GPU is compared

* with the C++ restatement: status and SQP iterations equal, x and u to 1e-6 (1 + |.|);
* with the numpy oracle (dense KKT IPM): x, u, u0 to the same bound and the stage costs as
  tests/test_gpu_parity.py::test_closed_loop_parity does; the tightening to rtol 1e-7 against the
  oracle's propagate_constraint_limits at the previous solution the GPU holds;
* with the certificate of tests/kkt_ref.py on the GPU's own (x, u) and the bounds of its own
  tightening: equality residual and bound violation <= tol, stationarity <= 2 sqrt(n) tol for the
  best multipliers the certificate can find itself.

All sides see the same observations (the plant moves with the oracle's u0).
"""

import numpy as np
import pytest

import constrained_cases as cc
import kkt_ref
from helpers import O, lqr, oracle_gps, product_gps

pytestmark = pytest.mark.gpu

SHAPES = {"quad2d": ((1, 0), (2, 1), (4, 1)), "cartpole": ((1, 0), (2, 1), (4, 1)), "quad3d": ((None, None),)}
RUNS = [pytest.param(c, w, g, id=f"{c.id}-" + ("default" if w is None else f"w{w}s{g}"))
        for c in cc.CASES for w, g in SHAPES[c.model]]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not cc.cpu_ref_built():
        pytest.skip("oracle/lib/libcpuref.so not built")
    return torch


def _solver(case, spec, data, hyp, waves, seg, max_iter=25):
    from gpmpc.solver import BatchSolver

    gs = BatchSolver(spec, case.H, case.B, tol=cc.TOL, qp_tol=cc.QP_TOL, qp_max_iter=cc.QP_MAX_ITER, max_iter=max_iter)
    if waves is not None:
        gs.set_launch(waves=waves)
        gs.set_tuning(seg=seg)
    gs.set_gps(product_gps(data, hyp))
    gs.set_tightening(True, cc.PROB, *lqr(spec))
    gs.reset(reset_iterate=True)
    gs.set_cost_output(True)
    return gs


def _gpu_bounds(sd, tight, nx, nu, H):
    """Stage bounds from the magnitudes the GPU stores (icdf sqrt(var) per stage variable)."""
    sc = -np.concatenate([tight[:, :nx].T, tight[:, :nx].T])          # (2 nx, H+1), as the oracle signs it
    ic = -np.concatenate([tight[:H, nx:].T, tight[:H, nx:].T])
    return O.stage_bounds(sd, sc, ic, -1e-8)


@pytest.mark.parametrize("case,waves,seg", RUNS)
def test_active_bounds_match_references_and_certificate(case, waves, seg):
    torch = _torch()
    spec, data, hyp = cc.case_spec(case)
    sd = spec.to_dict()
    gpo = oracle_gps(data, hyp)
    dyn = O.Dynamics(sd, gpo)
    mats = lqr(spec)
    traj = spec.reference_trajectory()
    nx, nu, H = spec.nx, spec.nu, case.H
    n = H * (nx + nu)
    orun, crun = cc.oracle_run(case.id), cc.cpp_run(case.id)
    gs = _solver(case, spec, data, hyp, waves, seg)
    if waves is not None:
        assert gs.launch_info()["waves"] == waves
    _, phase = cc.case_starts(case, spec)
    prev = [None] * case.B
    for s, (row, (cst, cit, cx, cu)) in enumerate(zip(orun, crun)):
        obs = np.array([o.x0 for o in row])
        u0 = gs.solve(torch.tensor(obs, device="cuda"),
                      torch.tensor(phase + s, dtype=torch.int32, device="cuda")).cpu().numpy()
        st, it = gs.status.cpu().numpy(), gs.sqp_iter.cpu().numpy()
        xs, us, tight = (a.cpu().numpy() for a in gs.solution())
        cost = gs.stage_cost.cpu().numpy()
        for b, (inst, o) in enumerate(zip(case.instances, row)):
            at = (case.id, inst.label, s)
            # ---- the C++ restatement
            assert st[b] == cst[b] == 0, (at, st[b], cst[b])
            assert it[b] == cit[b], (at, it[b], cit[b])
            ex = np.abs(xs[b] - cx[b]).max() / (1 + np.abs(cx[b]).max())
            eu = np.abs(us[b] - cu[b]).max() / (1 + np.abs(cu[b]).max())
            # ---- the certificate on the GPU's own solution and bounds
            win = O.reference_window(traj, inst.phase0 + s, H)
            cert = kkt_ref.certificate(sd, dyn, xs[b], us[b], *_gpu_bounds(sd, tight[b], nx, nu, H), win, x0=o.x0)
            print(f"{at} vs cpp x {ex:.1e} u {eu:.1e}  vs oracle x {np.abs(xs[b] - o.x).max():.1e} "
                  f"u {np.abs(us[b] - o.u).max():.1e}  cert eq {cert.eq:.1e} viol {cert.viol:.1e} stat {cert.stat:.1e} "
                  f"active {int(cert.act_lo.sum())}+{int(cert.act_hi.sum())}")
            assert max(ex, eu) <= 1e-6, (at, ex, eu)
            assert cert.eq <= cc.TOL and cert.viol <= cc.TOL, (at, cert.eq, cert.viol)
            assert cert.stat <= 2 * np.sqrt(n) * cc.TOL, (at, cert.stat)
            # ---- the numpy oracle
            assert o.status == 0, at
            if s not in inst.oracle_weak_steps:   # (there the oracle's solution is no reference, see Instance)
                np.testing.assert_allclose(xs[b], o.x, rtol=0, atol=1e-6 * (1 + np.abs(o.x).max()), err_msg=str(at))
                np.testing.assert_allclose(us[b], o.u, rtol=0, atol=1e-6 * (1 + np.abs(o.u).max()), err_msg=str(at))
                np.testing.assert_allclose(u0[b], o.u[0], rtol=0, atol=1e-6 * (1 + np.abs(o.u).max()), err_msg=str(at))
                co = O.stage_costs(sd, o.x, o.u, traj, inst.phase0 + s)
                np.testing.assert_allclose(cost[b], co, rtol=0, atol=1e-6 * (1.0 + co.sum()), err_msg=str(at))
            # ---- the tightening: the oracle's formula at the previous solution the GPU itself holds (the
            # variance is steep in u: two solutions 3e-7 apart, both within the solver tolerance, move
            # it by 2e-6 relative, so the oracle's own previous solution would blur this comparison)
            sc, ic = o.sc, o.ic
            if prev[b] is not None:
                sc, ic = O.propagate_constraint_limits(sd, gpo, prev[b][0], prev[b][1], *mats, cc.PROB)
            np.testing.assert_allclose(tight[b, :, :nx], -sc[:nx].T, rtol=1e-7, atol=1e-12, err_msg=str(at))
            np.testing.assert_allclose(tight[b, :H, nx:], -ic[:nu].T, rtol=1e-7, atol=1e-12, err_msg=str(at))
            prev[b] = (xs[b].T.copy(), us[b].T.copy())


def _res_tolerances(case_id, steps):
    """Ten times the largest change of the oracle's own res[0] (stationarity) and res[3]
    (complementarity) over the batch when its QP tolerance goes from 1e-11 to 1e-12."""
    a = cc.oracle_run(case_id, cc.TOL, 1e-11, 2, steps)
    b = cc.oracle_run(case_id, cc.TOL, 1e-12, 2, steps)
    d = np.array([[[abs(p.res[i] - q.res[i]) for i in (0, 3)] for p, q in zip(ra, rb)] for ra, rb in zip(a, b)])
    return 10 * d[..., 0].max(), 10 * d[..., 1].max()


@pytest.mark.parametrize("case_id", ["cartpole_u_vx", "quad2d_inputs"])
def test_residual_outputs_match_recomputation_and_oracle(case_id):
    """``res[B][4]`` (stationarity, equality, inequality, complementarity: what decides convergence)
    against something other than itself, on unconverged iterates: two SQP iterations only, so that the
    off-reference instances stop with status 2 and residuals up to 2e-2, over two steps (the second
    with tightening).

    res[:, 1] and res[:, 2] are recomputed from the returned (x, u) with the oracle's dynamics and the
    bounds of the returned tightening, the stage-0 terms of ``SQPSolver.solve`` included, to within
    dt sum_g 1e-10 sf2_g sum|alpha_g| + 1e-12: the bound test_linearisation_gp_mean_grad_matches_oracle
    holds the kernel's GP means to, through f = ... + m_g and one RK4 step.

    res[:, 0] and res[:, 3] depend on the IPM's multipliers and are compared with the oracle's, within
    ten times what the oracle's own values move between QP tolerances 1e-11 and 1e-12 on these
    instances (computed by ``_res_tolerances``; measured: cartpole_u_vx 8.1e-8 and 3.1e-9 on residuals
    of 1e-10..1.8e-5, quad2d_inputs 1.0e-8 and 3.6e-9 on residuals of 4.5e-6..2.2e-2)."""
    torch = _torch()
    steps = 2
    case = cc.BY_ID[case_id]
    spec, data, hyp = cc.case_spec(case)
    sd = spec.to_dict()
    gpo = oracle_gps(data, hyp)
    dyn = O.Dynamics(sd, gpo)
    nx, nu, H = spec.nx, spec.nu, case.H
    orun = cc.oracle_run(case.id, cc.TOL, cc.QP_TOL, 2, steps)
    tol0, tol3 = _res_tolerances(case.id, steps)
    tol_f = spec.dt * sum(1e-10 * g.sf2 * np.abs(g.alpha).sum() for g in gpo) + 1e-12
    gs = _solver(case, spec, data, hyp, None, None, max_iter=2)
    _, phase = cc.case_starts(case, spec)
    for s, row in enumerate(orun):
        obs = np.array([o.x0 for o in row])
        gs.solve(torch.tensor(obs, device="cuda"), torch.tensor(phase + s, dtype=torch.int32, device="cuda"))
        st, res = gs.status.cpu().numpy(), gs.res.cpu().numpy()
        xs, us, tight = (a.cpu().numpy() for a in gs.solution())
        for b, (inst, o) in enumerate(zip(case.instances, row)):
            at = (case.id, inst.label, s)
            assert st[b] == o.status and (o.status == 2 or not inst.kinds), (at, st[b], o.status)
            eq = max(np.abs(dyn.rk4(xs[b, k], us[b, k])[0] - xs[b, k + 1]).max() for k in range(H))
            lbx, ubx, lbu, ubu = _gpu_bounds(sd, tight[b], nx, nu, H)
            w = kkt_ref.pack(xs[b], us[b])
            ineq = max(0.0, (kkt_ref.pack(lbx, lbu) - w).max(), (w - kkt_ref.pack(ubx, ubu)).max(),
                       np.abs(o.x0 - xs[b, 0]).max(), (lbx[0] - xs[b, 0]).max(), (xs[b, 0] - ubx[0]).max())
            print(f"{at} res {res[b]}  eq {eq:.3e} ineq {ineq:.3e}  oracle res {o.res}  tol {tol_f:.1e} {tol0:.1e} {tol3:.1e}")
            assert abs(res[b, 1] - eq) <= tol_f, (at, res[b, 1], eq, tol_f)
            assert abs(res[b, 2] - ineq) <= tol_f, (at, res[b, 2], ineq, tol_f)
            assert abs(res[b, 0] - o.res[0]) <= tol0, (at, res[b, 0], o.res[0], tol0)
            assert abs(res[b, 3] - o.res[3]) <= tol3, (at, res[b, 3], o.res[3], tol3)
