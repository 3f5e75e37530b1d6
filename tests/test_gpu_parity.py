"""HIP path vs CPU oracle on identical seeded inputs (MI355X only).

Tolerances (float64 everywhere):
* GP mean: |m_gpu - m_cpu| <= 1e-10 * (sf2 * sum|alpha|)   (summation order only)
* GP variance: |v_gpu - v_cpu| <= 1e-9 * sf2              (explicit L^-1 vs triangular solve)
* SQP solutions, both solved to KKT tolerance 1e-9: |x_gpu - x_cpu| <= 1e-6 (1 + |x_cpu|).
  The oracle solves its QPs on the dense KKT system, the GPU by Riccati recursions, so
  agreement is at the converged NLP solution, not iterate by iterate.
"""

import numpy as np
import pytest

from helpers import (O, fitc_oracle_gps, fitc_weights, initial_states, lqr, oracle_gps, oracle_step, problem,
                     product_gps)

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("name,N", [("quad2d", 200), ("cartpole", 50), ("quad3d", 100), ("quad2d", 1000)])
def test_gp_predict_matches_oracle(name, N):
    torch = _torch()
    spec, data, hyp = problem(name, N)
    gpo = oracle_gps(data, hyp)
    gpp = product_gps(data, hyp)
    rng = np.random.default_rng(7)
    for g in range(spec.n_gp):
        X = data[g][0]
        Z = X[rng.integers(0, N, 300)] + 0.3 * rng.standard_normal((300, X.shape[1]))
        Z = np.vstack([Z, X[:5]])  # points on the training set: variance ~ noise
        m, v = gpp[g].predict(torch.tensor(Z, device="cuda"), with_noise=True)
        m, v = m.cpu().numpy(), v.cpu().numpy()
        mo = gpo[g].mean(Z)
        vo = gpo[g].var(Z, with_noise=True)
        scale = gpo[g].sf2 * np.abs(gpo[g].alpha).sum()
        assert np.abs(m - mo).max() <= 1e-10 * scale, (g, np.abs(m - mo).max(), scale)
        assert np.abs(v - vo).max() <= 1e-9 * gpo[g].sf2, (g, np.abs(v - vo).max())


@pytest.mark.parametrize("name,N,H,B", [("quad2d", 200, 30, 16), ("quad2d", 200, 30, 512), ("quad2d", 200, 30, 1024),
                                         ("cartpole", 50, 20, 256), ("quad2d", 17, 10, 3),
                                         ("quad2d", 60, 63, 3), ("cartpole", 50, 49, 5), ("quad3d", 60, 47, 2)])
def test_tightening_variance_matches_oracle(name, N, H, B):
    """The variance launch of the tightening (gp_var_tri_kernel, or gp_var_split_kernel with the column
    tiles over four waves when the 128-point workgroups would fill at most half the CUs: B = 16, 3 and
    cartpole's 256 here; quad2d at 512 and 1024 keeps one wave per point tile) at the previous
    solution's points, read back
    with gpmpc_get_variance, vs the oracle's variance with the likelihood noise:
    |v - v_oracle| <= 1e-9 sf2.  The last three cases take their B H point counts from long horizons
    (quad2d H = 63: 189, cartpole H = 49: 245, quad3d H = 47, its longest: 94; none a multiple of 16)."""
    torch = _torch()
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem(name, N)
    gpo = oracle_gps(data, hyp)
    gs = BatchSolver(spec, H, B)
    gs.set_gps(product_gps(data, hyp))
    gs.set_tightening(True, 0.95, *lqr(spec))
    gs.reset(reset_iterate=True)
    x0, ph = initial_states(spec, spec.reference_trajectory(), B)
    obs = torch.tensor(x0, device="cuda")
    ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
    gs.solve(obs, ts)                                   # marks a previous solution
    rng = np.random.default_rng(11)
    xs = x0[:, None, :] + 0.1 * rng.standard_normal((B, H + 1, spec.nx))
    us = 0.1 * rng.standard_normal((B, H, spec.nu))
    gs.set_iterate(torch.tensor(xs, device="cuda"), torch.tensor(us, device="cuda"))
    gs.solve(obs, ts)                                   # variance launch at (xs, us)
    v = gs.variance().cpu().numpy()                     # (B, H, n_gp)
    z = np.concatenate([xs[:, :H, :], us], axis=2)      # z_k = [x_k; u_k]
    for g, idx in enumerate(spec.var_inputs):
        vo = gpo[g].var(z[:, :, list(idx)].reshape(B * H, len(idx)), with_noise=True).reshape(B, H)
        err = np.abs(v[:, :, g] - vo).max()
        assert err <= 1e-9 * gpo[g].sf2, (g, err)


@pytest.mark.parametrize("name,N,M", [("quad2d", 200, None), ("quad2d", 17, None), ("cartpole", 50, None),
                                      ("quad3d", 120, 60)])
def test_linearisation_gp_mean_grad_matches_oracle(name, N, M):
    """The SQP linearisation's GP sums (MFMA tile path, centred inputs) vs the oracle's
    mean_grad: |dm| <= 1e-10 sf2 sum|alpha|, |dgrad| <= 1e-9 sf2 sum|alpha| / ell^2."""
    torch = _torch()
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem(name, N)
    gpo = oracle_gps(data, hyp)
    gpp = product_gps(data, hyp)
    fitc = fitc_weights(gpp, M) if M else None
    if fitc is not None:
        gpo = fitc_oracle_gps(gpo, fitc)
    solver = BatchSolver(spec, 10, 1)
    solver.set_gps(gpp, fitc=fitc)
    rng = np.random.default_rng(11)
    for g in range(spec.n_gp):
        X = data[g][0]
        Z = X[rng.integers(0, N, 150)] + 0.3 * rng.standard_normal((150, X.shape[1]))
        Z = np.vstack([Z, X[:3], 50.0 + X[:2]])  # on the data and far away (mean 0)
        m, gr = solver.gp_mean_grad(g, torch.tensor(Z, device="cuda"))
        m, gr = m.cpu().numpy(), gr.cpu().numpy()
        ref = [gpo[g].mean_grad(z) for z in Z]
        mo = np.array([r[0] for r in ref])
        go = np.array([r[1] for r in ref])
        scale = gpo[g].sf2 * np.abs(gpo[g].alpha).sum()
        assert np.abs(m - mo).max() <= 1e-10 * scale, (g, np.abs(m - mo).max(), scale)
        assert np.abs(gr - go).max() <= 1e-9 * scale / gpo[g].ell**2, (g, np.abs(gr - go).max())


def test_gp_predict_edge_cases():
    torch = _torch()
    spec, data, hyp = problem("quad2d", 17)  # n not a multiple of 16: padded rows
    gpp = product_gps(data, hyp)
    gpo = oracle_gps(data, hyp)
    m, v = gpp[1].predict(torch.zeros(0, 3, dtype=torch.float64, device="cuda"))
    assert m.shape == (0,) and v.shape == (0,)
    Z = np.array([[0.1, -0.2, 0.05]])
    m, v = gpp[1].predict(torch.tensor(Z, device="cuda"), with_noise=False)
    np.testing.assert_allclose(m.cpu().numpy(), gpo[1].mean(Z), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(v.cpu().numpy(), gpo[1].var(Z, with_noise=False), rtol=1e-8, atol=1e-12)
    far = np.array([[1e3, 1e3, 1e3]])  # far from the data: mean 0, variance sf2
    m, v = gpp[1].predict(torch.tensor(far, device="cuda"), with_noise=False)
    assert abs(float(m[0])) < 1e-12 and abs(float(v[0]) - hyp[1][1]) < 1e-12
    # further than the reduction of exp_rbf could index before its argument was clamped (the kernel's
    # exponent is -3.75e11 and -3.75e15 here): mean 0 or subnormal-small, variance sf2
    for dist in (1e6, 1e8):
        m, v = gpp[1].predict(torch.full((1, 3), dist, dtype=torch.float64, device="cuda"), with_noise=False)
        assert abs(float(m[0])) < 1e-290 and abs(float(v[0]) - hyp[1][1]) < 1e-12, (dist, float(m[0]), float(v[0]))


@pytest.mark.parametrize("name,N,H,B,steps,M,love", [("quad2d", 200, 30, 4, 3, None, False),
                                                      ("cartpole", 50, 20, 3, 3, None, False),
                                                      ("quad3d", 60, 15, 2, 2, None, False),
                                                      ("quad3d", 120, 40, 1, 2, 60, False),
                                                      ("quad2d", 1000, 30, 2, 2, None, False),
                                                      ("quad2d", 200, 30, 3, 3, None, True),
                                                      ("quad3d", 120, 40, 1, 2, 60, True),
                                                      ("quad2d", 1000, 30, 4, 2, None, "default")])
def test_closed_loop_parity(name, N, H, B, steps, M, love):
    """M: FITC mean on M inducing rows (`gpmpc/gpmpc.py:377-400`, config 5's sparse GP), exact variance.
    love: the tightening variance from the LOVE root (gpytorch fast_pred_var, `gpmpc/gpmpc.py:442-444`;
    True: forced at every size; "default": the solver's default, LOVE above 800 training rows, i.e.
    config 4's N=1000), the oracle's variance from the same root (oracle.love_var)."""
    torch = _torch()
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem(name, N)
    gpo = oracle_gps(data, hyp)
    gpp = product_gps(data, hyp)
    fitc = fitc_weights(gpp, M) if M else None
    if fitc is not None:
        gpo = fitc_oracle_gps(gpo, fitc)
    if love:
        for og, gp in zip(gpo, gpp):
            if love == "default" and N <= 800:
                continue
            R = gp.love_root(100).cpu().numpy()
            og.var = (lambda Z, with_noise=True, og=og, R=R: O.love_var(og, R, Z, with_noise))
    mats = lqr(spec)
    tol = 1e-9
    solver = BatchSolver(spec, H, B, tol=tol, qp_tol=1e-11, qp_max_iter=100)  # tight KKT for parity
    solver.set_gps(gpp, fitc=fitc, variance="love" if love else "exact", love_force=love is True)
    if love == "default":
        assert all(r is not None for r in solver.love_ranks), solver.love_ranks
    solver.set_tightening(True, 0.95, *mats)
    solver.reset(reset_iterate=True)
    solver.set_cost_output(True)
    sd = spec.to_dict()
    opts = O.SQPOptions(tol_stat=tol, tol_eq=tol, tol_ineq=tol, tol_comp=tol, qp_tol=1e-11)
    orc = [O.SQPSolver(sd, O.Dynamics(sd, gpo), H, opts) for _ in range(B)]
    plant = O.Dynamics(sd, None, params=spec.true_params)
    traj = spec.reference_trajectory()
    x0, phase = initial_states(spec, traj, B)
    prev = [None] * B
    for step in range(steps):
        xt = torch.tensor(x0, device="cuda")
        ts = torch.tensor(phase + step, dtype=torch.int32, device="cuda")
        u0 = solver.solve(xt, ts).cpu().numpy()
        st = solver.status.cpu().numpy()
        xs, us, tight = (a.cpu().numpy() for a in solver.solution())
        cost = solver.stage_cost.cpu().numpy()
        for b in range(B):
            so, sc, ic = oracle_step(spec, orc[b], gpo, x0[b], phase[b] + step, H, traj, prev[b], lqr_mats=mats)
            assert st[b] == so == 0, (step, b, st[b], so)
            # stage costs (acados LINEAR_LS, dt-scaled stages, unscaled terminal) of the GPU solution
            # against the same costs of the oracle's solution
            co = O.stage_costs(sd, orc[b].x, orc[b].u, traj, phase[b] + step)
            np.testing.assert_allclose(cost[b], co, rtol=0, atol=1e-6 * (1.0 + co.sum()))
            scale = 1.0 + np.abs(orc[b].x).max()
            np.testing.assert_allclose(xs[b], orc[b].x, rtol=0, atol=1e-6 * scale)
            np.testing.assert_allclose(us[b], orc[b].u, rtol=0, atol=1e-6 * (1 + np.abs(orc[b].u).max()))
            np.testing.assert_allclose(u0[b], orc[b].u[0], rtol=0, atol=1e-6 * (1 + np.abs(orc[b].u).max()))
            # tightening magnitudes: GPU stores icdf*sqrt(var) per stage variable
            np.testing.assert_allclose(tight[b, :, :spec.nx], -sc[:spec.nx].T, rtol=1e-7, atol=1e-12)
            np.testing.assert_allclose(tight[b, :H, spec.nx:], -ic[:spec.nu].T, rtol=1e-7, atol=1e-12)
            prev[b] = (orc[b].x.T.copy(), orc[b].u.T.copy())
        # next observation from the oracle's plant (same obs for both sides)
        for b in range(B):
            x0[b] = plant.rk4(x0[b], orc[b].u[0])[0]


def test_status_codes_and_maxiter():
    torch = _torch()
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem("quad2d", 50)
    solver = BatchSolver(spec, 10, 2, max_iter=1)
    solver.set_gps(product_gps(data, hyp))
    solver.reset(reset_iterate=True)
    traj = spec.reference_trajectory()
    x0, phase = initial_states(spec, traj, 2)
    solver.solve(torch.tensor(x0, device="cuda"), torch.tensor(phase, dtype=torch.int32, device="cuda"))
    st = solver.status.cpu().numpy()
    it = solver.sqp_iter.cpu().numpy()
    assert (st == 2).all() and (it == 1).all(), (st, it)


def test_plant_step_matches_oracle():
    torch = _torch()
    from gpmpc.solver import BatchSolver

    for name in ("quad2d", "quad3d", "cartpole"):
        spec, data, hyp = problem(name, 20)
        solver = BatchSolver(spec, 5, 7)
        rng = np.random.default_rng(3)
        x = spec.reference_trajectory()[:, :7].T + 0.1 * rng.standard_normal((7, spec.nx))
        u = spec.u_eq + 0.05 * rng.standard_normal((7, spec.nu))
        ts = torch.zeros(7, dtype=torch.int32, device="cuda")
        xn = solver.plant_step(torch.tensor(x, device="cuda"), torch.tensor(u, device="cuda"), ts).cpu().numpy()
        dyn = O.Dynamics(spec.to_dict(), None, params=spec.true_params)
        for b in range(7):
            np.testing.assert_allclose(xn[b], dyn.rk4(x[b], u[b])[0], rtol=1e-13, atol=1e-13)
        assert (ts.cpu().numpy() == 1).all()


def test_nominal_mpc_class_matches_oracle():
    """`gpmpc/mpc.py` MPC: prior model only, no tightening, uh = +1e-8, default acados tolerances.
    Compared at the converged solution within the north-star tolerance (1e-4 relative)."""
    torch = _torch()
    from gpmpc.mpc import MPC

    spec, _, _ = problem("cartpole", 10)
    H = 10
    ctrl = MPC("cartpole", horizon=H)
    ctrl.reset()
    sd = spec.to_dict()
    orc = O.SQPSolver(sd, O.Dynamics(sd, None), H, O.SQPOptions(qp_tol=1e-10, qp_max_iter=100))
    plant = O.Dynamics(sd, None, params=spec.true_params)
    traj = spec.reference_trajectory()
    x = initial_states(spec, traj, 1)[0][0]
    for step in range(3):
        u = ctrl.select_action(x)
        st, _, _ = oracle_step(spec, orc, None, x, step, H, traj, None, tighten=False, uh=1e-8)
        assert st == 0
        xs, us, _ = (a.cpu().numpy()[0] for a in ctrl.solver.solution())
        assert np.abs(xs - orc.x).max() <= 1e-4 * (1 + np.abs(orc.x).max())
        assert np.abs(u - orc.u[0]).max() <= 1e-4 * (1 + np.abs(orc.u).max())
        x = plant.rk4(x, u)[0]


def test_gpmpc_class_select_action_matches_oracle():
    """The drop-in `GPMPC.select_action` (B=1, numpy in/out) over a short closed loop."""
    torch = _torch()
    from gpmpc.gpmpc import GPMPC

    spec, data, hyp = problem("quad2d", 120)
    H = 12
    ctrl = GPMPC("quad2d", horizon=H, prob=0.95)
    ctrl.set_gaussian_processes(product_gps(data, hyp))
    ctrl.reset()
    gpo = oracle_gps(data, hyp)
    sd = spec.to_dict()
    orc = O.SQPSolver(sd, O.Dynamics(sd, gpo), H, O.SQPOptions(qp_tol=1e-10, qp_max_iter=100))
    plant = O.Dynamics(sd, None, params=spec.true_params)
    traj = spec.reference_trajectory()
    x = initial_states(spec, traj, 1)[0][0]
    mats = lqr(spec)
    prev = None
    for step in range(3):
        u = ctrl.select_action(x)
        st, _, _ = oracle_step(spec, orc, gpo, x, step, H, traj, prev, lqr_mats=mats)
        assert st == 0
        assert np.abs(u - orc.u[0]).max() <= 1e-4 * (1 + np.abs(orc.u).max()), (step, u, orc.u[0])
        prev = (orc.x.T.copy(), orc.u.T.copy())
        x = plant.rk4(x, u)[0]


@pytest.mark.parametrize("name,N,H,B,steps,var", [("quad3d", 100, 40, 8, 4, "dynamics"), ("quad3d", 100, 40, 8, 3, "reference"),
                                                   ("quad2d", 200, 30, 16, 4, "reference"),
                                                   ("cartpole", 50, 20, 16, 6, "reference")])
def test_closed_loop_parity_vs_cpp_restatement(name, N, H, B, steps, var):
    """GPU vs the C++ CPU restatement (oracle/cpu_ref.cpp) in the same closed loop at KKT tol
    1e-9: identical status and SQP/QP iteration counts, |x_gpu - x_cpu| <= 1e-6 (1 + |x|).
    Covers both tightening-variance input maps (gpmpc_set_var_inputs)."""
    torch = _torch()
    from oracle import cpu_ref
    from gpmpc.solver import BatchSolver

    if not cpu_ref.LIB_PATH.exists():
        pytest.skip("oracle/lib/libcpuref.so not built")
    spec, data, hyp = problem(name, N)
    if var == "dynamics":
        spec.var_inputs = spec.gp_inputs
    gpo, gpp = oracle_gps(data, hyp), product_gps(data, hyp)
    mats = lqr(spec)
    tol = 1e-9
    ref = cpu_ref.CpuRef(spec, H, B, gps=gpo, lqr_mats=mats, tol=tol, qp_tol=1e-11, qp_max_iter=100)
    gs = BatchSolver(spec, H, B, tol=tol, qp_tol=1e-11, qp_max_iter=100)
    gs.set_gps(gpp)
    gs.set_tightening(True, 0.95, *mats)
    gs.reset(reset_iterate=True)
    gs.set_cost_output(True)
    traj = spec.reference_trajectory()
    sd = spec.to_dict()
    x0, phase = initial_states(spec, traj, B)
    plant = O.Dynamics(sd, None, params=spec.true_params)
    for s in range(steps):
        gs.solve(torch.tensor(x0, device="cuda"), torch.tensor(phase + s, dtype=torch.int32, device="cuda"))
        u0 = ref.step(x0, phase + s, threads=4).copy()
        xg, ug, _ = (t.cpu().numpy() for t in gs.solution())
        st = gs.status.cpu().numpy()
        np.testing.assert_array_equal(st, ref.status)
        # stage costs of the GPU solution (kernel) against the same costs of the C++ solution
        cost = gs.stage_cost.cpu().numpy()
        for b in range(B):
            co = O.stage_costs(sd, ref.x[b], ref.u[b], traj, phase[b] + s)
            bound = 1e-6 if st[b] == 0 else 1e-4
            np.testing.assert_allclose(cost[b], co, rtol=0, atol=bound * (1.0 + co.sum()))
        # the same SQP iterations on both sides (the QP counts may differ by an IPM iteration where a
        # residual sits at the 1e-11 QP tolerance)
        np.testing.assert_array_equal(gs.sqp_iter.cpu().numpy(), ref.sqp_iter)
        ok = st == 0   # instances that reach the 1e-9 KKT tolerance (both sides agree on which)
        # every instance-step converges except quad2d's one instance at step 1 that needs more than
        # 25 SQP iterations at this tolerance (tools/status_census.py, profiles/r4/status_census.jsonl)
        if name == "quad2d" and s == 1:
            assert (~ok).sum() <= 1, (s, st)
        else:
            assert ok.all(), (s, st)
        err = np.abs(xg - ref.x).max(axis=(1, 2)) / (1 + np.abs(ref.x).max(axis=(1, 2)))
        assert err[ok].max() <= 1e-6, (s, err[ok].max())
        # instances stopped at the SQP iteration limit (status 2, both sides) ran the same iterations
        # from the same start: their last iterates agree too, at a looser bound (not converged)
        if (~ok).any():
            assert (st[~ok] == 2).all(), (s, st)
            assert err[~ok].max() <= 1e-4, (s, err[~ok].max())
        for b in range(B):
            x0[b] = plant.rk4(x0[b], u0[b])[0]
