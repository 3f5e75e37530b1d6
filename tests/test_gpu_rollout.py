"""gpmpc_rollout on the MI355X: open-loop rollouts of the model the MPC plans with.

Cases (the smallest sizes at which the kernel can go wrong):
  a  quad2d,   17 training rows (two tiles, the second ragged),  P = 3,  T = 4, exact GPs
  b  quad2d,   200 rows,                                         P = 65, T = 6 (crosses a 16- and a 64-lane tile)
  c  cartpole, 50 rows (both GPs state-dependent),               P = 16, T = 5
  d  quad3d,   60 rows, FITC mean over 24 inducing rows,         P = 17, T = 4, exact variance
x0 comes from initial_states and u is drawn near u_eq (sigma 0.1), so the inputs stay where the GPs are non-zero.
The with_gp = 1 kernel has one launch shape (16 trajectories per wavefront) and the with_gp = 0 kernel one (64), so
the independence test reaches every shape with P = 1, 33 and 65.  Each case's handle, inputs and results are
computed once and shared."""

import ctypes
import functools

import numpy as np
import pytest

import gp_update_util as U
import rollout_ref as RR
from helpers import fitc_oracle_gps, fitc_weights, initial_states, oracle_gps, problem, product_gps

pytestmark = pytest.mark.gpu

CASES = {"a": ("quad2d", 17, 3, 4, None), "b": ("quad2d", 200, 65, 6, None), "c": ("cartpole", 50, 16, 5, None),
         "d": ("quad3d", 60, 17, 4, 24)}


class Case:
    def __init__(self, key):
        U.gpu_torch()
        name, N, self.P, self.T, M = CASES[key]
        self.spec, self.data, self.hyp = problem(name, N)
        self.gpp = product_gps(self.data, self.hyp)
        self.exact = oracle_gps(self.data, self.hyp)               # the variance's GPs
        self.fitc = fitc_weights(self.gpp, M) if M else None
        self.gpo = oracle_gps(self.data, self.hyp)                 # the mean's GPs
        if self.fitc is not None:
            self.gpo = fitc_oracle_gps(self.gpo, self.fitc)
        self.x0, _ = initial_states(self.spec, self.spec.reference_trajectory(), self.P)
        rng = np.random.default_rng(100 + N)
        self.u = self.spec.u_eq + 0.1 * rng.standard_normal((self.P, self.T, self.spec.nu))
        self.s = self.handle()

    def handle(self, **kw):
        from gpmpc.solver import BatchSolver

        s = BatchSolver(self.spec, 5, 2)
        s.set_gps(self.gpp, fitc=self.fitc, **kw)
        return s

    @functools.lru_cache(maxsize=None)
    def run(self, with_gp=True, var=False):
        """The case's rollout (numpy; with var a pair), computed once per variant and left unchanged."""
        out = rollout(self.s, self.x0, self.u, with_gp, var)
        for a in (out if var else (out,)):
            a.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def case(key):
    return Case(key)


def rollout(s, x0, u, with_gp=True, var=False):
    torch = U.gpu_torch()
    out = s.rollout(torch.tensor(np.ascontiguousarray(x0), device="cuda"), torch.tensor(np.ascontiguousarray(u), device="cuda"),
                    with_gp=with_gp, var=var)
    return tuple(t.cpu().numpy() for t in out) if var else out.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("key", list(CASES))
def test_one_step_parity_with_the_oracle_from_the_gpus_own_states(key):
    """x_gpu[k+1] against rk4_oracle(x_gpu[k], u[k]) for every k: restarted from the GPU's own states, no error is
    amplified along the horizon.  The GP means enter the state derivative with coefficients of magnitude <= 1 in
    all three models and the tile-path mean is held to 1e-10 sf2 sum|alpha| (test_gpu_parity.py), hence
    |d| <= 1e-10 (1 + |x_ref| + dt sum_g sf2_g sum|alpha_g|)."""
    c = case(key)
    spec = c.spec
    x = c.run(True)
    assert x.shape == (c.P, c.T + 1, spec.nx) and same(x[:, 0], c.x0)
    ref = np.stack([RR.one_step(spec, c.gpo, x[:, k], c.u[:, k]) for k in range(c.T)], axis=1)
    scale = sum(gp.sf2 * np.abs(gp.alpha).sum() for gp in c.gpo)
    bound = 1e-10 * (1.0 + np.abs(ref) + spec.dt * scale)
    err = np.abs(x[:, 1:] - ref)
    print(f"[rollout] case {key}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3e}, "
          f"smallest bound {bound.min():.3e}")
    assert (err <= bound).all(), (key, float((err / bound).max()))
    # the GPs matter here: a rollout that ignored them would fail
    m = RR.means(spec, c.gpo, x, c.u)
    print(f"[rollout] case {key}: GP means along the trajectory up to {np.abs(m).max(axis=(0, 1))}")
    assert np.abs(m).max() > 1e-6
    prior = c.run(False)
    assert same(prior[:, 0], c.x0) and not same(prior, x)
    assert not (np.abs(prior[:, 1:] - ref) <= bound).all()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("with_gp", (True, False))
def test_independence_of_the_batch_and_prefixes_bit_for_bit(with_gp):
    c = case("b")
    x = c.run(with_gp)
    for i in (5, 20, 64):   # (slot 5 of GP tile 0, slot 4 of tile 1, and the first lane of tile 4 / of the prior kernel's second block)
        alone = rollout(c.s, c.x0[i:i + 1], c.u[i:i + 1], with_gp)
        assert same(alone[0], x[i]), i
        last = rollout(c.s, np.vstack([c.x0[:32], c.x0[i:i + 1]]), np.vstack([c.u[:32], c.u[i:i + 1]]), with_gp)
        assert same(last[32], x[i]) and same(last[:32], x[:32]), i
    head = rollout(c.s, c.x0, c.u[:, :2], with_gp)
    tail = rollout(c.s, head[:, -1], c.u[:, 2:], with_gp)
    assert same(head, x[:, :3]) and same(tail, x[:, 2:])
    assert same(rollout(c.s, c.x0, c.u, with_gp), x)   # and the call repeats itself


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("key", ("a", "c", "d"))
def test_prior_rollout_is_the_chain_of_plant_steps(key):
    from gpmpc.solver import BatchSolver

    torch = U.gpu_torch()
    c = case(key)
    spec = c.spec
    x = c.run(False)
    xt = torch.tensor(c.x0, device="cuda")
    ut = torch.tensor(c.u, device="cuda")
    chain = [xt]
    for k in range(c.T):
        chain.append(c.s.plant_step(chain[-1], ut[:, k].contiguous(), params=spec.prior))
    want = torch.stack(chain, dim=1).cpu().numpy()
    assert same(x, want)
    bare = BatchSolver(spec, 5, 2)   # no GP set
    assert same(rollout(bare, c.x0, c.u, with_gp=False), want)


# ------------------------------------------------------------------------------------------------ 4
def _predicted_variances(s, spec, x, u):
    torch = U.gpu_torch()
    out = []
    for g, Z in enumerate(RR.gp_points(spec, x, u)):
        Zt = torch.tensor(np.ascontiguousarray(Z.reshape(-1, Z.shape[-1])), device="cuda")
        out.append(s.gp_predict(g, Zt, with_noise=False, mean=False)[1].cpu().numpy().reshape(Z.shape[:2]))
    return np.stack(out, axis=-1)


@pytest.mark.parametrize("key", ("a", "d"))
def test_variance_is_gp_predicts_bit_for_bit(key):
    c = case(key)
    spec = c.spec
    for with_gp in (True, False):
        x, v = c.run(with_gp, True)
        assert same(x, c.run(with_gp)) and v.shape == (c.P, c.T, spec.n_gp)
        assert same(v, _predicted_variances(c.s, spec, x, c.u)), (key, with_gp)
        want = RR.variances(spec, c.exact, x, c.u)
        assert np.isfinite(v).all() and np.abs(v - want).max() <= 1e-6 * max(gp.sf2 for gp in c.exact)
    if key == "d":   # a LOVE root is ignored
        s = c.handle(variance="love", love_force=True, love_rank=8)
        assert all(r is not None for r in s.love_ranks)
        x, v = rollout(s, c.x0, c.u, True, True)
        assert same(x, c.run(True)) and same(v, c.run(True, True)[1])


# ------------------------------------------------------------------------------------------------ 5
def test_defect_of_a_solved_problem_is_within_the_reported_residual():
    """The B H pairs (x_k, u_k) of a converged solution as one-step rollouts: the shooting defect the rollout sees is at
    most the equality residual the solver reports, plus the rounding between two evaluations of the same map."""
    from gpmpc.solver import BatchSolver

    torch = U.gpu_torch()
    H, B = 5, 8
    spec, data, hyp = problem("quad2d", 28)
    s = BatchSolver(spec, H, B)
    s.set_options(tol=1e-9)
    s.set_gps(product_gps(data, hyp))
    s.reset(reset_iterate=True)
    x0, phase = initial_states(spec, spec.reference_trajectory(), B)
    s.solve(torch.tensor(x0, device="cuda"), torch.tensor(phase, dtype=torch.int32, device="cuda"))
    x, u, _ = s.solution()
    status, res = s.status.cpu().numpy(), s.res.cpu().numpy()
    step = s.rollout(x[:, :-1].reshape(B * H, spec.nx), u.reshape(B * H, 1, spec.nu))
    assert same(step[:, 0].cpu().numpy(), x[:, :-1].reshape(B * H, spec.nx).cpu().numpy())
    xn = x.cpu().numpy()
    defect = np.abs(xn[:, 1:] - step[:, 1].reshape(B, H, spec.nx).cpu().numpy())
    print(f"[rollout] status {status.tolist()}\n[rollout] defect {defect.max(axis=(1, 2))}\n[rollout] res_eq {res[:, 1]}")
    assert (status == 0).any()
    for b in np.flatnonzero(status == 0):
        assert (defect[b] <= res[b, 1] + 1e-10 * (1.0 + np.abs(xn[b, 1:]))).all(), (b, defect[b].max(), res[b, 1])


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("with_gp", (True, False))
def test_a_nan_stays_in_its_trajectory(with_gp):
    c = case("b")
    clean = c.run(with_gp)
    u = c.u.copy()
    u[5, 2] = np.nan
    x = rollout(c.s, c.x0, u, with_gp)
    assert (~np.isfinite(x[5, 3:])).any(axis=-1).all()
    assert same(x[5, :3], clean[5, :3])
    others = np.arange(c.P) != 5
    assert same(x[others], clean[others])


# ------------------------------------------------------------------------------------------------ 7
def test_the_call_waits_for_the_handles_last_call_on_another_stream():
    """A delay and a gpmpc_gp_refactor of GP 1 at a scaled lengthscale on stream A, then the rollout: when it returns
    the delay has ended, and its states and variances are those of the serial run behind the refactorisation."""
    from gpmpc import _lib
    from gpmpc.solver import BatchSolver
    from stream_order_util import DELAY_FLOOR_MS, Delay

    torch = U.gpu_torch()
    g, P, T = 1, 20, 3
    spec, data, hyp = problem("quad2d", 28)
    ell, sf2, sn2 = hyp[g]
    y = torch.tensor(data[g][1], device="cuda")
    ok = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    x0, _ = initial_states(spec, spec.reference_trajectory(), P)
    u = spec.u_eq + 0.1 * np.random.default_rng(9).standard_normal((P, T, spec.nu))
    x0t, ut = torch.tensor(x0, device="cuda"), torch.tensor(u, device="cuda")

    def handle():
        s = BatchSolver(spec, 5, 2)
        s.set_gps(product_gps(data, hyp))
        for k in range(spec.n_gp):
            s.reserve_gp(k, 32)
        return s

    def refactor(s, stream):
        _lib.check(s.lib.gpmpc_gp_refactor(s._h, g, y.data_ptr(), 1.3 * ell, sf2, sn2, ok.data_ptr(), stream))

    s = handle()
    before = rollout(s, x0, u, True, True)
    refactor(s, s._stream())
    torch.cuda.synchronize()
    serial = rollout(s, x0, u, True, True)
    assert ok.cpu().tolist() == [1]
    assert not same(serial[0], before[0]) and not same(serial[1], before[1])
    # the same on two streams: everything staged, then the delay, the writer and the call with no synchronise between
    s = handle()
    A, delay = torch.cuda.Stream(), Delay(torch)
    xo = torch.full((P, T + 1, spec.nx), float("nan"), dtype=torch.float64, device="cuda")
    vo = torch.full((P, T, spec.n_gp), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    delay.queue(A, DELAY_FLOOR_MS)
    end = torch.cuda.Event()
    end.record(A)
    refactor(s, A.cuda_stream)
    pending = not end.query()
    status = s.lib.gpmpc_rollout(s._h, P, T, x0t.data_ptr(), ut.data_ptr(), 1, xo.data_ptr(), vo.data_ptr())
    done = end.query()
    got = (xo.cpu().numpy(), vo.cpu().numpy())   # (the call returned with its work completed: a plain copy reads it)
    torch.cuda.synchronize()
    _lib.check(status)
    assert pending, "the delay had ended before the call was made: it showed nothing"
    assert done, "the call returned while the delay ahead of the refactorisation still ran: it did not wait"
    assert same(got[0], serial[0]) and same(got[1], serial[1])


# ------------------------------------------------------------------------------------------------ 8
def test_refusals_leave_the_outputs_untouched():
    from gpmpc.solver import BatchSolver

    torch = U.gpu_torch()
    c = case("a")
    spec, P, T = c.spec, c.P, c.T
    x0t, ut = torch.tensor(c.x0, device="cuda"), torch.tensor(c.u, device="cuda")
    xo = torch.full((P, T + 1, spec.nx), float("nan"), dtype=torch.float64, device="cuda")
    vo = torch.full((P, T, spec.n_gp), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = c.s.lib

    def call(h, P=P, T=T, x0=True, u=True, with_gp=1, x=True, var=True):
        return lib.gpmpc_rollout(h, P, T, x0t.data_ptr() if x0 else None, ut.data_ptr() if u else None, with_gp,
                                 xo.data_ptr() if x else None, vo.data_ptr() if var else None)

    for kw, cause in ((dict(P=0), b"P, T >= 1"), (dict(P=-2), b"P, T >= 1"), (dict(T=0), b"P, T >= 1"), (dict(T=-1), b"P, T >= 1"),
                      (dict(x0=False), b"null array"), (dict(u=False), b"null array"), (dict(x=False), b"null array"),
                      (dict(with_gp=2), b"with_gp"), (dict(with_gp=-1), b"with_gp"),
                      (dict(P=60_000_000, T=5), b"int32"), (dict(P=1, T=2**31 - 1), b"int32")):
        assert call(c.s._h, **kw) == -1 and cause in lib.gpmpc_last_error(), kw
    assert lib.gpmpc_rollout(None, P, T, x0t.data_ptr(), ut.data_ptr(), 1, xo.data_ptr(), vo.data_ptr()) == -1
    # before gpmpc_set_model
    h = ctypes.c_void_p()
    assert lib.gpmpc_create(spec.model_id, 5, 2, torch.cuda.current_device(), ctypes.byref(h)) == 0
    try:
        for with_gp in (0, 1):
            assert call(h, with_gp=with_gp, var=False) == -3 and b"gpmpc_set_model" in lib.gpmpc_last_error()
    finally:
        lib.gpmpc_destroy(h)
    # the GPs off: none set, or switched off; the variance without a GP, or without its Linv
    fresh = BatchSolver(spec, 5, 2)
    assert call(fresh._h, var=False) == -3 and b"GPs are off" in lib.gpmpc_last_error()
    assert call(fresh._h, with_gp=0) == -3 and b"not set" in lib.gpmpc_last_error()
    fresh.set_gps(c.gpp, with_variance=False)
    assert call(fresh._h) == -3 and b"Linv" in lib.gpmpc_last_error()
    assert call(fresh._h, with_gp=0) == -3 and b"Linv" in lib.gpmpc_last_error()
    fresh.set_gps(c.gpp)
    fresh.set_gps(None)
    assert call(fresh._h, var=False) == -3 and b"GPs are off" in lib.gpmpc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(xo).all() and torch.isnan(vo).all()
    # and the calls go through where nothing is in their way
    assert call(fresh._h, with_gp=0) == 0   # (the GPs are switched off, not gone: the variance reads them)
    assert same(xo.cpu().numpy(), c.run(False)) and same(vo.cpu().numpy(), c.run(False, True)[1])
    fresh.set_gps(c.gpp, with_variance=False)
    xo.fill_(float("nan"))
    torch.cuda.synchronize()
    assert call(fresh._h, var=False) == 0
    assert same(xo.cpu().numpy(), c.run(True))


# ------------------------------------------------------------------------------------------------ 9
@functools.lru_cache(maxsize=None)
def _controller():
    from gpmpc.gpmpc import GPMPC

    U.gpu_torch()
    spec, data, _ = problem("quad2d", 40)
    ctrl = GPMPC("quad2d", horizon=5, batch=8, variance="exact")
    ctrl.train_gp(np.hstack([X for X, _ in data]), np.column_stack([y for _, y in data]), lr=0.05, iterations=20)
    ctrl.reset()
    return spec, ctrl


def test_controller_predicts_trajectories_and_reports_prediction_error():
    from gpmpc.learning import prediction_error, run_evaluation

    spec, ctrl = _controller()
    B, S, h = 8, 12, 4
    x0, phase = initial_states(spec, ctrl.traj, B)
    u = spec.u_eq + 0.1 * np.random.default_rng(4).standard_normal((B, 6, spec.nu))
    for with_gp in (True, False):
        want = rollout(ctrl.solver, x0, u, with_gp, True)
        got = ctrl.predict_trajectory(x0, u, with_gp=with_gp, return_var=True)
        assert same(got[0], want[0]) and same(got[1], want[1])
        assert same(ctrl.predict_trajectory(x0[3], u[3], with_gp=with_gp), want[0][3])
    assert same(ctrl.prior_ctrl.predict_trajectory(x0, u), rollout(ctrl.solver, x0, u, False))
    assert not same(ctrl.predict_trajectory(x0, u), ctrl.predict_trajectory(x0, u, with_gp=False))
    data = run_evaluation(ctrl, x0, S, phase)
    assert data["obs"].shape == (S + 1, B, spec.nx) and data["action"].shape == (S, B, spec.nu)
    for with_gp in (True, False):
        e = prediction_error(ctrl, data, h, with_gp=with_gp)
        assert e.shape == (h, spec.nx) and np.isfinite(e).all()
        sq = np.zeros((h, spec.nx))
        for s in range(S - h + 1):
            xp = ctrl.predict_trajectory(data["obs"][s], data["action"][s:s + h].transpose(1, 0, 2), with_gp=with_gp)
            sq += ((xp[:, 1:] - data["obs"][s + 1:s + h + 1].transpose(1, 0, 2)) ** 2).sum(axis=0)
        want = np.sqrt(sq / ((S - h + 1) * B))
        print(f"[rollout] prediction error, with_gp {with_gp}: {e.max(axis=1)}")
        np.testing.assert_allclose(e, want, rtol=1e-12, atol=0)


def test_learn_reports_both_prediction_curves_when_asked():
    from gpmpc.learning import learn

    spec, ctrl = _controller()
    kw = dict(n_epochs=1, ctrl=ctrl, lr=0.05, gp_iterations=5, seed=5, samples_per_epoch=30, episode_len=6)
    _, test, _ = learn(report_prediction=2, **kw)
    assert "prediction_error" not in test[0]
    pe = test[1]["prediction_error"]
    assert set(pe) == {"gp", "prior"} and all(v.shape == (2, spec.nx) and np.isfinite(v).all() for v in pe.values())
    assert not np.array_equal(pe["gp"], pe["prior"])
