"""gpmpc_rollout_lin on the MI355X: the rollout's Jacobians and the state covariance along it.

Cases (the smallest sizes at which the kernels can go wrong):
  a  quad2d,   17 training rows (two tiles, the second ragged),        P = 3,  T = 4
  b  quad2d,   40 rows (three tiles, odd count),                       P = 17, T = 3 (crosses a 16-trajectory tile)
  c  cartpole, 50 rows (both GPs state-dependent),                     P = 16, T = 5: 5 tangent columns over four lane rows
  d  quad3d,   60 rows, FITC mean over 24 inducing rows,               P = 17, T = 4: 4 columns a lane, the largest footprint
Inputs as in test_gpu_rollout.py: x0 from initial_states, u near u_eq (sigma 0.1).  Both rollout kernels have one launch
shape (16 trajectories per wavefront) and the covariance kernel holds 7, 16 and 1 trajectories per block, so P = 1, 17
and 33 reach every shape.  Each case's handle, inputs and results are computed once and shared."""

import ctypes
import functools
import itertools

import numpy as np
import pytest

import gp_update_util as U
import rollout_lin_ref as LR
from helpers import fitc_oracle_gps, fitc_weights, initial_states, lqr, oracle_gps, problem, product_gps

pytestmark = pytest.mark.gpu

CASES = {"a": ("quad2d", 17, 3, 4, None), "b": ("quad2d", 40, 17, 3, None), "c": ("cartpole", 50, 16, 5, None),
         "d": ("quad3d", 60, 17, 4, 24)}
KEYS = ("x", "A", "B", "var", "cov")


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def lin(s, x0, u, with_gp=True, var=False, cov=False, K=None, cov0=None, with_noise=False):
    torch = U.gpu_torch()
    out = s.rollout_lin(torch.tensor(np.ascontiguousarray(x0), device="cuda"), torch.tensor(np.ascontiguousarray(u), device="cuda"),
                        with_gp=with_gp, var=var, cov=cov, K=K, with_noise=with_noise,
                        cov0=None if cov0 is None else torch.tensor(np.ascontiguousarray(cov0), device="cuda"))
    return {k: v.cpu().numpy() for k, v in out.items()}


def plain(s, x0, u, with_gp=True, var=False):
    torch = U.gpu_torch()
    out = s.rollout(torch.tensor(np.ascontiguousarray(x0), device="cuda"), torch.tensor(np.ascontiguousarray(u), device="cuda"),
                    with_gp=with_gp, var=var)
    return tuple(t.cpu().numpy() for t in out) if var else out.cpu().numpy()


class Case:
    def __init__(self, key):
        U.gpu_torch()
        name, N, self.P, self.T, M = CASES[key]
        self.spec, self.data, self.hyp = problem(name, N)
        self.gpp = product_gps(self.data, self.hyp)
        self.fitc = fitc_weights(self.gpp, M) if M else None
        self.gpo = oracle_gps(self.data, self.hyp)                 # the mean's GPs
        if self.fitc is not None:
            self.gpo = fitc_oracle_gps(self.gpo, self.fitc)
        self.noise = np.array([h[2] for h in self.hyp[:self.spec.n_gp]])
        self.x0, _ = initial_states(self.spec, self.spec.reference_trajectory(), self.P)
        rng = np.random.default_rng(100 + N)
        self.u = self.spec.u_eq + 0.1 * rng.standard_normal((self.P, self.T, self.spec.nu))
        self.K = np.ascontiguousarray(lqr(self.spec)[2])
        L = 0.02 * rng.standard_normal((self.P, self.spec.nx, self.spec.nx))
        c0 = L @ L.transpose(0, 2, 1) + 1e-4 * np.eye(self.spec.nx)
        self.cov0 = np.triu(c0) + np.triu(c0, 1).transpose(0, 2, 1)     # SPD, and symmetric bit for bit
        from gpmpc.solver import BatchSolver

        self.s = BatchSolver(self.spec, 5, 2)
        self.s.set_gps(self.gpp, fitc=self.fitc)

    @functools.lru_cache(maxsize=None)
    def run(self, with_gp=True, closed=True, start=True, with_noise=True):
        """The case's full call (x, A, B, var, cov), computed once per variant and left unchanged."""
        out = lin(self.s, self.x0, self.u, with_gp, True, True, self.K if closed else None, self.cov0 if start else None,
                  with_noise)
        for a in out.values():
            a.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def case(key):
    return Case(key)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("key", list(CASES))
def test_states_and_variances_are_gpmpc_rollouts_bit_for_bit(key):
    c = case(key)
    for with_gp in (True, False):
        x, v = plain(c.s, c.x0, c.u, with_gp, True)
        full = c.run(with_gp)
        assert same(full["x"], x) and same(full["var"], v), (key, with_gp)
        bare = lin(c.s, c.x0, c.u, with_gp)
        assert set(bare) == {"x", "A", "B"} and all(same(bare[k], full[k]) for k in bare), (key, with_gp)
        assert bare["A"].shape == (c.P, c.T, c.spec.nx, c.spec.nx) and bare["B"].shape == (c.P, c.T, c.spec.nx, c.spec.nu)
        assert np.isfinite(bare["A"]).all() and np.isfinite(bare["B"]).all()
    assert not same(c.run(True)["x"], c.run(False)["x"])


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("key", list(CASES))
def test_one_step_jacobian_parity_with_the_oracle_from_the_gpus_own_states(key):
    """A_k, B_k against Dynamics.rk4(x_gpu[k], u[k]) for every k.  J = E + dt/6 sum_s w_s dk_s, and each dk_s is a
    product of the model's partial derivatives (magnitude of the order |J_ref|) with (a) the GP input gradients, which
    the tile path holds to 1e-9 sf2 sum|alpha| / ell^2, and (b) the GP means, which enter the partials with
    coefficients of magnitude <= 1 and are held to 1e-10 sf2 sum|alpha| (test_gpu_parity.py); both enter through the
    step length dt.  Hence entrywise |d| <= 1e-9 (1 + |J_ref| + dt sum_g sf2_g sum|alpha_g| (1 + 1 / ell_g^2))."""
    c = case(key)
    spec = c.spec
    out = c.run(True)
    J = np.concatenate([out["A"], out["B"]], axis=-1)
    ref = []
    for k in range(c.T):
        _, A, B = LR.jacobians(spec, c.gpo, out["x"][:, k], c.u[:, k])
        ref.append(np.concatenate([A, B], axis=-1))
    ref = np.stack(ref, axis=1)
    scale = sum(gp.sf2 * np.abs(gp.alpha).sum() * (1.0 + 1.0 / gp.ell**2) for gp in c.gpo)
    bound = 1e-9 * (1.0 + np.abs(ref) + spec.dt * scale)
    err = np.abs(J - ref)
    print(f"[rollout_lin] case {key}: Jacobian max err {err.max():.3e}, max err / bound {(err / bound).max():.3e}, "
          f"smallest bound {bound.min():.3e}")
    assert (err <= bound).all(), (key, float((err / bound).max()))
    # the GP gradients matter here: the prior's Jacobians fail the same bound
    prior = c.run(False)
    Jp = np.concatenate([prior["A"], prior["B"]], axis=-1)
    print(f"[rollout_lin] case {key}: prior Jacobians off by up to {np.abs(Jp - ref).max():.3e}")
    assert not (np.abs(Jp - ref) <= bound).all()


# ------------------------------------------------------------------------------------------------ 3
def _q(c, out, with_noise):
    return np.stack([LR.process_noise(c.spec, out["x"][p, :-1], c.u[p], out["var"][p], c.noise if with_noise else None)
                     for p in range(c.P)])


@pytest.mark.parametrize("key", list(CASES))
def test_one_step_covariance_parity_from_the_gpus_own_values(key):
    """S_{k+1} against numpy's Phi S_k Phi^T + Bd diag(q_k) Bd^T on the GPU's own S_k, A_k, B_k, var_k, x_k: only the
    order of at most 2 nx + 3 operations per entry differs (gamma ~ 3e-15 at nx = 12); entrywise
    1e-13 (|Phi||S||Phi|^T + |Q|)."""
    c = case(key)
    spec = c.spec
    worst = 0.0
    for closed, start, with_noise in itertools.product((True, False), (True, False), (True, False)):
        out = c.run(True, closed, start, with_noise)
        S = out["cov"]
        assert S.shape == (c.P, c.T + 1, spec.nx, spec.nx) and np.isfinite(S).all()
        assert same(S[:, 0], c.cov0 if start else np.zeros_like(c.cov0))
        assert same(S, np.ascontiguousarray(S.transpose(0, 1, 3, 2))), "every S_k equals its transpose bit for bit"
        assert all(same(out[k], c.run(True)[k]) for k in ("x", "A", "B", "var"))
        q = _q(c, out, with_noise)
        for p in range(c.P):
            for k in range(c.T):
                want, mag = LR.cov_step(spec, S[p, k], out["A"][p, k], out["B"][p, k], c.K if closed else None, q[p, k])
                err = np.abs(S[p, k + 1] - want)
                assert (err <= 1e-13 * mag).all(), (key, closed, start, with_noise, p, k, float((err / mag).max()))
                worst = max(worst, float(np.max(err / np.maximum(mag, 1e-300))))
        assert (np.diagonal(S[:, 1:], axis1=-2, axis2=-1)[..., spec.to_dict()["unc_dims"]] > 0).all()
    print(f"[rollout_lin] case {key}: covariance step max err / scale {worst:.3e}")
    # the options matter
    assert not same(c.run(True, True)["cov"], c.run(True, False)["cov"])
    assert not same(c.run(True, True, True, True)["cov"], c.run(True, True, True, False)["cov"])
    # one step from zero is Bd diag(q_0) Bd^T, exact zeros elsewhere
    for with_noise in (True, False):
        one = lin(c.s, c.x0, c.u[:, :1], True, True, True, c.K, None, with_noise)
        q0 = _q(c, c.run(True), with_noise)[:, 0]
        Q = np.zeros((c.P, spec.nx, spec.nx))
        unc = spec.to_dict()["unc_dims"]
        Q[:, unc, unc] = q0
        assert not one["cov"][:, 0].any() and np.array_equal(one["cov"][:, 1] == 0, Q == 0)
        assert (np.abs(one["cov"][:, 1] - Q) <= 1e-13 * np.abs(Q)).all() and (q0 > 0).all()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("key,with_gp", [("b", True), ("b", False), ("d", True)])
def test_independence_of_the_batch_and_prefixes_bit_for_bit(key, with_gp):
    c = case(key)
    full = c.run(with_gp)
    kw = dict(with_gp=with_gp, var=True, cov=True, K=c.K, with_noise=True)
    for i in (5, 16):   # (a slot inside the first tile, and the first lane of the second)
        alone = lin(c.s, c.x0[i:i + 1], c.u[i:i + 1], cov0=c.cov0[i:i + 1], **kw)
        assert all(same(alone[k][0], full[k][i]) for k in KEYS), (i, "alone")
        for lead in (16, 32):   # last of 17, last of 33
            idx = np.r_[np.arange(lead) % 16, i]
            last = lin(c.s, c.x0[idx], c.u[idx], cov0=c.cov0[idx], **kw)
            assert all(same(last[k][-1], full[k][i]) and same(last[k][:16], full[k][:16]) for k in KEYS), (i, lead)
    head = lin(c.s, c.x0, c.u[:, :2], cov0=c.cov0, **kw)
    assert all(same(head[k], full[k][:, :2]) for k in ("A", "B", "var"))
    assert same(head["x"], full["x"][:, :3]) and same(head["cov"], full["cov"][:, :3])
    # the covariance with the variances kept in the handle's scratch
    torch = U.gpu_torch()
    out = c.s.rollout_lin(torch.tensor(c.x0, device="cuda"), torch.tensor(c.u, device="cuda"), with_gp=with_gp, var=False,
                          cov=True, K=c.K, cov0=torch.tensor(c.cov0, device="cuda"), with_noise=True)
    assert "var" not in out and same(out["cov"].cpu().numpy(), full["cov"])
    again = lin(c.s, c.x0, c.u, cov0=c.cov0, **kw)   # and the call repeats itself
    assert all(same(again[k], full[k]) for k in KEYS)


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("with_gp", (True, False))
def test_a_nan_stays_in_its_trajectory(with_gp):
    c = case("b")
    clean = c.run(with_gp)
    u = c.u.copy()
    p, k = 5, 1
    u[p, k] = np.nan
    out = lin(c.s, c.x0, u, with_gp, True, True, c.K, c.cov0, True)
    others = np.arange(c.P) != p
    for key in ("x", "A", "B", "cov"):
        assert same(out[key][others], clean[key][others]), key
    assert same(out["x"][p, :k + 1], clean["x"][p, :k + 1]) and same(out["cov"][p, :k + 1], clean["cov"][p, :k + 1])
    assert same(out["A"][p, :k], clean["A"][p, :k]) and same(out["B"][p, :k], clean["B"][p, :k])
    assert (~np.isfinite(out["x"][p, k + 1:])).any(axis=-1).all()
    assert (~np.isfinite(out["B"][p, k:])).any(axis=(-2, -1)).all()
    assert (~np.isfinite(out["cov"][p, k + 1:])).any(axis=(-2, -1)).all()


# ------------------------------------------------------------------------------------------------ 6
def test_the_call_waits_for_the_handles_last_call_on_another_stream():
    """A delay and a gpmpc_gp_refactor of GP 1 at a scaled lengthscale on stream A, then the call: when it returns the
    delay has ended, and its outputs are those of the serial run behind the refactorisation."""
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
    K = np.ascontiguousarray(lqr(spec)[2])

    def handle():
        s = BatchSolver(spec, 5, 2)
        s.set_gps(product_gps(data, hyp))
        for k in range(spec.n_gp):
            s.reserve_gp(k, 32)
        return s

    def refactor(s, stream):
        _lib.check(s.lib.gpmpc_gp_refactor(s._h, g, y.data_ptr(), 1.3 * ell, sf2, sn2, ok.data_ptr(), stream))

    s = handle()
    before = lin(s, x0, u, True, True, True, K, None, True)
    refactor(s, s._stream())
    torch.cuda.synchronize()
    serial = lin(s, x0, u, True, True, True, K, None, True)
    assert ok.cpu().tolist() == [1]
    assert not any(same(serial[k], before[k]) for k in KEYS)
    s = handle()
    A, delay = torch.cuda.Stream(), Delay(torch)
    nx, nu = spec.nx, spec.nu
    shapes = dict(x=(P, T + 1, nx), A=(P, T, nx, nx), B=(P, T, nx, nu), var=(P, T, spec.n_gp), cov=(P, T + 1, nx, nx))
    o = {k: torch.full(sh, float("nan"), dtype=torch.float64, device="cuda") for k, sh in shapes.items()}
    torch.cuda.synchronize()
    delay.queue(A, DELAY_FLOOR_MS)
    end = torch.cuda.Event()
    end.record(A)
    refactor(s, A.cuda_stream)
    pending = not end.query()
    status = s.lib.gpmpc_rollout_lin(s._h, P, T, x0t.data_ptr(), ut.data_ptr(), 1, o["x"].data_ptr(), o["A"].data_ptr(),
                                     o["B"].data_ptr(), o["var"].data_ptr(), K.ctypes.data, None, 1, o["cov"].data_ptr())
    done = end.query()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    torch.cuda.synchronize()
    _lib.check(status)
    assert pending, "the delay had ended before the call was made: it showed nothing"
    assert done, "the call returned while the delay ahead of the refactorisation still ran: it did not wait"
    assert all(same(got[k], serial[k]) for k in KEYS)


# ------------------------------------------------------------------------------------------------ 7
def test_refusals_leave_the_outputs_untouched():
    from gpmpc.solver import BatchSolver

    torch = U.gpu_torch()
    c = case("a")
    spec, P, T = c.spec, c.P, c.T
    nx, nu = spec.nx, spec.nu
    x0t, ut, c0t = torch.tensor(c.x0, device="cuda"), torch.tensor(c.u, device="cuda"), torch.tensor(c.cov0, device="cuda")
    shapes = dict(x=(P, T + 1, nx), A=(P, T, nx, nx), B=(P, T, nx, nu), var=(P, T, spec.n_gp), cov=(P, T + 1, nx, nx))
    o = {k: torch.full(sh, float("nan"), dtype=torch.float64, device="cuda") for k, sh in shapes.items()}
    torch.cuda.synchronize()
    lib = c.s.lib
    Kbad = c.K.copy()
    Kbad[1, 2] = np.inf
    Knan = c.K.copy()
    Knan[0, 0] = np.nan

    def call(h, P=P, T=T, x0=True, u=True, with_gp=1, x=True, A=True, B=True, var=True, K=c.K, with_noise=1, cov=True):
        pick = lambda on, t: t.data_ptr() if on else None   # noqa: E731
        return lib.gpmpc_rollout_lin(h, P, T, pick(x0, x0t), pick(u, ut), with_gp, pick(x, o["x"]), pick(A, o["A"]),
                                     pick(B, o["B"]), pick(var, o["var"]), None if K is None else K.ctypes.data,
                                     c0t.data_ptr(), with_noise, pick(cov, o["cov"]))

    for kw, cause in ((dict(P=0), b"P, T >= 1"), (dict(P=-2), b"P, T >= 1"), (dict(T=0), b"P, T >= 1"), (dict(T=-1), b"P, T >= 1"),
                      (dict(x0=False), b"null array"), (dict(u=False), b"null array"), (dict(x=False), b"null array"),
                      (dict(A=False), b"A_dev and B_dev"), (dict(B=False), b"A_dev and B_dev"),
                      (dict(with_gp=2), b"with_gp"), (dict(with_gp=-1), b"with_gp"),
                      (dict(with_noise=2), b"with_noise"), (dict(with_noise=-1), b"with_noise"),
                      (dict(K=Kbad), b"non-finite"), (dict(K=Knan), b"non-finite"),
                      (dict(P=60_000_000, T=5), b"int32"), (dict(P=1, T=2**31 - 1), b"int32"),
                      (dict(P=10_000_000, T=6), b"P T nx nx")):   # (P (T + 1) nx = 4.2e8 fits, P T nx nx = 2.16e9 does not)
        assert call(c.s._h, **kw) == -1 and cause in lib.gpmpc_last_error(), kw
    assert call(None) == -1
    h = ctypes.c_void_p()   # before gpmpc_set_model
    assert lib.gpmpc_create(spec.model_id, 5, 2, torch.cuda.current_device(), ctypes.byref(h)) == 0
    try:
        for with_gp in (0, 1):
            assert call(h, with_gp=with_gp, var=False, cov=False) == -3 and b"gpmpc_set_model" in lib.gpmpc_last_error()
    finally:
        lib.gpmpc_destroy(h)
    # the GPs off: none set, or switched off; the variance or the covariance without a GP, or without its Linv
    fresh = BatchSolver(spec, 5, 2)
    assert call(fresh._h, var=False, cov=False) == -3 and b"GPs are off" in lib.gpmpc_last_error()
    for kw in (dict(), dict(var=False), dict(cov=False)):
        assert call(fresh._h, with_gp=0, **kw) == -3 and b"not set" in lib.gpmpc_last_error(), kw
    fresh.set_gps(c.gpp, with_variance=False)
    for with_gp, kw in itertools.product((0, 1), (dict(), dict(var=False), dict(cov=False))):
        assert call(fresh._h, with_gp=with_gp, **kw) == -3 and b"Linv" in lib.gpmpc_last_error(), (with_gp, kw)
    fresh.set_gps(c.gpp)
    fresh.set_gps(None)
    assert call(fresh._h, var=False, cov=False) == -3 and b"GPs are off" in lib.gpmpc_last_error()
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in o.values())
    # and the calls go through where nothing is in their way
    assert call(fresh._h, with_gp=0) == 0   # (the GPs are switched off, not gone: the variance reads them)
    want = c.run(False)
    assert all(same(o[k].cpu().numpy(), want[k]) for k in KEYS)
    fresh.set_gps(c.gpp, with_variance=False)
    for t in o.values():
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    assert call(fresh._h, var=False, cov=False) == 0
    want = c.run(True)
    assert all(same(o[k].cpu().numpy(), want[k]) for k in ("x", "A", "B"))
    assert torch.isnan(o["var"]).all() and torch.isnan(o["cov"]).all()


# ------------------------------------------------------------------------------------------------ 8
@functools.lru_cache(maxsize=None)
def _controller():
    from gpmpc.gpmpc import GPMPC

    U.gpu_torch()
    spec, data, _ = problem("quad2d", 40)
    ctrl = GPMPC("quad2d", horizon=5, batch=8, variance="exact")
    ctrl.train_gp(np.hstack([X for X, _ in data]), np.column_stack([y for _, y in data]), lr=0.05, iterations=20)
    ctrl.reset()
    return spec, ctrl


def test_controller_predicts_covariances_and_reports_calibration():
    from gpmpc.learning import prediction_calibration, run_evaluation

    spec, ctrl = _controller()
    B, S, h = 8, 12, 4
    x0, phase = initial_states(spec, ctrl.traj, B)
    u = spec.u_eq + 0.1 * np.random.default_rng(4).standard_normal((B, 6, spec.nu))
    Kl = np.ascontiguousarray(ctrl.lqr_gain)
    for with_gp, (feedback, K), with_noise in itertools.product((True, False), ((None, None), ("lqr", Kl), (2.0 * Kl, 2.0 * Kl)),
                                                                (False, True)):
        want = lin(ctrl.solver, x0, u, with_gp, True, True, K, None, with_noise)
        got = ctrl.predict_trajectory(x0, u, with_gp=with_gp, return_var=True, return_cov=True, feedback=feedback,
                                      with_noise=with_noise)
        assert len(got) == 3 and same(got[0], want["x"]) and same(got[1], want["var"]) and same(got[2], want["cov"])
        x3, c3 = ctrl.predict_trajectory(x0[3], u[3], with_gp=with_gp, return_cov=True, feedback=feedback, with_noise=with_noise)
        assert same(x3, want["x"][3]) and same(c3, want["cov"][3])
    # the defaults return what the call returned before
    assert same(ctrl.predict_trajectory(x0, u), plain(ctrl.solver, x0, u))
    xv = ctrl.predict_trajectory(x0, u, return_var=True)
    assert len(xv) == 2 and all(same(a, b) for a, b in zip(xv, plain(ctrl.solver, x0, u, True, True)))
    data = run_evaluation(ctrl, x0, S, phase)
    for feedback, K in ((None, None), ("lqr", Kl)):
        z = prediction_calibration(ctrl, data, h, feedback=feedback)
        assert z.shape == (h, spec.nx)
        num = np.zeros((h, spec.nx))
        bad = np.zeros((h, spec.nx), dtype=bool)
        for s in range(S - h + 1):
            out = lin(ctrl.solver, data["obs"][s], data["action"][s:s + h].transpose(1, 0, 2), True, False, True, K, None, True)
            var = np.diagonal(out["cov"][:, 1:], axis1=-2, axis2=-1)
            err = out["x"][:, 1:] - data["obs"][s + 1:s + h + 1].transpose(1, 0, 2)
            bad |= (var <= 0).any(axis=0)
            num += (err ** 2 / np.where(var > 0, var, 1.0)).sum(axis=0)
        want = np.where(bad, np.nan, np.sqrt(num / ((S - h + 1) * B)))
        print(f"[rollout_lin] calibration, feedback {feedback}:\n{z}")
        assert np.array_equal(np.isnan(z), bad) and np.isfinite(z[:, spec.to_dict()["unc_dims"]]).all()
        np.testing.assert_allclose(z[~bad], want[~bad], rtol=1e-12, atol=0)


def test_learn_records_the_calibration_beside_the_error_curves():
    from gpmpc.learning import learn

    spec, ctrl = _controller()
    kw = dict(n_epochs=1, ctrl=ctrl, lr=0.05, gp_iterations=5, seed=5, samples_per_epoch=30, episode_len=6)
    _, test, _ = learn(report_prediction=2, **kw)
    assert "calibration" not in test[0] and set(test[1]["prediction_error"]) == {"gp", "prior"}
    z = test[1]["calibration"]
    assert z.shape == (2, spec.nx) and np.isfinite(z[:, spec.to_dict()["unc_dims"]]).all() and (z[np.isfinite(z)] > 0).all()
    _, test, _ = learn(**kw)
    assert "calibration" not in test[1] and "prediction_error" not in test[1]
