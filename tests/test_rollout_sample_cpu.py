"""gpmpc_rollout_sample without a GPU: the CPU reference of rollout_sample_ref.py against rollout_ref.py and against
the first-order effect of a draw, learning.tightening_coverage and GPMPC.sample_trajectories on stubs, and the
declaration in the header and the ctypes binding."""

import re

import numpy as np
import pytest
import torch

import rollout_ref as RR
import rollout_sample_ref as SR
from helpers import O, initial_states, lqr, oracle_gps, problem

NX, NU, NGP = 3, 2, 2
M = np.array([[0.5, -1.0, 0.25], [2.0, 0.125, -0.75]])   # the fake's input map (nu, nx)
D = np.array([[1.0, 0.0, -2.0], [0.0, 0.5, 0.25]])       # and its disturbance map (n_gp, nx)


def _inputs(name, N, P, T, seed=5):
    spec, data, hyp = problem(name, N)
    gps = oracle_gps(data, hyp)
    x0, _ = initial_states(spec, spec.reference_trajectory(), P)
    rng = np.random.default_rng(seed)
    u = spec.u_eq + 0.1 * rng.standard_normal((P, T, spec.nu))
    xi = rng.standard_normal((P, T, spec.n_gp))
    return spec, gps, x0, u, xi


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", ("quad2d", "cartpole"))
def test_reference_without_draws_or_feedback_is_the_plain_rollout(name):
    spec, gps, x0, u, xi = _inputs(name, 17, 2, 4)
    for g in (gps, None):
        want = RR.rollout(spec, g, x0, u)
        out = SR.rollout(spec, g, x0, u, xi=np.zeros_like(xi), exact_gps=gps, var=True)
        assert np.array_equal(out["x"], want) and np.array_equal(out["u"], u)
        assert np.array_equal(out["var"], RR.variances(spec, gps, want, u))
        assert np.array_equal(SR.rollout(spec, g, x0, u)["x"], want)
        # a gain around the trajectory's own mean adds exact zeros
        K = lqr(spec)[2]
        fb = SR.rollout(spec, g, x0, u, xref=want, K=K)
        assert np.array_equal(fb["x"], want) and np.array_equal(fb["u"], u)
    # the draws matter, and so does the feedback around another reference
    assert not np.array_equal(SR.rollout(spec, gps, x0, u, xi=xi, exact_gps=gps)["x"], want)
    moved = SR.rollout(spec, gps, x0, u, xref=want + 0.01, K=K)
    assert not np.array_equal(moved["u"], u) and not np.array_equal(moved["x"], want)


def test_reference_feedback_is_the_fma_chain_and_the_clip_keeps_a_nan():
    spec, gps, x0, u, _ = _inputs("quad2d", 17, 3, 1)
    K = lqr(spec)[2]
    xref = x0 + 0.05 * np.random.default_rng(1).standard_normal(x0.shape)
    got = SR.applied_input(spec, x0, u[:, 0], xref, K)
    want = u[:, 0] + (x0 - xref) @ K.T
    assert np.abs(got - want).max() <= 1e-15 * (1 + np.abs(want).max()) * spec.nx
    assert SR.fma(3.0, 1.0 / 3.0, -1.0) == -2.0 ** -54 and 3.0 * (1.0 / 3.0) - 1.0 == 0.0   # one rounding, not two
    lo, hi = spec.u_lo, spec.u_hi
    wide = np.array([[hi[0] + 1.0, lo[1] - 1.0], [np.nan, 0.0], [0.5 * (lo[0] + hi[0]), np.nan]])
    c = SR.applied_input(spec, x0, wide, clip=True)
    assert c[0, 0] == hi[0] and c[0, 1] == lo[1] and np.isnan(c[1, 0]) and c[1, 1] == 0.0 and np.isnan(c[2, 1])
    assert c[2, 0] == wide[2, 0]
    assert np.array_equal(SR.applied_input(spec, x0, wide), wide, equal_nan=True)


def _first_order(spec, gps, x, u, e):
    """d x+ / d eps at eps = 0 of the RK4 step with gm_g = mean_g + eps e_g at every substage: the tangent of the
    step in the offset, dk_s = df/dgm|_s e + df/dx|_s c_s dt dk_{s-1}, with df/dgm from a central difference of the
    oracle's f in gm (f is affine in gm, so the difference is exact to rounding) and df/dx the oracle's Jacobian."""
    sd = spec.to_dict()
    dyn = O.Dynamics(sd, gps)
    nx, dt, h = spec.nx, spec.dt, 1e-3

    def dfdgm(xs):
        z = np.concatenate([xs, u])
        mg = [gps[i].mean_grad(z[idx]) for i, idx in enumerate(sd["gp_inputs"])]
        gm, gg = [m for m, _ in mg], [d for _, d in mg]
        G = np.empty((nx, spec.n_gp))
        for g in range(spec.n_gp):
            up, dn = list(gm), list(gm)
            up[g] += h
            dn[g] -= h
            G[:, g] = (dyn._f(dyn.p, dyn.g, xs, u, up, gg)[0] - dyn._f(dyn.p, dyn.g, xs, u, dn, gg)[0]) / (2 * h)
        return G

    cs, ws = (0.0, 0.5, 0.5, 1.0), (1.0, 2.0, 2.0, 1.0)
    k, dk, total = np.zeros(nx), np.zeros(nx), np.zeros(nx)
    for c, w in zip(cs, ws):
        xs = x + c * dt * k
        k, J = dyn.f_jac(xs, u)
        dk = dfdgm(xs) @ e + J[:, :nx] @ (c * dt * dk)
        total += w * dk
    return dt / 6.0 * total, dt * (dfdgm(x) @ e)


@pytest.mark.parametrize("name", ("quad2d", "quad3d", "cartpole"))
def test_a_small_draw_moves_the_state_by_dt_dfdgm_sqrt_var_xi(name):
    """(x(eps) - x(0)) / eps at row 1, eps = 1e-6, against the first-order term of the step in the draw: dt/6 times the
    RK4-weighted df/dgm sqrt(var) xi of the four substages (_first_order), within 1e-5 of its largest entry: the
    O(eps) remainder is the only error.  df/dgm at (x_0, u_0) alone, dt df/dgm sqrt(var) xi, leaves out how the offset
    of one substage moves the state of the next (a velocity's draw reaches its position within the step), which is no
    error of the reference; its distance is printed (measured: quad2d 1.0e-1, quad3d 1.0e-1, cartpole 2.5e-2 of the
    largest entry, against 5.2e-7 at most for the substage form)."""
    spec, gps, x0, u, xi = _inputs(name, 20, 2, 1)
    eps = 1e-6
    base = SR.rollout(spec, gps, x0, u, xi=np.zeros_like(xi), exact_gps=gps, var=True)
    moved = SR.rollout(spec, gps, x0, u, xi=eps * xi, exact_gps=gps)
    fd = (moved["x"][:, 1] - base["x"][:, 1]) / eps
    for p in range(2):
        e = np.sqrt(base["var"][p, 0]) * xi[p, 0]
        want, naive = _first_order(spec, gps, x0[p], u[p, 0], e)
        top = np.abs(want).max()
        err, err_naive = np.abs(fd[p] - want).max() / top, np.abs(fd[p] - naive).max() / top
        print(f"[rollout_sample] {name} trajectory {p}: largest entry {top:.3e}, error {err:.3e} of it; "
              f"against dt df/dgm at (x_0, u_0) alone {err_naive:.3e}")
        assert top > 0 and err <= 1e-5


def test_noise_enters_under_the_root_once():
    spec, gps, x0, u, xi = _inputs("quad2d", 17, 2, 1)
    v = SR.point_variances(spec, gps, x0, u[:, 0])
    sn2 = np.array([gp.sn2 for gp in gps])
    assert np.array_equal(SR.draws(gps, v, xi[:, 0], True), np.sqrt(v + sn2) * xi[:, 0])
    assert np.array_equal(SR.draws(gps, v, xi[:, 0]), np.sqrt(v) * xi[:, 0])
    assert np.array_equal(SR.draws(gps, -v, xi[:, 0]), np.zeros_like(v) * xi[:, 0])   # the tightening's clamp
    # with_gp = 0: the value passed to f is the draw alone
    a = SR.rollout(spec, None, x0, u, xi=xi, exact_gps=gps)["x"]
    assert not np.array_equal(a, RR.rollout(spec, None, x0, u))


# ------------------------------------------------------------------------------------------------ Python, on stubs
class StubCtrl:
    """predict_trajectory and sample_trajectories return fixed arrays and record what they were asked."""

    inverse_cdf = 1.5

    def __init__(self, xbar, cov, x):
        self.xbar, self.cov, self.x = xbar, cov, x
        self.calls = []

    def predict_trajectory(self, x0, u, **kw):
        self.calls.append(("predict", kw))
        return self.xbar, self.cov

    def sample_trajectories(self, x0, u, n_samples, **kw):
        self.calls.append(("sample", dict(kw, n_samples=n_samples)))
        return self.x, None


@pytest.mark.parametrize("batch", (False, True))
def test_tightening_coverage_is_its_formula(batch):
    from gpmpc.learning import tightening_coverage

    rng = np.random.default_rng(12)
    P, S, T = 3, 7, 4
    xbar = rng.standard_normal((P, T + 1, NX))
    A = rng.standard_normal((P, T + 1, NX, NX))
    cov = A @ A.transpose(0, 1, 3, 2)
    cov[:, 0] = 0.0
    cov[1, 2, 1, :] = cov[1, 2, :, 1] = 0.0   # one trajectory's zero variance makes (stage 2, state 1) NaN
    x = xbar[:, None] + 1.2 * np.sqrt(np.diagonal(cov, axis1=-2, axis2=-1))[:, None] * rng.standard_normal((P, S, T + 1, NX))
    if not batch:
        xbar, cov, x, P = xbar[0], cov[0], x[0], 1
    ctrl = StubCtrl(xbar, cov, x)
    got = tightening_coverage(ctrl, "x0", "u", S, seed=9, feedback="lqr", with_noise=False)
    assert ctrl.calls == [("predict", dict(return_cov=True, feedback="lqr", with_noise=False)),
                          ("sample", dict(n_samples=S, seed=9, feedback="lqr", with_noise=False))]
    xb, cv, xs = (xbar, cov, x) if batch else (xbar[None], cov[None], x[None])
    want = np.full((T + 1, NX), np.nan)
    for k in range(1, T + 1):
        for i in range(NX):
            if batch and (k, i) == (2, 1):
                continue
            n = sum(abs(xs[p, s, k, i] - xb[p, k, i]) <= 1.5 * np.sqrt(cv[p, k, i, i]) for p in range(P) for s in range(S))
            want[k, i] = n / (P * S)
    assert got.shape == (T + 1, NX) and np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[0]).all() and ((got[1:] >= 0) | np.isnan(got[1:])).all() and np.nanmax(got) <= 1.0
    assert ((got > 0.0) & (got < 1.0)).any(), "the case separates inside from outside"
    # the defaults: the LQR gain and the likelihood noise
    tightening_coverage(ctrl, "x0", "u", 2)
    assert ctrl.calls[-1] == ("sample", dict(n_samples=2, seed=0, feedback="lqr", with_noise=True))


class FakeSolver:
    """x_{k+1} = x_k + u_k M + xi_k D on CPU tensors, u_k = u_nom,k + (x_k - xref_k) K^T, clipped to [-1, 1]."""

    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def rollout(self, x0, u, with_gp=True, var=False):
        return self.rollout_sample(x0, u)["x"]

    def rollout_sample(self, x0, u, xref=None, K=None, clip=False, xi=None, with_gp=True, with_noise=False, var=False):
        assert all(isinstance(t, torch.Tensor) and t.dtype == torch.float64 for t in (x0, u))
        self.calls.append(dict(xref=xref, K=K, clip=clip, xi=xi, with_gp=with_gp, with_noise=with_noise, var=var))
        P, T = u.shape[:2]
        x = torch.empty(P, T + 1, NX, dtype=torch.float64)
        ua = torch.empty(P, T, NU, dtype=torch.float64)
        x[:, 0] = x0
        for k in range(T):
            ua[:, k] = u[:, k] if K is None else u[:, k] + (x[:, k] - xref[:, k]) @ torch.tensor(K).T
            if clip:
                ua[:, k] = ua[:, k].clamp(-1.0, 1.0)
            x[:, k + 1] = x[:, k] + ua[:, k] @ torch.tensor(M) + (0 if xi is None else xi[:, k] @ torch.tensor(D))
        return {"x": x, "u": ua}


class FakeCtrl:
    def __init__(self):
        self.solver = FakeSolver()
        self.lqr_gain = np.full((NU, NX), -0.25)
        self.model = type("Spec", (), {"n_gp": NGP})()


def test_sample_trajectories_repeats_seeds_and_shapes():
    from gpmpc.gpmpc import GPMPC

    rng = np.random.default_rng(2)
    P, S, T = 3, 4, 5
    x0, u = rng.standard_normal((P, NX)), 0.2 * rng.standard_normal((P, T, NU))
    ctrl = FakeCtrl()
    x, ua = GPMPC.sample_trajectories(ctrl, x0, u, S, seed=7)
    call = ctrl.solver.calls[-1]
    assert x.shape == (P, S, T + 1, NX) and ua.shape == (P, S, T, NU)
    assert call["K"] is None and call["xref"] is None and call["clip"] is True and call["with_noise"] is True
    assert call["with_gp"] is True and tuple(call["xi"].shape) == (P * S, T, NGP)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(7)
    assert torch.equal(call["xi"], torch.randn(P * S, T, NGP, dtype=torch.float64, generator=gen))
    # every input trajectory is repeated n_samples times: the samples of trajectory p start at x0[p] under u[p]
    assert np.array_equal(x[:, :, 0], np.repeat(x0[:, None], S, axis=1)) and np.array_equal(ua, np.repeat(u[:, None], S, axis=1))
    assert not np.array_equal(x[:, 0], x[:, 1])
    again, _ = GPMPC.sample_trajectories(ctrl, x0, u, S, seed=7)
    other, _ = GPMPC.sample_trajectories(ctrl, x0, u, S, seed=8)
    assert np.array_equal(again, x) and not np.array_equal(other, x)
    # one trajectory; the LQR gain around the mean prediction; an array as the gain
    x1, u1 = GPMPC.sample_trajectories(ctrl, x0[1], u[1], 2, seed=7, feedback="lqr", clip=False, with_noise=False, with_gp=False)
    call = ctrl.solver.calls[-1]
    assert x1.shape == (2, T + 1, NX) and u1.shape == (2, T, NU) and call["K"] is ctrl.lqr_gain
    assert call["clip"] is False and call["with_noise"] is False and call["with_gp"] is False
    mean = ctrl.solver.rollout(torch.tensor(x0[1:2]), torch.tensor(u[1:2])).numpy()
    assert np.array_equal(call["xref"].numpy(), np.repeat(mean, 2, axis=0))
    assert not np.array_equal(u1[0], u[1])   # the feedback acts on the disturbed state
    Kz = np.zeros((NU, NX))
    GPMPC.sample_trajectories(ctrl, x0, u, 1, feedback=Kz)
    assert ctrl.solver.calls[-1]["K"] is Kz
    for bad in (dict(feedback="pid"), dict(n_samples=0)):
        with pytest.raises(ValueError):
            GPMPC.sample_trajectories(ctrl, x0, u, **dict(dict(n_samples=2), **bad))
    for xb, ub in ((x0[0], u), (x0, u[0]), (x0[:2], u)):
        with pytest.raises(ValueError):
            GPMPC.sample_trajectories(ctrl, xb, ub, 2)


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_and_binding():
    from ctypes import c_int32, c_void_p

    from gpmpc import _lib
    from stream_order_util import HEADER, stream_functions

    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    found = re.findall(r"\bgpmpc_status\s+gpmpc_rollout_sample\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert len(found) == 1, "gpmpc_rollout_sample is declared once in the header"
    params = [" ".join(p.split()) for p in found[0].split(",")]
    assert params == ["gpmpc_handle* h", "int32_t P", "int32_t T", "const double* x0_dev", "const double* u_dev",
                      "const double* xref_dev", "const double* K", "int32_t clip", "const double* xi_dev",
                      "int32_t with_gp", "int32_t with_noise", "double* x_dev", "double* uapp_dev", "double* var_dev"]
    assert "stream" not in found[0] and "gpmpc_rollout_sample" not in stream_functions()
    res, args = _lib.SIGNATURES["gpmpc_rollout_sample"]
    assert res is c_int32
    assert args == [c_int32 if p.startswith("int32_t ") else c_void_p for p in params]
    assert text.index("gpmpc_rollout_lin(") < text.index("gpmpc_rollout_sample(")   # next to gpmpc_rollout_lin
    head = raw.split("#ifndef GPMPC_MI355X_H")[0]
    assert "gpmpc_rollout_sample does too" in head and "xref_dev and xi_dev" in head


def test_null_handle_is_refused_without_a_device():
    from gpmpc import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load(require_gpu=False)
    assert lib.gpmpc_rollout_sample(None, 1, 1, None, None, None, None, 0, None, 0, 0, None, None, None) == -1
    assert b"null handle" in lib.gpmpc_last_error()
