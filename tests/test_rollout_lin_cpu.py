"""gpmpc_rollout_lin without a GPU: the declaration in the header and the ctypes binding, the numpy covariance
recursion of rollout_lin_ref.py pinned against the oracle's tightening, and learning.prediction_calibration /
predict_trajectory(return_cov=True) against a fake solver whose rollout_lin is known in closed form."""

import re

import numpy as np
import pytest
import torch

import rollout_lin_ref as LR
from helpers import O, initial_states, lqr, oracle_gps, problem

NX, NU, NGP = 3, 2, 2
M = np.array([[0.5, -1.0, 0.25], [2.0, 0.125, -0.75]])   # the fake's input map (nu, nx)
C = np.array([0.25, 4.0, 0.0])                           # its variance growth per step and state (state 2: none)


class FakeSolver:
    """x_{k+1} = x_k + u_k M on CPU tensors; cov[p][k] = k diag(C) (+ 1 on the diagonal from step 1 on with a gain)."""

    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def rollout_lin(self, x0, u, with_gp=True, var=False, cov=False, K=None, cov0=None, with_noise=False):
        assert isinstance(x0, torch.Tensor) and isinstance(u, torch.Tensor) and x0.dtype == u.dtype == torch.float64
        self.calls.append(dict(x0=x0.numpy().copy(), u=u.numpy().copy(), with_gp=with_gp, var=var, cov=cov, K=K,
                               cov0=cov0, with_noise=with_noise))
        P, T = u.shape[:2]
        x = torch.empty(P, T + 1, NX, dtype=torch.float64)
        x[:, 0] = x0
        for k in range(T):
            x[:, k + 1] = x[:, k] + u[:, k] @ torch.tensor(M)
        out = {"x": x, "A": torch.eye(NX, dtype=torch.float64).expand(P, T, NX, NX).clone(),
               "B": torch.tensor(M.T).expand(P, T, NX, NU).clone()}
        if var:
            out["var"] = torch.ones(P, T, NGP, dtype=torch.float64)
        if cov:
            d = torch.arange(T + 1, dtype=torch.float64)[:, None] * torch.tensor(C)[None, :]
            if K is not None:
                d[1:] += 1.0
            out["cov"] = torch.diag_embed(d).expand(P, T + 1, NX, NX).clone()
        return out


class FakeCtrl:
    def __init__(self):
        self.solver = FakeSolver()
        self.lqr_gain = np.full((NU, NX), 0.5)


def _run(S, B, d):
    rng = np.random.default_rng(3)
    act = rng.standard_normal((S, B, NU))
    obs = np.empty((S + 1, B, NX))
    obs[0] = rng.standard_normal((B, NX))
    for s in range(S):
        obs[s + 1] = obs[s] + act[s] @ M + d[s]
    return dict(obs=obs, action=act)


# ------------------------------------------------------------------------------------------------ header and binding
def _header():
    from stream_order_util import HEADER

    return HEADER


def test_header_and_binding():
    from ctypes import c_int32, c_void_p

    from gpmpc import _lib
    from stream_order_util import stream_functions

    text = re.sub(r"/\*.*?\*/", " ", _header().read_text(), flags=re.S)
    found = re.findall(r"\bgpmpc_status\s+gpmpc_rollout_lin\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert len(found) == 1, "gpmpc_rollout_lin is declared once in the header"
    params = [" ".join(p.split()) for p in found[0].split(",")]
    assert params == ["gpmpc_handle* h", "int32_t P", "int32_t T", "const double* x0_dev", "const double* u_dev",
                      "int32_t with_gp", "double* x_dev", "double* A_dev", "double* B_dev", "double* var_dev",
                      "const double* K", "const double* cov0_dev", "int32_t with_noise", "double* cov_dev"]
    assert "stream" not in found[0] and "gpmpc_rollout_lin" not in stream_functions()
    res, args = _lib.SIGNATURES["gpmpc_rollout_lin"]
    assert res is c_int32
    assert args == [c_int32 if p.startswith("int32_t ") else c_void_p for p in params]
    raw = _header().read_text()
    head = raw.split("#ifndef GPMPC_MI355X_H")[0]
    assert "gpmpc_rollout_lin follows the same rule" in head
    assert "THE NOISE ENTERS ONCE" in raw


def test_null_handle_is_refused_without_a_device():
    from gpmpc import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load(require_gpu=False)
    assert lib.gpmpc_rollout_lin(None, 1, 1, None, None, 0, None, None, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.gpmpc_last_error()


def test_the_new_source_is_built_and_hashed():
    from gpmpc import _lib
    from stream_order_util import HEADER

    mk = (HEADER.parents[1] / "gp-mpc_amd" / "csrc" / "Makefile").read_text()
    srcs = [f for line in re.findall(r"^SRCS \+?= (.*)$", mk, re.M) for f in line.split()]
    hashed = re.search(r"^HASHED = (.*)$", mk, re.M).group(1).split()
    assert srcs.count("rollout_cov.hip") == 1 and hashed.count("rollout_cov.hip") == 1 and hashed == _lib.HASHED


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", ("quad2d", "quad3d", "cartpole"))
def test_recursion_is_the_oracles_tightening_on_constant_matrices(name):
    """Fed constant A_k = Ad, B_k = Bd_u, the LQR K and q_k = the oracle's cov_d + cov_n, the recursion's diagonals are
    those O.propagate_constraint_limits takes the square root of.  The oracle expands (Ad + Bd_u K) S (Ad + Bd_u K)^T
    into its four terms, so the two forms differ in the order of fewer than 2 nx + 4 additions per entry: entrywise
    1e-12 relative to the sum of the absolute terms."""
    spec, data, hyp = problem(name, 20)
    sd = spec.to_dict()
    gps = oracle_gps(data, hyp)
    Ad, Bdu, K = lqr(spec)
    T, prob = 6, 0.95
    rng = np.random.default_rng(8)
    x0, _ = initial_states(spec, spec.reference_trajectory(), 1)
    x = x0[0][None, :] + 0.05 * rng.standard_normal((T + 1, spec.nx))
    u = spec.u_eq + 0.1 * rng.standard_normal((T, spec.nu))
    sc, _ = O.propagate_constraint_limits(sd, gps, x.T, u.T, Ad, Bdu, K, prob)
    icdf = O.inverse_cdf(prob, spec.nx)
    want = (sc[spec.nx:] / -icdf).T ** 2                                    # (T+1, nx): diag of cov_x
    z = np.hstack([x[:-1], u])
    var = np.stack([gp.var(z[:, idx], with_noise=True) for gp, idx in zip(gps, sd["var_inputs"])], axis=-1)
    q = LR.process_noise(spec, x[:-1], u, var, noise=[gp.sn2 for gp in gps])
    A, B = np.broadcast_to(Ad, (T,) + Ad.shape), np.broadcast_to(Bdu, (T,) + Bdu.shape)
    S = LR.cov_recursion(spec, A, B, K, q)
    assert S.shape == (T + 1, spec.nx, spec.nx) and not S[0].any()
    scale = np.zeros((T + 1, spec.nx))
    for k in range(T):
        nxt, mag = LR.cov_step(spec, S[k], Ad, Bdu, K, q[k])
        assert np.array_equal(nxt, S[k + 1])
        scale[k + 1] = np.diag(mag)
    got = np.diagonal(S, axis1=1, axis2=2)
    err = np.abs(got - want)
    print(f"[rollout_lin] {name}: max |diag - oracle| / scale {np.max(err / np.maximum(scale, 1e-300)):.3e}, largest diag {got.max():.3e}")
    assert (err <= 1e-12 * scale).all()
    assert got[1:].max() > 0 and (got[1, sd["unc_dims"]] > 0).all()
    # open loop and closed loop differ, and a start covariance passes through
    assert not np.allclose(LR.cov_recursion(spec, A, B, None, q)[-1], S[-1], rtol=1e-6, atol=0)
    c0 = np.diag(np.arange(1.0, spec.nx + 1))
    assert np.array_equal(LR.cov_recursion(spec, A, B, K, q, c0)[0], c0)


def test_reference_jacobians_are_the_oracles_and_differentiate_the_step():
    spec, data, hyp = problem("quad2d", 17)
    gps = oracle_gps(data, hyp)
    x0, _ = initial_states(spec, spec.reference_trajectory(), 2)
    u = spec.u_eq + 0.1 * np.random.default_rng(5).standard_normal((2, spec.nu))
    xn, A, B = LR.jacobians(spec, gps, x0, u)
    assert xn.shape == (2, spec.nx) and A.shape == (2, spec.nx, spec.nx) and B.shape == (2, spec.nx, spec.nu)
    h = 1e-6
    for j in range(spec.nx):
        e = np.zeros(spec.nx)
        e[j] = h
        fd = (LR.jacobians(spec, gps, x0 + e, u)[0] - LR.jacobians(spec, gps, x0 - e, u)[0]) / (2 * h)
        assert np.abs(fd - A[:, :, j]).max() <= 1e-7
    for j in range(spec.nu):
        e = np.zeros(spec.nu)
        e[j] = h
        fd = (LR.jacobians(spec, gps, x0, u + e)[0] - LR.jacobians(spec, gps, x0, u - e)[0]) / (2 * h)
        assert np.abs(fd - B[:, :, j]).max() <= 1e-7


# ------------------------------------------------------------------------------------------------ Python, on a stub
@pytest.mark.parametrize("stride,starts", [(1, list(range(7))), (3, [0, 3, 6])])
def test_prediction_calibration_windows_and_arithmetic(stride, starts):
    from gpmpc.learning import prediction_calibration

    S, B, h = 10, 3, 4
    d = 0.1 * np.random.default_rng(11).standard_normal((S, B, NX))
    data = _run(S, B, d)
    ctrl = FakeCtrl()
    z = prediction_calibration(ctrl, data, h, stride=stride)
    call = ctrl.solver.calls[-1]
    assert z.shape == (h, NX) and call["cov"] is True and call["with_noise"] is True and call["K"] is None
    assert call["with_gp"] is True and call["cov0"] is None and len(ctrl.solver.calls) == 1
    assert np.array_equal(call["x0"], data["obs"][starts].reshape(-1, NX))
    want_u = np.stack([data["action"][s:s + h].transpose(1, 0, 2) for s in starts]).reshape(-1, h, NU)
    assert np.array_equal(call["u"], want_u)
    # x_pred[k] - obs[s + k] = -(d[s] + .. + d[s + k - 1]), and the variance of state i at step k is k C[i]
    acc = np.stack([np.cumsum(d[s:s + h], axis=0) for s in starts])          # (W, h, B, nx)
    k = np.arange(1, h + 1)[:, None]
    want = np.sqrt((acc[..., :2] ** 2).mean(axis=(0, 2)) / (k * C[None, :2]))
    np.testing.assert_allclose(z[:, :2], want, rtol=1e-13, atol=0)
    assert np.isnan(z[:, 2]).all()   # a variance of 0 gives NaN for that state, not a division error
    # feedback: "lqr" passes the controller's gain, an array is taken as K
    z1 = prediction_calibration(ctrl, data, h, stride=stride, feedback="lqr")
    assert ctrl.solver.calls[-1]["K"] is ctrl.lqr_gain
    want1 = np.sqrt((acc ** 2).mean(axis=(0, 2)) / (k * C[None, :] + 1.0))
    np.testing.assert_allclose(z1, want1, rtol=1e-13, atol=0)
    K = np.zeros((NU, NX))
    prediction_calibration(ctrl, data, h, stride=stride, feedback=K)
    assert ctrl.solver.calls[-1]["K"] is K
    for bad in (dict(horizon=S + 1), dict(horizon=0), dict(horizon=2, stride=0), dict(horizon=2, feedback="pid")):
        with pytest.raises(ValueError):
            prediction_calibration(ctrl, data, **bad)


def test_predict_trajectory_return_cov_shapes():
    from gpmpc.gpmpc import GPMPC

    rng = np.random.default_rng(2)
    x0, u = rng.standard_normal((4, NX)), rng.standard_normal((4, 5, NU))
    ctrl = FakeCtrl()
    want = ctrl.solver.rollout_lin(torch.tensor(x0), torch.tensor(u), cov=True)
    x, c = GPMPC.predict_trajectory(ctrl, x0, u, return_cov=True)
    call = ctrl.solver.calls[-1]
    assert np.array_equal(x, want["x"].numpy()) and np.array_equal(c, want["cov"].numpy()) and c.shape == (4, 6, NX, NX)
    assert call["K"] is None and call["with_noise"] is False and call["var"] is False and call["with_gp"] is True
    x1, v1, c1 = GPMPC.predict_trajectory(ctrl, x0[2], u[2], with_gp=False, return_var=True, return_cov=True,
                                          feedback="lqr", with_noise=True)
    call = ctrl.solver.calls[-1]
    assert x1.shape == (6, NX) and v1.shape == (5, NGP) and c1.shape == (6, NX, NX)
    assert call["K"] is ctrl.lqr_gain and call["with_noise"] is True and call["with_gp"] is False
    assert c1[1, 0, 0] == C[0] + 1.0
    K = np.ones((NU, NX))
    GPMPC.predict_trajectory(ctrl, x0, u, return_cov=True, feedback=K)
    assert ctrl.solver.calls[-1]["K"] is K
    with pytest.raises(ValueError):
        GPMPC.predict_trajectory(ctrl, x0, u, return_cov=True, feedback="pid")
