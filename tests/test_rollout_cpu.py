"""gpmpc_rollout without a GPU: the CPU reference's composition property, learning.prediction_error and
predict_trajectory against a fake controller whose solver.rollout is a known linear map on CPU tensors, and the
declaration in the header and the ctypes binding."""

import re

import numpy as np
import pytest
import torch

import rollout_ref as RR
from helpers import initial_states, oracle_gps, problem

NX, NU, NGP = 3, 2, 2
M = np.array([[0.5, -1.0, 0.25], [2.0, 0.125, -0.75]])   # the fake's input map (nu, nx)


class FakeSolver:
    """x_{k+1} = x_k + u_k M on CPU tensors; var[p][k][g] = g + 1 + k.  Records what it was asked."""

    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def rollout(self, x0, u, with_gp=True, var=False):
        assert isinstance(x0, torch.Tensor) and isinstance(u, torch.Tensor) and x0.dtype == u.dtype == torch.float64
        assert x0.ndim == 2 and u.ndim == 3 and x0.shape[0] == u.shape[0]
        self.calls.append(dict(x0=x0.numpy().copy(), u=u.numpy().copy(), with_gp=with_gp, var=var))
        P, T = u.shape[:2]
        x = torch.empty(P, T + 1, x0.shape[1], dtype=torch.float64)
        x[:, 0] = x0
        Mt = torch.tensor(M)
        for k in range(T):
            x[:, k + 1] = x[:, k] + u[:, k] @ Mt
        if not var:
            return x
        v = torch.arange(1, NGP + 1, dtype=torch.float64)[None, None, :] + torch.arange(T, dtype=torch.float64)[None, :, None]
        return x, v.expand(P, T, NGP).clone()


class FakeCtrl:
    def __init__(self):
        self.solver = FakeSolver()


def _run(S, B, d):
    """A recorded run whose plant is the fake's map plus the per-step disturbance d (S, B, nx)."""
    rng = np.random.default_rng(3)
    act = rng.standard_normal((S, B, NU))
    obs = np.empty((S + 1, B, NX))
    obs[0] = rng.standard_normal((B, NX))
    for s in range(S):
        obs[s + 1] = obs[s] + act[s] @ M + d[s]
    return dict(obs=obs, action=act)


def test_reference_composes_exactly():
    """T = a + b steps equal a steps followed by b steps from their last row, bit for bit."""
    spec, data, hyp = problem("quad2d", 17)
    gps = oracle_gps(data, hyp)
    x0, _ = initial_states(spec, spec.reference_trajectory(), 2)
    u = spec.u_eq + 0.1 * np.random.default_rng(5).standard_normal((2, 5, spec.nu))
    for g in (gps, None):
        full = RR.rollout(spec, g, x0, u)
        head = RR.rollout(spec, g, x0, u[:, :2])
        tail = RR.rollout(spec, g, head[:, -1], u[:, 2:])
        assert full.shape == (2, 6, spec.nx) and np.array_equal(full[:, 0], x0)
        assert np.array_equal(full[:, :3], head) and np.array_equal(full[:, 2:], tail)
    assert not np.array_equal(RR.rollout(spec, gps, x0, u), RR.rollout(spec, None, x0, u))
    v = RR.variances(spec, gps, full, u)
    assert v.shape == (2, 5, spec.n_gp) and (v > 0).all()


@pytest.mark.parametrize("stride,starts", [(1, list(range(7))), (3, [0, 3, 6])])
def test_prediction_error_windows_and_rms(stride, starts):
    from gpmpc.learning import prediction_error

    S, B, h = 10, 3, 4
    rng = np.random.default_rng(11)
    d = 0.1 * rng.standard_normal((S, B, NX))
    data = _run(S, B, d)
    ctrl = FakeCtrl()
    for with_gp in (True, False):
        e = prediction_error(ctrl, data, h, stride=stride, with_gp=with_gp)
        call = ctrl.solver.calls[-1]
        assert e.shape == (h, NX) and call["with_gp"] is with_gp and call["var"] is False
        # one call, window-major then instance; the last admissible window (s = S - h = 6) is among them
        assert starts[-1] == S - h
        assert np.array_equal(call["x0"], data["obs"][starts].reshape(-1, NX))
        want_u = np.stack([data["action"][s:s + h].transpose(1, 0, 2) for s in starts]).reshape(-1, h, NU)
        assert np.array_equal(call["u"], want_u)
        # x_pred[k] - obs[s + k] = -(d[s] + .. + d[s + k - 1])
        acc = np.stack([np.cumsum(d[s:s + h], axis=0) for s in starts])          # (W, h, B, nx)
        want = np.sqrt((acc ** 2).mean(axis=(0, 2)))
        np.testing.assert_allclose(e, want, rtol=0, atol=1e-13)
    assert len(ctrl.solver.calls) == 2


def test_prediction_error_closed_form_and_refusals():
    from gpmpc.learning import prediction_error

    S, B = 6, 2
    c = np.array([0.5, -0.25, 0.0])
    data = _run(S, B, np.broadcast_to(c, (S, B, NX)))
    ctrl = FakeCtrl()
    e = prediction_error(ctrl, data, 3)
    np.testing.assert_allclose(e, np.arange(1, 4)[:, None] * np.abs(c)[None, :], rtol=0, atol=1e-13)
    e = prediction_error(ctrl, data, S)   # one window: horizon = S is admissible
    assert e.shape == (S, NX) and ctrl.solver.calls[-1]["x0"].shape == (B, NX)
    with pytest.raises(ValueError):
        prediction_error(ctrl, data, S + 1)
    with pytest.raises(ValueError):
        prediction_error(ctrl, data, 0)
    with pytest.raises(ValueError):
        prediction_error(ctrl, data, 2, stride=0)


def test_predict_trajectory_shapes():
    from gpmpc.gpmpc import GPMPC
    from gpmpc.mpc import MPC

    rng = np.random.default_rng(2)
    x0, u = rng.standard_normal((4, NX)), rng.standard_normal((4, 5, NU))
    ctrl = FakeCtrl()
    want = ctrl.solver.rollout(torch.tensor(x0), torch.tensor(u)).numpy()
    xb = GPMPC.predict_trajectory(ctrl, x0, u)
    assert isinstance(xb, np.ndarray) and xb.shape == (4, 6, NX) and np.array_equal(xb, want)
    assert ctrl.solver.calls[-1]["with_gp"] is True
    x1 = GPMPC.predict_trajectory(ctrl, x0[2], u[2], with_gp=False)
    assert x1.shape == (6, NX) and np.array_equal(x1, want[2]) and ctrl.solver.calls[-1]["with_gp"] is False
    xs, vs = GPMPC.predict_trajectory(ctrl, x0[1].tolist(), u[1].tolist(), return_var=True)
    assert xs.shape == (6, NX) and vs.shape == (5, NGP) and np.array_equal(xs, want[1]) and vs[2, 1] == 4.0
    xv, vv = GPMPC.predict_trajectory(ctrl, x0, u, return_var=True)
    assert xv.shape == (4, 6, NX) and vv.shape == (4, 5, NGP)
    xm = MPC.predict_trajectory(ctrl, x0, u)
    assert np.array_equal(xm, want) and ctrl.solver.calls[-1]["with_gp"] is False
    xm1, vm1 = MPC.predict_trajectory(ctrl, x0[0], u[0], return_var=True)
    assert xm1.shape == (6, NX) and vm1.shape == (5, NGP)
    for bad in ((x0[0], u), (x0, u[0]), (x0[:3], u), (x0[None], u)):
        with pytest.raises(ValueError):
            GPMPC.predict_trajectory(ctrl, *bad)


def test_header_and_binding():
    from ctypes import c_int32, c_void_p

    from gpmpc import _lib
    from stream_order_util import HEADER, stream_functions

    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    found = re.findall(r"\bgpmpc_status\s+gpmpc_rollout\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert len(found) == 1, "gpmpc_rollout is declared once in the header"
    params = [" ".join(p.split()) for p in found[0].split(",")]
    assert params == ["gpmpc_handle* h", "int32_t P", "int32_t T", "const double* x0_dev", "const double* u_dev",
                      "int32_t with_gp", "double* x_dev", "double* var_dev"]
    assert "stream" not in found[0] and "gpmpc_rollout" not in stream_functions()
    res, args = _lib.SIGNATURES["gpmpc_rollout"]
    assert res is c_int32
    assert args == [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]
    # the "Streams" paragraph says whose the buffers are to order
    head = HEADER.read_text().split("#ifndef GPMPC_MI355X_H")[0]
    assert "gpmpc_rollout takes no stream" in head and "x0_dev and u_dev must be complete when the call is made" in head
