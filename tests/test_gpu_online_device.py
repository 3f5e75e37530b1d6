"""The online learning loop with its data kept on the device (gpmpc.learning.run_online_episode with
device_data=True), MI355X only: the scenario of tests/test_gpu_online_sliding.py -- a quad2d GP-MPC batch of 16,
H = 10, 12 steps, room for 56 training rows, 40 uploaded, 8 of every step's 16 transitions appended, the oldest
rows making room from the third step on -- with the transitions preprocessed and appended by GPMPC.observe.  The
same things are asserted as there (statuses 0 or 2, the n_train sequence, the Python GPs in step with the handle
under gp_drop_ref.MARGIN_DROP against a fresh upload), and against the host path (device_data=False) for the same
seed: the same picks, and obs / action within 1e-6 (1 + |.|), since the two paths differ only by rounding in the
targets.  One more episode picks by variance (select="variance")."""

import numpy as np
import pytest

import gp_drop_ref as D
import gp_ref as R
from gp_append_ref import reference, worst_ratio

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

B, H, STEPS, CAP, SEED = 16, 10, 12, 56, 11


def _controller():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.synthetic import DEFAULT_HYPERS, initial_states, make_training_data

    ctrl = GPMPC("quad2d", horizon=H, batch=B, gp_capacity=CAP)
    gps = []
    for i, (X, y) in enumerate(make_training_data(ctrl.model, 40, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS["quad2d"][i])
        gps.append(gp)
    ctrl.set_gaussian_processes(gps)
    x0, phase = initial_states(ctrl.model, ctrl.traj, B)
    return ctrl, x0, phase


def _in_step_with_the_handle(ctrl):
    """The handle's GPs against a fresh upload of the Python GPs, under the drop criterion."""
    import torch

    from gpmpc.solver import BatchSolver
    from gpmpc.synthetic import gp_input_box

    spec = ctrl.model
    fresh = BatchSolver(spec, H, B)
    fresh.set_gps(ctrl.gaussian_process)
    for g, gp in enumerate(ctrl.gaussian_process):
        assert gp.train_inputs[0].shape[0] == CAP and gp.train_targets.shape[0] == CAP
        lo, hi = gp_input_box(spec, g)
        Z = np.random.default_rng(20 + g).uniform(lo, hi, size=(64, len(lo)))
        ref = reference(gp.train_inputs[0].cpu().numpy(), gp.train_targets.cpu().numpy(), gp.lengthscale,
                        gp.outputscale, gp.noise, Z)
        Zt = torch.tensor(Z, device="cuda")
        ma, va = ctrl.solver.gp_predict(g, Zt, with_noise=True)
        mf, vf = fresh.gp_predict(g, Zt, with_noise=True)
        for q, a, f in (("mean", ma, mf), ("var", va, vf)):
            e_dev, e_full, ratio = worst_ratio(a.cpu().numpy(), f.cpu().numpy(), ref[q])
            print(f"[online device] gp{g} {q}: e_dev {e_dev:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
            assert ratio <= D.MARGIN_DROP, (g, q, e_dev, e_full)


def test_device_data_episode_matches_the_host_path():
    from gpmpc.learning import run_online_episode

    ctrl, x0, phase = _controller()
    host = run_online_episode(ctrl, x0, STEPS, append_per_step=8, seed=SEED, tstep0=phase, sliding=True)
    assert "pick" not in host   # the default path is today's
    ctrl, x0, phase = _controller()
    out = run_online_episode(ctrl, x0, STEPS, append_per_step=8, seed=SEED, tstep0=phase, sliding=True,
                             device_data=True)
    spec = ctrl.model
    assert out["obs"].shape == (STEPS + 1, B, spec.nx) and out["action"].shape == (STEPS, B, spec.nu)
    assert out["status"].shape == (STEPS, B) and out["inference_time_data"].shape == (STEPS,)
    assert np.isin(out["status"], [0, 2]).all(), np.unique(out["status"])
    assert out["n_train"].tolist() == [48] + [56] * (STEPS - 1)
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(CAP, CAP)] * 2
    _in_step_with_the_handle(ctrl)
    # the host generator's draws, step by step
    rng = np.random.default_rng(SEED)
    for step in range(STEPS):
        assert out["pick"][step].tolist() == rng.choice(B, 8, replace=False).tolist(), step
    for k in ("obs", "action"):
        err = float((np.abs(out[k] - host[k]) / (1 + np.abs(host[k]))).max())
        print(f"[online device] {k}: worst difference to the host path {err:.3e}")
        assert err <= 1e-6, (k, err)


def test_variance_selected_episode():
    from gpmpc.learning import run_online_episode

    ctrl, x0, phase = _controller()
    with pytest.raises(ValueError, match="device_data=True"):
        run_online_episode(ctrl, x0, STEPS, append_per_step=8, seed=SEED, tstep0=phase, sliding=True,
                           select="variance")
    out = run_online_episode(ctrl, x0, STEPS, append_per_step=8, seed=SEED, tstep0=phase, sliding=True,
                             device_data=True, select="variance")
    assert np.isin(out["status"], [0, 2]).all(), np.unique(out["status"])
    assert out["n_train"].tolist() == [48] + [56] * (STEPS - 1)
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(CAP, CAP)] * 2
    for step, pick in enumerate(out["pick"]):
        assert pick.shape == (8,) and len(set(pick.tolist())) == 8 and ((pick >= 0) & (pick < B)).all(), (step, pick)
    _in_step_with_the_handle(ctrl)
    # GPMPC.observe(select="variance") makes the same choice itself: the rows it returns are informative's picks
    import torch

    x, u, xn = (torch.tensor(a, device="cuda") for a in (out["obs"][-2], out["action"][-1], out["obs"][-1]))
    want = ctrl.solver.informative(x, u, 4)
    inputs, targets, accepted, dropped_ok = ctrl.observe(x, u, xn, m=4, select="variance", evict_oldest=True)
    ref_inputs, ref_targets = ctrl.solver.preprocess(x, u, xn, pick=want)
    np.testing.assert_array_equal(inputs.cpu().numpy(), ref_inputs.cpu().numpy())
    np.testing.assert_array_equal(targets.cpu().numpy(), ref_targets.cpu().numpy())
    assert accepted.cpu().numpy().tolist() == [[1], [1]] and dropped_ok.cpu().numpy().tolist() == [[1], [1]]
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(CAP, CAP)] * 2
    for g, idx in enumerate(ctrl.gp_idx):
        gp = ctrl.gaussian_process[g]
        assert gp.train_inputs[0].shape[0] == CAP
        np.testing.assert_array_equal(gp.train_inputs[0][-4:].cpu().numpy(), inputs[:, idx].cpu().numpy())
        np.testing.assert_array_equal(gp.train_targets[-4:].cpu().numpy(), targets[:, g].cpu().numpy())
    with pytest.raises(ValueError, match="pass m, not pick"):
        ctrl.observe(x, u, xn, pick=want, select="variance")
    with pytest.raises(_lib_error(), match="capacity exceeded"):
        ctrl.observe(x, u, xn, m=4)


def _lib_error():
    from gpmpc import _lib

    return _lib.GPMPCError
