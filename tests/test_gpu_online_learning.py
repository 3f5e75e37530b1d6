"""Learning while the loop runs (gpmpc.learning.run_online_episode), MI355X only: a quad2d GP-MPC
batch of 16 with room for 96 training rows starts from 40 rows and appends 4 of every step's 16
transitions over 12 steps.  Every status is 0 or 2, the handle ends with 88 rows, and its GPs agree
with a fresh upload of the controller's Python GPs (which GPMPC.append_data kept in step) under the
append tests' criterion: worst error against the longdouble reference at most 8 times the fresh
upload's (tests/gp_append_ref.py)."""

import numpy as np
import pytest

import gp_ref as R
from gp_append_ref import MARGIN, reference, worst_ratio

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]


def test_online_episode_appends_and_stays_in_step():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpmpc import _lib
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.learning import run_online_episode
    from gpmpc.solver import BatchSolver
    from gpmpc.synthetic import DEFAULT_HYPERS, gp_input_box, initial_states, make_training_data

    B, H, steps = 16, 10, 12
    ctrl = GPMPC("quad2d", horizon=H, batch=B, gp_capacity=96)
    spec = ctrl.model
    gps = []
    for i, (X, y) in enumerate(make_training_data(spec, 40, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS["quad2d"][i])
        gps.append(gp)
    ctrl.set_gaussian_processes(gps)
    x0, phase = initial_states(spec, ctrl.traj, B)
    out = run_online_episode(ctrl, x0, steps, append_per_step=4, seed=11, tstep0=phase)
    assert out["obs"].shape == (steps + 1, B, spec.nx) and out["action"].shape == (steps, B, spec.nu)
    assert out["status"].shape == (steps, B) and out["inference_time_data"].shape == (steps,)
    assert np.isin(out["status"], [0, 2]).all(), np.unique(out["status"])
    assert out["n_train"].tolist() == [44 + 4 * k for k in range(steps)] and out["n_train"][-1] == 88
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(88, 96)] * 2
    assert all(gp.train_inputs[0].shape[0] == 88 and gp.train_targets.shape[0] == 88 for gp in ctrl.gaussian_process)
    # the next append would need 4 of the 8 rows left: fine; 9 rows are refused before any GP changes
    with pytest.raises(_lib.GPMPCError, match="capacity exceeded"):
        ctrl.append_data(np.zeros((9, sum(spec.gp_dims))), np.zeros((9, spec.n_gp)))
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(88, 96)] * 2
    # the handle's GPs against a fresh upload of the Python GPs, under the append criterion
    refs, Zs = [], []
    for g, gp in enumerate(ctrl.gaussian_process):
        lo, hi = gp_input_box(spec, g)
        Z = np.random.default_rng(20 + g).uniform(lo, hi, size=(64, len(lo)))
        Zs.append(Z)
        refs.append(reference(gp.train_inputs[0].cpu().numpy(), gp.train_targets.cpu().numpy(), gp.lengthscale,
                              gp.outputscale, gp.noise, Z))
    fresh = BatchSolver(spec, H, B)
    fresh.set_gps(ctrl.gaussian_process)
    for g, Z in enumerate(Zs):
        Zt = torch.tensor(Z, device="cuda")
        ma, va = ctrl.solver.gp_predict(g, Zt, with_noise=True)
        mf, vf = fresh.gp_predict(g, Zt, with_noise=True)
        for q, a, f in (("mean", ma, mf), ("var", va, vf)):
            e_app, e_full, ratio = worst_ratio(a.cpu().numpy(), f.cpu().numpy(), refs[g][q])
            print(f"[online] gp{g} {q}: e_app {e_app:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
            assert ratio <= MARGIN, (g, q, e_app, e_full)
