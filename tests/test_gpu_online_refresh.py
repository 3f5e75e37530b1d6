"""Refreshing and refitting the uploaded GPs while the loop runs, MI355X only.

* gpmpc.learning.run_online_episode(sliding=True, refresh_every=4) on the setting of
  tests/test_gpu_online_sliding.py: a quad2d GP-MPC batch of 16 with room for 56 training rows starts
  from 40 rows and appends 8 of every step's 16 transitions over 12 steps, dropping its 8 oldest rows
  first once the capacity is reached; every fourth step ends with GPMPC.refresh_gps (a
  refactorisation on the device, gpmpc_gp_refactor), the last one included.  The handle's GPs then
  agree with a fresh upload of the controller's Python GPs within MARGIN_REFACTOR
  (tests/gp_refactor_ref.py); without the refresh the same episode is only held to MARGIN_DROP, and
  measured a ratio of 266 for GP 1's variance at the controller's sf2 / sn2 of 2.5e5 and 5e5.
* GPMPC.refit_hyperparameters(lr, 5 iterations) on 40 rows: the handle's predictions match a fresh
  upload of the refitted Python GPs within MARGIN_REFACTOR, with no recompile pending.
"""

import numpy as np
import pytest

import gp_ref as R
import gp_refactor_ref as G
from gp_append_ref import reference, worst_ratio

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

B, H = 16, 10


def _controller(cap):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.synthetic import DEFAULT_HYPERS, make_training_data

    ctrl = GPMPC("quad2d", horizon=H, batch=B, gp_capacity=cap)
    gps = []
    for i, (X, y) in enumerate(make_training_data(ctrl.model, 40, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS["quad2d"][i])
        gps.append(gp)
    ctrl.set_gaussian_processes(gps)
    return ctrl


def _judge(tag, ctrl):
    """The handle's GPs against a fresh upload of the Python GPs: mean and variance within MARGIN_REFACTOR."""
    import torch

    from gpmpc.solver import BatchSolver
    from gpmpc.synthetic import gp_input_box

    spec = ctrl.model
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
            e, e_full, ratio = worst_ratio(a.cpu().numpy(), f.cpu().numpy(), refs[g][q])
            print(f"[{tag}] gp{g} {q}: e {e:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
            assert ratio <= G.MARGIN_REFACTOR, (tag, g, q, e, e_full)


def test_online_episode_refreshes_every_fourth_step():
    from gpmpc.learning import run_online_episode
    from gpmpc.synthetic import initial_states

    steps, cap = 12, 56
    ctrl = _controller(cap)
    x0, phase = initial_states(ctrl.model, ctrl.traj, B)
    calls = []
    refresh = ctrl.refresh_gps
    ctrl.refresh_gps = lambda *a, **kw: calls.append(ctrl.solver.gp_size(0)[0]) or refresh(*a, **kw)
    out = run_online_episode(ctrl, x0, steps, append_per_step=8, seed=11, tstep0=phase, sliding=True, refresh_every=4)
    assert calls == [56, 56, 56]   # after the appends of steps 4, 8 and 12
    assert np.isin(out["status"], [0, 2]).all(), np.unique(out["status"])
    assert out["n_train"].tolist() == [48] + [56] * (steps - 1)
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(cap, cap)] * 2
    assert ctrl._requires_recompile is False
    _judge("online refresh", ctrl)


def test_refit_hyperparameters_matches_a_fresh_upload():
    ctrl = _controller(56)
    ctrl.reset()
    before = [(gp.lengthscale, gp.outputscale, gp.noise) for gp in ctrl.gaussian_process]
    flags = ctrl.refit_hyperparameters(lr=0.05, iterations=5)
    assert [f.cpu().tolist() for f in flags] == [[1], [1]]
    assert ctrl._requires_recompile is False
    after = [(gp.lengthscale, gp.outputscale, gp.noise) for gp in ctrl.gaussian_process]
    assert all(a != b for a, b in zip(after, before))
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(40, 56)] * 2
    _judge("refit", ctrl)
