"""Learning on a moving window while the loop runs (gpmpc.learning.run_online_episode with
sliding=True), MI355X only: a quad2d GP-MPC batch of 16 with room for 56 training rows starts from
40 rows and appends 8 of every step's 16 transitions over 12 steps.  The first two steps fill the
capacity; from then on every step drops its 8 oldest rows on the device first
(GPMPC.append_data(evict_oldest=True) -> gpmpc_gp_drop_oldest), so the handle stays at 56 rows.
Every status is 0 or 2, as in the non-sliding episode (tests/test_gpu_online_learning.py), and the
handle's GPs agree with a fresh upload of the controller's Python GPs (which append_data and
drop_oldest kept in step) under the drop tests' criterion: worst error against the longdouble
reference at most MARGIN_DROP times the fresh upload's (tests/gp_drop_ref.py).  The tighter
MARGIN_BULK does not apply here: it was measured at sf2 / sn2 = 1e3, and the controller's GPs have
sf2 / sn2 = 2.5e5 and 5e5 (DEFAULT_HYPERS), where ten consecutive drops cost more: the numpy model
gives a variance ratio of 80 on such a window of random rows, the MI355X measured 0.1 (gp0 mean),
14 (gp0 variance), 25 (gp1 mean) and 266 (gp1 variance: 1.3e-8 against 5.0e-11, on variances no
smaller than sn2 = 1e-4)."""

import numpy as np
import pytest

import gp_drop_ref as D
import gp_ref as R
from gp_append_ref import reference, worst_ratio

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]


def test_online_episode_slides_and_stays_in_step():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.learning import run_online_episode
    from gpmpc.solver import BatchSolver
    from gpmpc.synthetic import DEFAULT_HYPERS, gp_input_box, initial_states, make_training_data

    B, H, steps, cap = 16, 10, 12, 56
    ctrl = GPMPC("quad2d", horizon=H, batch=B, gp_capacity=cap)
    spec = ctrl.model
    gps, first = [], []
    for i, (X, y) in enumerate(make_training_data(spec, 40, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS["quad2d"][i])
        gps.append(gp)
        first.append(np.asarray(X, dtype=np.float64).reshape(40, -1))
    ctrl.set_gaussian_processes(gps)
    x0, phase = initial_states(spec, ctrl.traj, B)
    out = run_online_episode(ctrl, x0, steps, append_per_step=8, seed=11, tstep0=phase, sliding=True)
    assert out["obs"].shape == (steps + 1, B, spec.nx) and out["action"].shape == (steps, B, spec.nu)
    assert np.isin(out["status"], [0, 2]).all(), np.unique(out["status"])
    assert out["n_train"].tolist() == [48] + [56] * (steps - 1)
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(cap, cap)] * 2
    # 96 rows went in, 80 came out: none of the 40 uploaded rows is left
    for g, gp in enumerate(ctrl.gaussian_process):
        X = gp.train_inputs[0].cpu().numpy()
        assert X.shape[0] == cap and gp.train_targets.shape[0] == cap
        assert not (X[:, None, :] == first[g][None, :, :]).all(-1).any()
    # the handle's GPs against a fresh upload of the Python GPs, under the drop criterion
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
            e_drop, e_full, ratio = worst_ratio(a.cpu().numpy(), f.cpu().numpy(), refs[g][q])
            print(f"[online sliding] gp{g} {q}: e_drop {e_drop:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
            assert ratio <= D.MARGIN_DROP, (g, q, e_drop, e_full)
