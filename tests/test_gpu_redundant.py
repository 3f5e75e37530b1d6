"""The rows the GPs would miss least on the device (gpmpc_gp_redundant; csrc/gp_drop.hip) and the Python surface of
the eviction by choice, MI355X only.

The picks are compared with the float64 model in the kernel's summation order (gp_drop_rows_ref.redundant_f64), which
tests/test_gp_redundant_cpu.py holds to the longdouble reference; the scores must agree within what that test allows
at each step, a thousandth of the gap between the best score and the runner-up."""

import numpy as np
import pytest

import gp_drop_ref as D
import gp_drop_rows_ref as DR
import gp_ref as R
import gp_update_util as U
from gp_append_ref import reference, worst_ratio

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

_torch = U.gpu_torch


def _solver(key):
    return U.solver(__name__, key)


def _redundant(s, m, what):
    """gpmpc_gp_redundant with guarded outputs; returns (picks, scores, ok) on the host."""
    torch = _torch()
    from gpmpc import _lib

    pk, sc, ok = U.guarded(m, torch.int32), U.guarded(m), U.guarded(1, torch.int32)
    _lib.check(s.lib.gpmpc_gp_redundant(s._h, m, pk.data_ptr(), sc.data_ptr(), ok.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return U.read(pk, m, what + " picks"), U.read(sc, m, what + " scores"), int(U.read(ok, 1, what + " ok")[0])


@pytest.mark.parametrize("n", [24, 40, 272])
def test_picks_are_the_models(n):
    torch = _torch()
    ms = [1, 17, min(n - 1, 33)]
    assert (n, ms[-1]) in DR.GPU_RED_CASES   # (whose gap condition tests/test_gp_redundant_cpu.py checks step by step)
    c = DR.red_case(n, ms[-1])
    model, ref = c["model"], c["ref"]
    s = _solver("A")
    U.upload(s, c["data"], slice(0, n), capacity=n if n != 40 else 56)
    Zt = [torch.tensor(dg["Z"], device="cuda") for dg in c["data"]]
    before = [tuple(t.cpu().numpy() for t in s.gp_predict(g, Zt[g], with_noise=True)) for g in range(2)]
    for m in ms:
        picks, scores, ok = _redundant(s, m, f"n {n} m {m}")
        allowed = ref["gaps"][:m] / DR.GAP_FACTOR
        want = model["picks"][:m].tolist()
        if DR.structural_tie(n, m, m - 1):
            # with two rows left the scores are equal in exact arithmetic: either row may leave, and the score is held
            # to the conditioning of K + sn2 I instead of to a gap that is zero
            left = np.flatnonzero(~np.isnan(ref["tables"][m - 1].astype(np.float64))).tolist()
            assert picks[-1] in left
            want[-1] = int(picks[-1])
            allowed[-1] = 64 * (n * DR.SF2 / DR.SN2) * R.EPS64 * model["scores"][m - 1]
        assert ok == 1 and picks.tolist() == want, (n, m, picks.tolist())
        err = np.abs(scores - model["scores"][:m])
        print(f"[redundant] n {n} m {m}: worst score difference to the model {err.max():.3e}, least allowed "
              f"{allowed.min():.3e}")
        assert (err <= allowed).all(), (n, m)
        assert (np.diff(scores) >= 0).all() and (scores > 0).all()
        again = _redundant(s, m, f"n {n} m {m} again")
        assert np.array_equal(picks, again[0]) and np.array_equal(scores, again[1]) and again[2] == 1
    # the Python call, and the GPs untouched
    pk, sc, ok = s.redundant(ms[1], scores=True)
    assert pk.is_cuda and pk.dtype == torch.int32 and pk.cpu().tolist() == model["picks"][:ms[1]].tolist()
    assert sc.shape == (ms[1],) and ok.cpu().tolist() == [1] and s.redundant(1).cpu().tolist() == [int(model["picks"][0])]
    after = [tuple(t.cpu().numpy() for t in s.gp_predict(g, Zt[g], with_noise=True)) for g in range(2)]
    for b, a in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(b, a))
    assert [s.gp_size(g)[0] for g in range(2)] == [n, n]


def test_a_duplicated_row_leaves_first_and_alone():
    """Rows a and b, the lowest and the highest of the seven rows that outlast 33 picks at n = 40, are made copies of
    each other in both GPs.  While both are there each says all the other says, and what a copy observed with noise
    sn2 leaves of a row is at most sf2 sn2 / (sf2 + sn2): one of them is picked (the model: at step 8).  With it
    gone the other is the row that outlasts the picks again.  The twins' scores agree to rounding, not in bits (they
    are sums over different rows of the factor), so which of the two leaves is not fixed; the picks are the model's
    up to that."""
    n, m = 40, 33
    rest = np.setdiff1d(np.arange(n), DR.red_case(n, m)["model"]["picks"])
    a, b = int(rest[0]), int(rest[-1])
    data = DR.data(n)
    for dg in data:
        dg["X"][b], dg["y"][b] = dg["X"][a], dg["y"][a]
    states = [D.upload_state(dg["X"], dg["y"], dg["ell"]) for dg in data]
    model = DR.redundant_f64([st[1] for st in states], [(DR.SF2, DR.SN2)] * 2, m)
    s = _solver("A")
    U.upload(s, data, slice(0, n), capacity=n)
    picks, scores, ok = _redundant(s, m, "twins")
    canon = lambda p: [a if int(v) == b else int(v) for v in p]   # noqa: E731
    assert ok == 1 and canon(picks) == canon(model["picks"]), (picks.tolist(), model["picks"].tolist())
    at = canon(picks).index(a)
    assert canon(picks).count(a) == 1 and scores[at] < DR.SN2 / DR.SF2
    rel = np.abs(scores / model["scores"] - 1).max()
    print(f"[redundant] twins {a}, {b}: row {int(picks[at])} leaves at step {at}; worst relative score difference to "
          f"the model {rel:.3e}")
    # two float64 evaluations of quantities whose condition is that of K + sn2 I, at most n sf2 / sn2
    assert rel <= 64 * (n * DR.SF2 / DR.SN2) * R.EPS64 and (np.diff(scores) >= 0).all()


def test_a_row_inert_in_every_gp_is_picked_first():
    data = DR.data(24)
    s = _solver("A")
    U.upload(s, data, slice(0, 20), capacity=32)
    for g, dg in enumerate(data):
        U.nan_block(s, g, dg["d"], 1, 3 + g)
        assert s.append_gp(g, dg["X"][20:24], dg["y"][20:24]).cpu().tolist() == [1]
    picks, scores, ok = _redundant(s, 3, "inert")
    assert ok == 1 and picks[0] == 20 and scores[0] == 0.0 and (scores[1:] > 0).all() and 20 not in picks[1:].tolist()
    # the live rows rank as in a GP without the inert row
    states = [D.upload_state(dg["X"], dg["y"], dg["ell"]) for dg in data]
    model = DR.redundant_f64([st[1] for st in states], [(DR.SF2, DR.SN2)] * 2, 2)
    assert [p + (1 if p >= 20 else 0) for p in model["picks"].tolist()] == picks[1:].tolist()


def test_refusals():
    from gpmpc import _lib

    data = DR.data(24)
    s = _solver("A")
    U.upload(s, data, slice(0, 24), capacity=32)
    torch = _torch()
    Zt = torch.tensor(data[0]["Z"], device="cuda")
    before = [t.cpu().numpy() for t in s.gp_predict(0, Zt, with_noise=True)]
    for m, cause in ((0, "m must be in 1"), (24, "at least one row stays"), (257, "m must be")):
        with pytest.raises(_lib.GPMPCError, match=rf"error -1: .*{cause}"):
            s.redundant(m)
    s.drop_gp(1, 2)
    with pytest.raises(_lib.GPMPCError, match=r"error -3: .*differ in their training rows"):
        s.redundant(3)
    after = [t.cpu().numpy() for t in s.gp_predict(0, Zt, with_noise=True)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    s.set_gps(U.gp_objects(data, slice(0, 24)), with_variance=False)
    with pytest.raises(_lib.GPMPCError, match=r"error -3: .*Linv"):
        s.redundant(3)
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    with pytest.raises(_lib.GPMPCError, match=r"error -3: GP not set"):
        BatchSolver(get_spec("quad2d"), 5, 2).redundant(1)


# ------------------------------------------------------------------------------------------- the Python surface
B, H, CAP = 16, 10, 56


def _controller(**kw):
    torch = _torch()
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.synthetic import DEFAULT_HYPERS, initial_states, make_training_data

    ctrl = GPMPC("quad2d", horizon=H, batch=B, gp_capacity=CAP, **kw)
    gps = []
    for i, (X, y) in enumerate(make_training_data(ctrl.model, 48, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS["quad2d"][i])
        gps.append(gp)
    ctrl.set_gaussian_processes(gps)
    x0, phase = initial_states(ctrl.model, ctrl.traj, B)
    return ctrl, x0, phase


def _in_step_with_the_handle(ctrl, rows, what):
    """The handle's GPs against a fresh upload of the Python GPs' rows, under the margin of the drop."""
    torch = _torch()
    from gpmpc.solver import BatchSolver
    from gpmpc.synthetic import gp_input_box

    fresh = BatchSolver(ctrl.model, H, B)
    fresh.set_gps(ctrl.gaussian_process)
    for g, gp in enumerate(ctrl.gaussian_process):
        assert gp.train_inputs[0].shape[0] == rows and gp.train_targets.shape[0] == rows
        assert ctrl.solver.gp_size(g) == (rows, CAP)
        lo, hi = gp_input_box(ctrl.model, g)
        Z = np.random.default_rng(20 + g).uniform(lo, hi, size=(64, len(lo)))
        ref = reference(gp.train_inputs[0].cpu().numpy(), gp.train_targets.cpu().numpy(), gp.lengthscale,
                        gp.outputscale, gp.noise, Z)
        Zt = torch.tensor(Z, device="cuda")
        ma, va = ctrl.solver.gp_predict(g, Zt, with_noise=True)
        mf, vf = fresh.gp_predict(g, Zt, with_noise=True)
        for q, a, f in (("mean", ma, mf), ("var", va, vf)):
            e_dev, e_full, ratio = worst_ratio(a.cpu().numpy(), f.cpu().numpy(), ref[q])
            print(f"[evict] {what} gp{g} {q}: e_dev {e_dev:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
            assert ratio <= DR.MARGIN, (what, g, q, e_dev, e_full)


@pytest.mark.parametrize("variance", ["exact", "love"])
def test_observe_and_drop_rows_keep_the_python_gps_in_step(variance, monkeypatch):
    torch = _torch()
    if variance == "love":   # the root at a small size: every GP above 16 rows gets one of rank 8
        monkeypatch.setattr("gpmpc.gpmpc.LOVE_CHOLESKY_ROWS", 16)
    ctrl, x0, phase = _controller(variance=variance)
    ctrl.reset()
    s = ctrl.solver
    if variance == "love":
        s.love_rank = 8
    x = torch.tensor(x0, device="cuda")
    u = ctrl.select_action_batch(x, torch.tensor(phase, dtype=torch.int32, device="cuda"))
    xn = s.plant_step(x, u.clone(), torch.tensor(phase, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="pass one of them"):
        ctrl.observe(x, u, xn, m=16, evict="redundant", evict_oldest=True)
    with pytest.raises(ValueError, match="evict must be"):
        ctrl.observe(x, u, xn, m=16, evict="oldest")
    want = s.redundant(8).cpu().tolist()                  # 48 + 16 rows, room for 56
    old = [gp.train_inputs[0].cpu().numpy().copy() for gp in ctrl.gaussian_process]
    inputs, targets, accepted, dropped_ok = ctrl.observe(x, u, xn, m=16, evict="redundant")
    assert accepted.cpu().tolist() == [[1], [1]] and dropped_ok.cpu().tolist() == [[1], [1]]
    kept = np.setdiff1d(np.arange(48), want)
    assert len(kept) == 40
    for g, idx in enumerate(ctrl.gp_idx):
        gp = ctrl.gaussian_process[g]
        X, y = gp.train_inputs[0].cpu().numpy(), gp.train_targets.cpu().numpy()
        assert np.array_equal(X[:40], old[g][kept]) and np.array_equal(X[40:], inputs[:, idx].cpu().numpy())
        assert np.array_equal(y[40:], targets[:, g].cpu().numpy())
        if variance == "love":
            assert s.love_ranks[g] is not None
    _in_step_with_the_handle(ctrl, CAP, f"observe ({variance})")
    flags = ctrl.drop_rows([55, 3, 20, 21])
    assert [f.cpu().tolist() for f in flags] == [[1], [1]]
    _in_step_with_the_handle(ctrl, CAP - 4, f"drop_rows ({variance})")
    with pytest.raises(ValueError, match="at least one row stays"):
        ctrl.drop_rows(list(range(CAP - 4)))


def test_episode_with_eviction_by_choice():
    from gpmpc.learning import run_online_episode

    ctrl, x0, phase = _controller()
    out = run_online_episode(ctrl, x0, 6, append_per_step=8, seed=11, tstep0=phase, sliding=True, device_data=True,
                             evict="redundant")
    assert np.isin(out["status"], [0, 2]).all(), np.unique(out["status"])
    assert out["n_train"].tolist() == [CAP] * 6
    _in_step_with_the_handle(ctrl, CAP, "episode")
