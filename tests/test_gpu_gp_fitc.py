"""Building the FITC inducing-point mean on the device (gpmpc_gp_fitc; csrc/gp_fitc.hip), MI355X only.

Setting: a quad2d BatchSolver (GP 0 has d = 1, GP 1 has d = 3), data from gp_drop_ref.data (sf2 = 1,
sn2 = 1e-3, targets sin(3 sum x) + 0.5), inducing rows drawn by default_rng(seed).choice (gp_fitc_ref.py).
The reference is the np.longdouble evaluation of the reference's formula with K_ss + jitter I (which asserts its
own pivots before any GPU call), the yardstick e_full the worst error of the plain float64 solve form.

Criterion.  The handle's worst error (gp_predict mean, gp_mean_grad mean and gradient at the case's 64 points)
is at most MARGIN_FITC e_full (gp_fitc_ref.py: four times the worst ratio of the float64 numpy model of the
kernels, measured on the CPU over the same cases).  The measured ratios are printed per case (run with -s).
Weights are never compared.  The variance must be bit-identical to the one before the build.

Every output is pre-filled with NaN and followed by 64 sentinels (gp_update_util.outputs).
"""

import ctypes
import functools

import numpy as np
import pytest

import gp_drop_ref as D
import gp_fitc_ref as F
import gp_ref as R
import gp_update_util as U
from gp_append_ref import worst_ratio
from gp_update_util import QUANT, REFKEY

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

_torch = U.gpu_torch
_outputs = U.outputs
_upload = U.upload
FQUANT = ("mean", "tmean", "grad")


def _solver(key):
    return U.solver(__name__, key)


@functools.lru_cache(maxsize=None)
def _yardstick(n, M, g, jitter):
    """(reference, float64 solve form) of GP g of the case, computed once."""
    data, idx = F.case_data(n, M)
    dg = data[g]
    return (F.reference(dg["X"], dg["y"], idx, dg["ell"], dg["Z"], jitter=jitter),
            F.numpy64(dg["X"], dg["y"], idx, dg["ell"], dg["Z"], jitter=jitter))


def _compare(case, g, got, full, ref):
    ratios = {}
    for q in FQUANT:
        e_got, e_full, ratios[q] = worst_ratio(got[q], full[REFKEY[q]], ref[REFKEY[q]])
        print(f"[gp-fitc] {case} gp{g} {q}: e {e_got:.3e} e_full {e_full:.3e} ratio {ratios[q]:.4f} (bound {F.MARGIN_FITC:g})")
    for q in FQUANT:
        assert ratios[q] <= F.MARGIN_FITC, (case, g, q, ratios[q])


def _same(a, b):
    return all(np.array_equal(a[q], b[q]) for q in QUANT)


def _read_back(s, g):
    idx, w = s.fitc_mean(g)
    return idx, w


@pytest.mark.parametrize("case", F.CASES, ids=F.CASE_IDS)
def test_build_matches_the_reference(case):
    cid, n, cap, M, jitter, gps = case
    data, idx = F.case_data(n, M)
    yard = {g: _yardstick(n, M, g, jitter) for g in gps}
    s = _solver("A")
    _upload(s, data, slice(0, n), capacity=cap)
    for g in gps:
        dg = data[g]
        before = _outputs(s, g, dg["Z"], f"{cid} exact gp{g}")
        assert s.fitc_size(g) == 0
        assert s.fitc_gp(g, idx, dg["y"], jitter) == 1
        assert s.gp_size(g) == (n, cap) and s.fitc_size(g) == M and s.fitc_sizes[g] == M
        got = _outputs(s, g, dg["Z"], f"{cid} gp{g}")
        assert np.array_equal(got["var"], before["var"]), "the variance moved"
        ref, full = yard[g]
        _compare(cid, g, got, full, ref)
        back, w = _read_back(s, g)
        assert np.array_equal(back, idx) and np.isfinite(w).all()
        # the weights read back give the mean the handle returns
        ev = F.evaluate(dg["X"][idx], w, dg["ell"], dg["Z"])
        assert np.abs(ev["mean"] - got["mean"]).max() <= 1e-9 * max(1.0, np.abs(w).max())
        # a second build gives the same bits; dropping the overlay restores the exact GP's
        assert s.fitc_gp(g, idx, dg["y"], jitter) == 1
        assert _same(got, _outputs(s, g, dg["Z"], f"{cid} again gp{g}"))
        assert np.array_equal(w, _read_back(s, g)[1])
        s.drop_fitc(g)
        assert s.fitc_size(g) == 0 and s.gp_size(g) == (n, cap)
        assert _same(before, _outputs(s, g, dg["Z"], f"{cid} dropped gp{g}"))


def test_inert_rows_take_no_part():
    data, mask, idx, ys = F.inert_case()
    s = _solver("A")
    _upload(s, data, slice(0, 40), capacity=64)
    for g, dg in enumerate(data):
        ref = F.reference(dg["X"], dg["y"], idx, dg["ell"], dg["Z"], jitter=F.JITTER)
        full = F.numpy64(dg["X"], dg["y"], idx, dg["ell"], dg["Z"], jitter=F.JITTER)
        U.nan_block(s, g, dg["d"], 5, seed=31 + g)
        assert s.gp_size(g) == (45, 64)
        before = _outputs(s, g, dg["Z"], f"inert exact gp{g}")
        assert s.fitc_gp(g, idx, ys[g], F.JITTER) == 1
        got = _outputs(s, g, dg["Z"], f"inert gp{g}")
        assert np.array_equal(got["var"], before["var"])
        _compare("inert rows", g, got, full, ref)
        assert s.gp_size(g) == (45, 64) and s.fitc_size(g) == 16


def test_status_zero_leaves_the_handle_unchanged():
    """A duplicate index at jitter 0 (the second pivot is exactly 1 - 1 * 1 = 0 at sf2 = 1), an index naming an
    inert row, an index equal to n and a NaN target of a live row: status 0, outputs bit-identical, first on the
    exact mean, then with a FITC mean installed earlier still in force."""
    data, mask, idx, ys = F.inert_case()
    s = _solver("A")
    _upload(s, data, slice(0, 40), capacity=64)
    for g, dg in enumerate(data):
        U.nan_block(s, g, dg["d"], 5, seed=31 + g)
        inert_idx, past, ynan = idx.copy(), idx.copy(), ys[g].copy()
        inert_idx[5] = 42
        past[15] = 45
        ynan[int(idx[2])] = np.nan
        bad = [("duplicate", np.full(6, 7, dtype=np.int32), ys[g], 0.0), ("inert index", inert_idx, ys[g], F.JITTER),
               ("index n", past, ys[g], F.JITTER), ("NaN target", idx, ynan, F.JITTER)]
        for installed in (False, True):
            if installed:
                assert s.fitc_gp(g, idx, ys[g], F.JITTER) == 1
            before = _outputs(s, g, dg["Z"], f"status gp{g}")
            back = _read_back(s, g)
            for what, ix, y, jit in bad:
                assert s.fitc_gp(g, ix, y, jit) == 0, what
                assert s.fitc_size(g) == (16 if installed else 0) and s.gp_size(g) == (45, 64), what
                assert _same(before, _outputs(s, g, dg["Z"], f"{what} gp{g}")), what
                after = _read_back(s, g)
                assert np.array_equal(back[0], after[0]) and np.array_equal(back[1], after[1]), what


def test_installed_like_an_upload_in_closed_loop():
    """Handle A with a device-built mean against handle B that uploads set_gps(fitc=[(S, w_model)]) with the
    model's weights: three closed-loop steps at n = 40, M = 16 (and the linearisation cache was invalidated)."""
    from helpers import product_gps

    cl = U.ClosedLoop(40)
    idx = F.draw(40, 16, 77)
    sa = cl.handle(cl.data, cl.hyp)
    fitc = []
    for g, (X, y) in enumerate(cl.data):
        sa.reserve_gp(g, 48)
        ell, sf2, sn2 = cl.hyp[g]
        (S, w), ok = F.fitc(X, y, idx, ell, sf2, sn2, jitter=F.JITTER)
        assert ok
        fitc.append((S, w))
    sb = cl.handle(cl.data, cl.hyp)
    sb.set_gps(product_gps(cl.data, cl.hyp), fitc=fitc)
    sb.reset(reset_iterate=True)
    for g, (X, y) in enumerate(cl.data):
        assert sa.fitc_gp(g, idx, y, F.JITTER) == 1
    cl.start(sa, sb)
    cl.three_steps()
    # back on the exact mean the next step computes its first linearisation again
    for g in range(2):
        sa.drop_fitc(g)
    cl.step_after_update()


def test_the_reference_fixture(golden3d):
    """The CPU test's three fixture comparisons with the device mean at gp_Zq in place of the model's."""
    torch = _torch()
    from gpmpc.gp import GaussianProcess
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver
    from test_gp_fitc_cpu import FIXTURE, fixture_gp

    s = BatchSolver(get_spec("quad3d"), 4, 2)
    gps, fx = [], [fixture_gp(golden3d, i) for i in range(3)]
    for X, y, hyp, idx, Zq, want in fx:
        gps.append(GaussianProcess(torch.tensor(X), torch.tensor(y)).set_hyperparameters(*hyp))
    s.set_gps(gps)
    for i, jit, tol in FIXTURE:
        X, y, (ell, sf2, sn2), idx, Zq, want = fx[i]
        s.reserve_gp(i, 40)
        assert s.fitc_gp(i, idx, y, jit * sf2) == 1
        got = _outputs(s, i, Zq, f"fixture gp{i}")
        for q in ("mean", "tmean"):
            err = float(np.abs(got[q] - want).max()) / float(np.abs(want).max())
            print(f"[gp-fitc] fixture gp{i} {q}: {err:.3e} of the largest mean (bound {tol:g})")
            assert err <= tol, (i, q, err)


def _fitc_call(s, g, M, idx, y, jitter):
    from gpmpc import _lib

    ok = ctypes.c_int32(-5)
    _lib.check(s.lib.gpmpc_gp_fitc(s._h, g, M, None if idx is None else idx.data_ptr(),
                                   None if y is None else y.data_ptr(), jitter, ctypes.byref(ok), s._stream()))
    return ok.value


def test_refusals():
    torch = _torch()
    from gpmpc import _lib

    data, idx = F.case_data(40, 16)
    s = _solver("A")
    g, dg = 1, data[1]
    it = torch.tensor(idx, device="cuda")
    yt = torch.tensor(dg["y"], device="cuda")
    # before a reserve
    _upload(s, data, slice(0, 40))
    with U.refused(s, g, dg, -3, "gpmpc_gp_reserve first"):
        _fitc_call(s, g, 16, it, yt, 0.0)
    # a GP set without Linv
    s.set_gps(U.gp_objects(data, slice(0, 40)), with_variance=False)
    with U.refused(s, g, dg, -3, "needs Linv", var=False):
        _fitc_call(s, g, 16, it, yt, 0.0)
    # a FITC upload
    (S, w), ok = F.fitc(dg["X"], dg["y"], idx, dg["ell"], jitter=F.JITTER)
    s.set_gps(U.gp_objects(data, slice(0, 40)), fitc=[None, (S, w)])
    with U.refused(s, g, dg, -3, "FITC upload"):
        _fitc_call(s, g, 16, it, yt, 0.0)
    # the call's own arguments
    _upload(s, data, slice(0, 40), capacity=64)
    big = torch.zeros(41, dtype=torch.int32, device="cuda")
    for M, ix, y, jit, cause in ((0, it, yt, 0.0, "takes no indices"), (41, big, yt, 0.0, "M must be 1 .. n"),
                                 (-1, it, yt, 0.0, "M must be"), (16, None, yt, 0.0, "no indices"),
                                 (16, it, None, 0.0, "no targets"), (16, it, yt, -1e-9, "jitter"),
                                 (16, it, yt, float("nan"), "jitter"), (16, it, yt, float("inf"), "jitter")):
        with U.refused(s, g, dg, -1, cause):
            _fitc_call(s, g, M, ix, y, jit)
    # with a FITC mean installed: every update that changes what it was built from, by the LOVE root's rule
    assert s.fitc_gp(g, idx, dg["y"], F.JITTER) == 1
    Xn, yn = torch.tensor(dg["X"][:4], device="cuda"), torch.tensor(dg["y"][:4], device="cuda")
    raw = [0.5, 0.5, -5.0]
    cause = "a FITC mean is installed: it belongs to the old training set .drop it first, gpmpc_gp_fitc with M = 0"
    for call in (lambda: s.append_gp(g, Xn, yn), lambda: s.drop_gp(g, 4), lambda: s.refactor_gp(g, dg["y"], *U.hyp(dg)),
                 lambda: s.gp_mll(g, dg["y"]), lambda: s.fit_gp(g, dg["y"], raw, 0.05, 2), lambda: s.reserve_gp(g, 80)):
        with U.refused(s, g, dg, -3, cause):
            call()
    # a LOVE root is no obstacle either way, and gpmpc_set_gp_variance_root leaves the overlay alone
    before = _outputs(s, g, dg["Z"], "before the root")
    rank, ok = s.love_root_gp(g, rank=8)
    assert ok == 1 and rank == 8 and s.fitc_size(g) == 16
    assert s.fitc_gp(g, idx, dg["y"], F.JITTER) == 1
    s.drop_love_root(g)
    assert s.fitc_size(g) == 16 and _same(before, _outputs(s, g, dg["Z"], "after the root"))
    # gpmpc_set_gp clears it
    _upload(s, data, slice(0, 40), capacity=64)
    assert s.fitc_size(g) == 0 and s.fitc_sizes == [0, 0]
    assert s.append_gp(g, Xn, yn).cpu().tolist() == [1]


def test_controller_learns_in_sparse_mode():
    torch = _torch()
    from gpmpc import _lib
    from gpmpc.gpmpc import GPMPC
    from gpmpc.synthetic import initial_states
    from helpers import problem, product_gps

    spec, data, hyp = problem("quad2d", 48)
    first = [(X[:40], y[:40]) for X, y in data]
    inputs = np.hstack([X[40:] for X, _ in data])
    targets = np.column_stack([y[40:] for _, y in data])
    kw = dict(horizon=5, batch=4, sparse_gp=True, gp_capacity=64, max_gp_samples=16, variance="exact")
    ctrl = GPMPC("quad2d", fitc="device", fitc_jitter=1e-8, **kw)
    ctrl.set_gaussian_processes(product_gps(first, hyp))
    ctrl.reset()
    s = ctrl.solver
    assert np.array_equal(ctrl.fitc_idx, np.random.default_rng(1337).choice(range(40), size=16, replace=False))
    assert [s.fitc_size(g) for g in range(2)] == [16, 16] and s.gp_size(0) == (40, 64)
    x0, phase = initial_states(spec, ctrl.traj, 4)
    obs = torch.tensor(x0, device="cuda")
    ts = torch.tensor(phase, dtype=torch.int32, device="cuda")
    ctrl.select_action_batch(obs, ts, check=True)
    flags = ctrl.append_data(inputs, targets)
    assert [f.cpu().tolist() for f in flags] == [[1], [1]]
    assert s.gp_size(0) == (48, 64) and [s.fitc_size(g) for g in range(2)] == [16, 16]
    rng = np.random.default_rng(1337)
    rng.choice(range(40), size=16, replace=False)
    want = rng.choice(range(48), size=16, replace=False)
    assert np.array_equal(ctrl.fitc_idx, want)
    for g, (X, y) in enumerate(data):
        ell, sf2, sn2 = hyp[g]
        Z = X[::3] + 0.01
        ref = F.reference(X, y, want, ell, Z, sf2, sn2, 1e-8)
        full = F.numpy64(X, y, want, ell, Z, sf2, sn2, 1e-8)
        assert np.array_equal(s.fitc_mean(g)[0], want)
        _compare("controller 48 rows", g, _outputs(s, g, Z, f"controller gp{g}"), full, ref)
    ctrl.drop_oldest(8)
    assert s.gp_size(0) == (40, 64) and [s.fitc_size(g) for g in range(2)] == [16, 16]
    ctrl.refresh_gps()
    assert [s.fitc_size(g) for g in range(2)] == [16, 16]
    flags = ctrl.refit_hyperparameters(0.05, 3, fit="device")
    assert len(flags) == 2 and [s.fitc_size(g) for g in range(2)] == [16, 16]
    u = ctrl.select_action_batch(obs, ts, check=True)
    assert torch.isfinite(u).all()
    # the host mode refuses where the device mode learns
    host = GPMPC("quad2d", **kw)
    host.set_gaussian_processes(product_gps(first, hyp))
    host.reset()
    with pytest.raises(_lib.GPMPCError, match="not available in sparse"):
        host.append_data(inputs, targets)
