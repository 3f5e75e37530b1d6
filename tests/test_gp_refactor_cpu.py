"""Refactorising an uploaded GP: what needs no GPU.

* The float64 numpy model of the blocked algorithm (tests/gp_refactor_ref.py) against the
  np.longdouble recompute (gp_append_ref.reference, which asserts var >= sn2 / 2 first, for the new
  hyperparameters too), over every state tests/test_gpu_gp_refactor.py judges: M is lower
  triangular, the status is 1 and the model's worst error is at most MARGIN_REFACTOR times that of
  the float64 full recompute the upload path uses (the measured ratios are printed: run with -s).
  Their maximum is recomputed and must not ask for a larger margin than the stored one.
* Inert rows end as exact zeros whatever their target; a NaN target on a live row clears the status.
* An append and a drop that follow a refactorisation keep their own margins.
* ``GPMPC.refresh_gps`` / ``refit_hyperparameters`` against a recording stand-in for the solver
  handle; ``run_online_episode``'s ``refresh_every`` default.
* The ctypes signature table lists gpmpc_gp_refactor with the header's types, and a null handle is
  refused without a device.
"""

import ctypes
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import gp_drop_ref as D
import gp_ref as R
import gp_refactor_ref as G
from gp_append_ref import MARGIN, reference, worst_ratio

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmpc_mi355x.h"
extended = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")
RATIOS: dict = {}
_CASES: list = []


def _cases():
    if not _CASES:
        _CASES.extend(G.model_cases())
    return _CASES


def _ratios(tag, case, g, state, dg, rows, hyp):
    ell, sf2, sn2 = hyp
    ref = reference(dg["X"][rows], dg["y"][rows], ell, sf2, sn2, dg["Z"])
    full = D.predict(D.upload_state(dg["X"][rows], dg["y"][rows], ell, sf2, sn2), ell, dg["Z"], sf2, sn2)
    got = D.predict(state, ell, dg["Z"], sf2, sn2)
    out = {}
    for q in ("mean", "var", "grad"):
        e_model, e_full, out[q] = worst_ratio(got[q], full[q], ref[q])
        print(f"[gp-refactor model] {tag}{case} gp{g} {q}: e_model {e_model:.3e} e_full {e_full:.3e} ratio {out[q]:.3f}")
    return out


@extended
def test_model_matches_full_recompute():
    for case, g, state, ok, dg, rows, hyp in _cases():
        X, M, alpha = state
        assert ok, (case, g)
        assert np.array_equal(M, np.tril(M)) and np.isfinite(M).all() and np.isfinite(alpha).all()
        for q, r in _ratios("", case, g, state, dg, rows, hyp).items():
            RATIOS[(case, g, q)] = r
            assert r <= G.MARGIN_REFACTOR, (case, g, q, r)


@extended
def test_zz_margin_is_the_recorded_one():
    """MARGIN_REFACTOR = ceil(4 R_MODEL), and the ratio recomputed here asks for no larger one."""
    if not RATIOS:   # (run on its own: nothing to report)
        return
    for q in ("mean", "var", "grad"):
        k = max((k for k in RATIOS if k[2] == q), key=lambda k: RATIOS[k])
        print(f"[gp-refactor model] worst {q}: {RATIOS[k]:.3f} ({k[0]}, gp{k[1]})")
    worst = max(RATIOS.values())
    print(f"[gp-refactor model] worst ratio overall: {worst:.3f}; R_MODEL {G.R_MODEL}, MARGIN_REFACTOR {G.MARGIN_REFACTOR}")
    assert G.MARGIN_REFACTOR == math.ceil(4 * G.R_MODEL)
    assert G.MARGIN_REFACTOR >= math.ceil(4 * worst), (worst, G.MARGIN_REFACTOR)


def test_model_inert_rows_end_as_exact_zeros():
    data, mask, live = G.inert_case()
    for dg in data:
        X, y = np.zeros((39, dg["d"])), np.full(39, np.nan)
        X[live], y[live] = dg["X"][:28], dg["y"][:28]
        (Xs, M, alpha), ok = G.refactor(X, y, dg["ell"], inert=mask)
        assert ok
        assert not M[mask].any() and not M[:, mask].any() and not alpha[mask].any()
        assert (np.diag(M)[live] > 0).all() and alpha[live].all()
        # the live rows' factor is that of the live rows alone
        (_, M2, a2), ok2 = G.refactor(dg["X"][:28], dg["y"][:28], dg["ell"])
        assert ok2
        np.testing.assert_allclose(M[np.ix_(live, live)], M2, rtol=0, atol=1e-9)
        np.testing.assert_allclose(alpha[live], a2, rtol=0, atol=1e-7)
        # a NaN target on a live row clears the status
        y[3] = np.nan
        assert not G.refactor(X, y, dg["ell"], inert=mask)[1]


@extended
def test_model_append_and_drop_after_a_refactorisation():
    for g, dg in enumerate(D.data(48 + 16, seed=1600)):
        state, ok = G.refactor(dg["X"][:48], dg["y"][:48], dg["ell"])
        assert ok
        state = D.append_block(state, dg["X"][48:64], dg["y"][48:64], dg["ell"])
        hyp = (dg["ell"], G.SF2, G.SN2)
        for q, r in _ratios("then append: ", "48 + 16", g, state, dg, slice(0, 64), hyp).items():
            assert r <= MARGIN, (g, q, r)
        state, flags = D.drop_oldest(state, 16)
        assert flags == [1]
        for q, r in _ratios("then drop: ", "64 - 16", g, state, dg, slice(16, 64), hyp).items():
            assert r <= D.MARGIN_BULK, (g, q, r)


# ------------------------------------------------------------------------------- Python mirrors
class _Handle:
    """Stands in for BatchSolver: refactor_gp recorded."""

    def __init__(self):
        self.calls = []

    def refactor_gp(self, g, y, ell, sf2, sn2):
        self.calls.append((g, y.clone(), ell, sf2, sn2))
        return torch.ones(1, dtype=torch.int32)


def _controller(n):
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.models import get_spec

    spec = get_spec("quad2d")
    ctrl = object.__new__(GPMPC)   # (the constructor opens a solver handle on the GPU)
    ctrl.model, ctrl.sparse, ctrl.device, ctrl._requires_recompile = spec, False, "cpu", False
    ctrl.gp_idx = GPMPC._gp_columns(spec)
    ctrl.solver = _Handle()
    rng = np.random.default_rng(3)
    ctrl.gaussian_process = []
    for d in spec.gp_dims:
        X = rng.uniform(-1, 1, (n, d))
        gp = GaussianProcess(torch.tensor(X), torch.tensor(np.sin(3 * X.sum(1)) + 0.5))
        ctrl.gaussian_process.append(gp.set_hyperparameters(1.0 + 0.1 * d, 1.0, 1e-3))
    return ctrl


def test_refresh_gps_passes_targets_and_hyperparameters():
    from gpmpc import _lib

    ctrl = _controller(20)
    flags = ctrl.refresh_gps()
    assert len(flags) == 2 and [c[0] for c in ctrl.solver.calls] == [0, 1]
    for (g, y, ell, sf2, sn2), gp in zip(ctrl.solver.calls, ctrl.gaussian_process):
        assert torch.equal(y, gp.train_targets)
        assert (ell, sf2, sn2) == (gp.lengthscale, gp.outputscale, gp.noise)
    ctrl.solver.calls.clear()
    gp0 = ctrl.gaussian_process[0]
    gp0.device_layout("cpu")
    new = [(0.7, 2.0, 5e-3), (0.9, 1.5, 2e-3)]
    ctrl.refresh_gps(new)
    for (g, y, ell, sf2, sn2), gp, want in zip(ctrl.solver.calls, ctrl.gaussian_process, new):
        assert (ell, sf2, sn2) == want
        assert gp.lengthscale == pytest.approx(want[0], rel=1e-12) and gp.outputscale == pytest.approx(want[1], rel=1e-12)
        assert gp.noise == pytest.approx(want[2], rel=1e-12)
    assert gp0._dev is None and gp0.K is None   # the cached layout belonged to the old hyperparameters
    assert ctrl._requires_recompile is False
    with pytest.raises(ValueError):
        ctrl.refresh_gps(new[:1])
    ctrl.sparse = True
    for call in (ctrl.refresh_gps, lambda: ctrl.refit_hyperparameters(0.01, 2)):
        with pytest.raises(_lib.GPMPCError, match="sparse"):
            call()
    ctrl.sparse, ctrl._requires_recompile = False, True
    with pytest.raises(AssertionError, match="must be uploaded"):
        ctrl.refresh_gps()


def test_refit_hyperparameters_fits_then_refreshes_without_a_recompile():
    ctrl = _controller(24)
    before = [(gp.lengthscale, gp.outputscale, gp.noise) for gp in ctrl.gaussian_process]
    flags = ctrl.refit_hyperparameters(lr=0.05, iterations=5)
    assert len(flags) == 2 and ctrl._requires_recompile is False
    for (g, y, ell, sf2, sn2), gp, old in zip(ctrl.solver.calls, ctrl.gaussian_process, before):
        assert (ell, sf2, sn2) == (gp.lengthscale, gp.outputscale, gp.noise) != old
        assert torch.equal(y, gp.train_targets)


def test_refresh_every_defaults_to_never():
    from gpmpc.learning import run_online_episode

    assert inspect.signature(run_online_episode).parameters["refresh_every"].default == 0


# ------------------------------------------------------------------------------------- C ABI
def test_signature_table_lists_refactor_with_the_header_types():
    from gpmpc import _lib

    text = HEADER.read_text()
    m = re.search(r"gpmpc_status\s+gpmpc_gp_refactor\(([^)]*)\)\s*;", text)
    assert m, "gpmpc_gp_refactor is not declared in the header"
    args = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["gpmpc_handle*", "int32_t", "const double*", "double", "double", "double", "int32_t*", "void*"]
    res, table = _lib.SIGNATURES["gpmpc_gp_refactor"]
    assert res is ctypes.c_int32
    assert table == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                     ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    assert "gp_refactor.hip" in _lib.HASHED


def test_null_handle_is_refused_without_a_device():
    from gpmpc import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load(require_gpu=False)
    st = lib.gpmpc_gp_refactor(None, 0, None, 1.0, 1.0, 1e-3, None, None)
    assert st == -1   # GPMPC_ERR_ARG
    assert b"null handle" in lib.gpmpc_last_error()
