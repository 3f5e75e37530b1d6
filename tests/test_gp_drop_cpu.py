"""Dropping the oldest GP training rows: what needs no GPU.

* The float64 numpy model of the update (tests/gp_drop_ref.py) against the np.longdouble recompute
  of the kept rows (gp_append_ref.reference), over the cases of tests/test_gpu_gp_drop.py: M' is
  lower triangular, inert rows are exact zeros, every flag is 1 and the model's worst error is at
  most MARGIN_DROP times that of a float64 full recompute, MARGIN_BULK times where two rows or
  more are kept (the measured ratios are printed: run with -s; their maxima are the R_MODEL and
  R_BULK gp_drop_ref.py and DESIGN section 12 record).
* ``GaussianProcess.drop_oldest`` followed by ``device_layout`` equals a GP built on the sliced data.
* ``GPMPC.append_data``: past the capacity it still raises by default; with ``evict_oldest=True``
  it drops exactly the excess first (against a recording stand-in for the solver handle).
* The ctypes signature table lists gpmpc_gp_drop_oldest with the header's types, and a null handle
  is refused without a device.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import gp_drop_ref as D
import gp_ref as R
from gp_append_ref import reference, worst_ratio

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmpc_mi355x.h"
extended = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")
RATIOS: dict = {}


def _judge(case, g, state, dg, rows):
    """Ratios of the model state against a float64 full recompute of `rows` of the GP's data."""
    ref = reference(dg["X"][rows], dg["y"][rows], dg["ell"], D.SF2, D.SN2, dg["Z"])
    full = D.predict(D.upload_state(dg["X"][rows], dg["y"][rows], dg["ell"]), dg["ell"], dg["Z"])
    got = D.predict(state, dg["ell"], dg["Z"])
    for q in ("mean", "var", "grad"):
        e_model, e_full, ratio = worst_ratio(got[q], full[q], ref[q])
        RATIOS[(case, g, q)] = ratio
        print(f"[gp-drop model] {case} gp{g} {q}: e_model {e_model:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
    bound = D.margin(state[0].shape[0])
    for q in ("mean", "var", "grad"):
        assert RATIOS[(case, g, q)] <= bound <= D.MARGIN_DROP, (case, g, q, RATIOS[(case, g, q)])


@extended
@pytest.mark.parametrize("case,n,drops", D.CASES, ids=D.CASE_IDS)
def test_model_matches_recompute_of_kept_rows(case, n, drops):
    info = {}
    for g, dg in enumerate(D.data(n, seed=600 + n)):
        state = D.upload_state(dg["X"], dg["y"], dg["ell"])
        for m in drops:
            state, flags = D.drop_oldest(state, m, info)
            assert flags == [1] * ((m + 15) // 16), (case, g, m)
            assert state[1].shape == (state[0].shape[0],) * 2 and np.array_equal(state[1], np.tril(state[1]))
        assert state[0].shape[0] == n - sum(drops)
        assert np.array_equal(state[0], dg["X"][sum(drops):])
        _judge(case, g, state, dg, slice(sum(drops), n))
    print(f"[gp-drop model] {case}: cond(G_T) <= {info['condG']:.3g}")
    assert info["condG"] <= 1e6


@extended
def test_model_inert_rows_stay_exact_zeros():
    """36 live rows with two inert blocks of 6 (rows 20..25 and 35..40 of 48); dropping 28 rows takes
    the first inert block (in the second 16-row block of the drop) and keeps the second one."""
    for g, dg in enumerate(D.data(36, seed=700)):
        state = D.with_inert(D.with_inert(D.upload_state(dg["X"], dg["y"], dg["ell"]), 20, 6), 35, 6)
        state, flags = D.drop_oldest(state, 28)
        assert flags == [1, 1]
        X, M, alpha = state
        inert = np.arange(7, 13)
        assert M.shape == (20, 20) and np.array_equal(M, np.tril(M))
        assert not X[inert].any() and not alpha[inert].any() and not M[inert].any() and not M[:, inert].any()
        live = np.r_[np.arange(0, 7), np.arange(13, 20)]
        assert (np.diag(M)[live] > 0).all() and alpha[live].all()
        _judge("inert rows", g, state, dg, slice(22, 36))


@extended
def test_model_sliding_window():
    """Capacity 64 filled, then six rounds of drop 16 / append 16: no original row is left."""
    for g, dg in enumerate(D.data(64 + 96, seed=800)):
        state = D.upload_state(dg["X"][:64], dg["y"][:64], dg["ell"])
        for r in range(6):
            state, flags = D.drop_oldest(state, 16)
            assert flags == [1]
            lo = 64 + 16 * r
            state = D.append_block(state, dg["X"][lo:lo + 16], dg["y"][lo:lo + 16], dg["ell"])
        assert np.array_equal(state[0], dg["X"][96:160])
        _judge("sliding window", g, state, dg, slice(96, 160))


@extended
def test_zz_model_ratio_is_the_recorded_one():
    """The worst model ratio over the tests above is the R_MODEL that fixes MARGIN_DROP."""
    if len(RATIOS) < 3 * 2 * (len(D.CASES) + 2):   # (run on its own: nothing to report)
        return
    for q in ("mean", "var", "grad"):
        k = max((k for k in RATIOS if k[2] == q), key=lambda k: RATIOS[k])
        print(f"[gp-drop model] worst {q}: {RATIOS[k]:.3f} ({k[0]}, gp{k[1]})")
    worst = max(RATIOS.values())
    bulk = max(v for k, v in RATIOS.items() if k[0] != "one row left")
    print(f"[gp-drop model] worst ratio overall: {worst:.3f}; R_MODEL {D.R_MODEL}, MARGIN_DROP {D.MARGIN_DROP}")
    print(f"[gp-drop model] worst ratio with two rows or more kept: {bulk:.3f}; R_BULK {D.R_BULK}, "
          f"MARGIN_BULK {D.MARGIN_BULK}")
    assert D.MARGIN_DROP == np.ceil(4 * D.R_MODEL) and D.MARGIN_BULK == np.ceil(4 * D.R_BULK)
    # (the BLAS's summation order moves the figures a little between machines)
    assert worst <= 2 * D.R_MODEL and bulk <= 2 * D.R_BULK


# ------------------------------------------------------------------------------- Python mirrors
def _gp(X, y, g):
    from gpmpc.gp import GaussianProcess

    gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
    gp.set_hyperparameters(g["ell"], g["sf2"], g["sn2"])
    return gp


@pytest.mark.parametrize("d,n,drops", [(1, 29, (5, 16)), (3, 40, (1, 7, 12))])
def test_layout_after_drop_equals_layout_of_sliced_data(d, n, drops):
    g = R.synthetic_gp(n, d, seed=9 + d)
    y = np.sin(g["X"].sum(1)) + 0.3
    gp = _gp(g["X"], y, g)
    assert gp.device_layout("cpu")["n"] == n   # cached: drop_oldest must drop it
    for m in drops:
        out = gp.drop_oldest(m)
        assert out is gp and gp.K is None and gp.K_inv is None and gp._dev is None
    k = sum(drops)
    assert gp.train_inputs[0].shape == (n - k, d) and gp.train_targets.shape == (n - k,) and gp.n_ind_points == n - k
    lay, want = gp.device_layout("cpu"), _gp(g["X"][k:], y[k:], g).device_layout("cpu")
    assert lay["n"] == want["n"] == n - k and lay["npad"] == want["npad"] and lay["d"] == d
    for key in ("rows", "linvT", "alpha", "Linv"):
        assert torch.equal(lay[key], want[key]), key
    for bad in (0, -1, n - k, n):   # at least one row is dropped and at least one stays
        with pytest.raises(ValueError):
            gp.drop_oldest(bad)
    assert gp.n_ind_points == n - k


class _Handle:
    """Stands in for BatchSolver: the row bookkeeping of gp_size / append_gp / drop_gp, calls recorded."""

    def __init__(self, n, cap, n_gp):
        self.n, self.cap, self.calls = [n] * n_gp, cap, []

    def gp_size(self, g):
        return self.n[g], self.cap

    def append_gp(self, g, X, y):
        self.calls.append(("append", g, X.shape[0]))
        self.n[g] += X.shape[0]
        return torch.ones((X.shape[0] + 15) // 16, dtype=torch.int32)

    def drop_gp(self, g, m):
        self.calls.append(("drop", g, m))
        self.n[g] -= m
        return torch.ones((m + 15) // 16, dtype=torch.int32)


def _controller(n, cap):
    from gpmpc.gpmpc import GPMPC
    from gpmpc.models import get_spec

    spec = get_spec("quad2d")
    ctrl = object.__new__(GPMPC)   # (the constructor opens a solver handle on the GPU)
    ctrl.model, ctrl.sparse, ctrl.device, ctrl._requires_recompile = spec, False, "cpu", False
    ctrl.gp_idx = GPMPC._gp_columns(spec)
    ctrl.solver = _Handle(n, cap, spec.n_gp)
    rng = np.random.default_rng(3)
    ctrl.gaussian_process = [_gp(rng.uniform(-1, 1, (n, d)), rng.uniform(0.5, 1.5, n), dict(ell=1.0, sf2=1.0, sn2=1e-3))
                             for d in spec.gp_dims]
    return ctrl, spec


def test_append_data_past_capacity_raises_unless_evicting():
    from gpmpc import _lib

    ctrl, spec = _controller(20, 24)
    cols = sum(spec.gp_dims)
    rng = np.random.default_rng(4)
    new = lambda m: (rng.uniform(-1, 1, (m, cols)), rng.uniform(0.5, 1.5, (m, spec.n_gp)))   # noqa: E731
    first = [gp.train_inputs[0].clone() for gp in ctrl.gaussian_process]
    for kw in ({}, {"evict_oldest": False}):
        with pytest.raises(_lib.GPMPCError, match="capacity exceeded"):
            ctrl.append_data(*new(5), **kw)
        assert ctrl.solver.calls == [] and all(gp.n_ind_points == 20 for gp in ctrl.gaussian_process)
    # room for 4: no eviction needed
    ctrl.append_data(*new(4), evict_oldest=True)
    assert ctrl.solver.calls == [("append", 0, 4), ("append", 1, 4)]
    # full: 7 new rows evict exactly 7
    ctrl.solver.calls.clear()
    inputs, targets = new(7)
    ctrl.append_data(inputs, targets, evict_oldest=True)
    assert ctrl.solver.calls == [("drop", 0, 7), ("drop", 1, 7), ("append", 0, 7), ("append", 1, 7)]
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(24, 24)] * 2
    for g, gp in enumerate(ctrl.gaussian_process):
        assert gp.n_ind_points == 24 and gp.train_targets.shape == (24,)
        assert torch.equal(gp.train_inputs[0][:13], first[g][7:])
        assert torch.equal(gp.train_inputs[0][-7:], torch.tensor(inputs[:, ctrl.gp_idx[g]]))
        assert torch.equal(gp.train_targets[-7:], torch.tensor(targets[:, g]))
    # more rows than the capacity holds is an error either way
    ctrl.solver.calls.clear()
    with pytest.raises(_lib.GPMPCError, match="capacity exceeded"):
        ctrl.append_data(*new(25), evict_oldest=True)
    assert ctrl.solver.calls == []
    # drop_oldest on its own keeps the Python GPs in step
    ctrl.drop_oldest(3)
    assert ctrl.solver.calls == [("drop", 0, 3), ("drop", 1, 3)]
    assert all(gp.n_ind_points == 21 for gp in ctrl.gaussian_process)
    ctrl.sparse = True
    with pytest.raises(_lib.GPMPCError, match="sparse"):
        ctrl.drop_oldest(1)


# ------------------------------------------------------------------------------------- C ABI
def test_signature_table_lists_drop_oldest_with_the_header_types():
    from gpmpc import _lib

    text = HEADER.read_text()
    m = re.search(r"gpmpc_status\s+gpmpc_gp_drop_oldest\(([^)]*)\)\s*;", text)
    assert m, "gpmpc_gp_drop_oldest is not declared in the header"
    args = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["gpmpc_handle*", "int32_t", "int32_t", "int32_t*", "void*"]
    res, table = _lib.SIGNATURES["gpmpc_gp_drop_oldest"]
    assert res is ctypes.c_int32
    assert table == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]


def test_null_handle_is_refused_without_a_device():
    from gpmpc import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load(require_gpu=False)
    st = lib.gpmpc_gp_drop_oldest(None, 0, 1, None, None)
    assert st == -1   # GPMPC_ERR_ARG
    assert b"null handle" in lib.gpmpc_last_error()
