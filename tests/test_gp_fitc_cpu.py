"""The device-built FITC mean: what needs no GPU.

* The float64 numpy model of the kernels (tests/gp_fitc_ref.py) against the np.longdouble evaluation of the
  reference's formula, over every case tests/test_gpu_gp_fitc.py judges: the reference alone goes through, the
  model's status is 1 and its worst error is at most MARGIN_FITC times that of the plain float64 solve form
  (the measured ratios are printed: run with -s).  Their maximum is recomputed and must not ask for a larger
  margin than the stored one.
* The model's status is 0 for a duplicate index at jitter 0, an index naming an inert row or equal to n and a
  NaN target of a live row; inert rows' targets are never read.
* The model on the reference-generated fixture (tests/golden/golden_quad3d.npz): GPs 1 and 2 at jitter 0
  within 1e-8 of the largest mean, GP 0 (cond(K_ss) 1.7e16) with jitter 1e-8 outputscale within 1e-3.
* ``GPMPC``'s host logic in device mode against a recording stand-in for the solver handle; the host mode's
  four refusals are unchanged.
* The ctypes signature table lists the two entry points with the header's types, and a null handle is
  refused without a device.
"""

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import gp_fitc_ref as F
import gp_ref as R
from gp_append_ref import worst_ratio

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmpc_mi355x.h"
extended = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")
RATIOS: dict = {}


def _judge(tag, g, dg, X, y, idx, jitter, **model_kw):
    """The model on (X, y, idx) of the case (with whatever inert rows model_kw adds) against the reference on
    the live rows: the ratios per quantity."""
    ref = F.reference(dg["X"], dg["y"], idx, dg["ell"], dg["Z"], jitter=jitter)   # (asserts its own pivots)
    full = F.numpy64(dg["X"], dg["y"], idx, dg["ell"], dg["Z"], jitter=jitter)
    (S, w), ok = F.fitc(X, y, idx, dg["ell"], jitter=jitter, **model_kw)
    assert ok, (tag, g)
    assert np.isfinite(w).all() and np.array_equal(S, dg["X"][idx])
    got = F.evaluate(S, w, dg["ell"], dg["Z"])
    for q in ("mean", "grad"):
        e_model, e_full, r = worst_ratio(got[q], full[q], ref[q])
        print(f"[gp-fitc model] {tag} gp{g} {q}: e_model {e_model:.3e} e_full {e_full:.3e} ratio {r:.4f}")
        RATIOS[(tag, g, q)] = r
        assert r <= F.MARGIN_FITC, (tag, g, q, r)


@extended
@pytest.mark.parametrize("case", F.CASES, ids=F.CASE_IDS)
def test_model_matches_the_reference(case):
    cid, n, cap, M, jitter, gps = case
    data, idx = F.case_data(n, M)
    assert len(set(idx.tolist())) == M and 0 <= idx.min() and idx.max() < n
    for g in gps:
        _judge(cid, g, data[g], data[g]["X"], data[g]["y"], idx, jitter)


@extended
def test_model_with_inert_rows():
    data, mask, idx, ys = F.inert_case()
    for g, dg in enumerate(data):
        X = np.vstack([dg["X"], np.zeros((5, dg["d"]))])
        _judge("inert rows", g, dg, X, ys[g], idx, F.JITTER, inert=mask)
        # the same weights, bit for bit, whatever the inert rows hold
        (_, w1), _ = F.fitc(X, ys[g], idx, dg["ell"], jitter=F.JITTER, inert=mask)
        X2, y2 = X.copy(), ys[g].copy()
        X2[40:], y2[40:] = 3.0, 7.0
        (_, w2), _ = F.fitc(X2, y2, idx, dg["ell"], jitter=F.JITTER, inert=mask)
        assert np.array_equal(w1, w2)


@extended
def test_zz_margin_is_the_recorded_one():
    """MARGIN_FITC = ceil(4 R_MODEL), and the ratio recomputed here asks for no larger one."""
    assert F.MARGIN_FITC == math.ceil(4 * F.R_MODEL)
    if not RATIOS:   # (run on its own: nothing to report)
        return
    k = max(RATIOS, key=RATIOS.get)
    print(f"[gp-fitc model] worst ratio {RATIOS[k]:.4f} ({k}); R_MODEL {F.R_MODEL}, MARGIN_FITC {F.MARGIN_FITC}")
    assert F.MARGIN_FITC >= math.ceil(4 * RATIOS[k]), (k, RATIOS[k], F.MARGIN_FITC)


def test_model_status_zero():
    data, idx = F.case_data(40, 16)
    dg = data[1]
    assert F.fitc(dg["X"], dg["y"], idx, dg["ell"], jitter=0.0)[1]
    # a duplicate at jitter 0: the second pivot is exactly 1 - 1 * 1 = 0 at sf2 = 1
    assert not F.fitc(dg["X"], dg["y"], np.full(4, 7), dg["ell"], jitter=0.0)[1]
    bad = idx.copy()
    bad[3] = 40
    assert not F.fitc(dg["X"], dg["y"], bad, dg["ell"], jitter=F.JITTER)[1]
    y = dg["y"].copy()
    y[int(idx[0]) ^ 1] = np.nan
    assert not F.fitc(dg["X"], y, idx, dg["ell"], jitter=F.JITTER)[1]
    data, mask, idx, ys = F.inert_case()
    X = np.vstack([data[1]["X"], np.zeros((5, 3))])
    bad = idx.copy()
    bad[0] = 42
    assert not F.fitc(X, ys[1], bad, data[1]["ell"], jitter=F.JITTER, inert=mask)[1]


# ------------------------------------------------------------------------------- the fixture
GP_IDX = [[0], [1, 2, 3], [4, 5, 6]]


def fixture_gp(g, i):
    """GP i of the fixture: (X, y, (ell, sf2, sn2), idx, Zq, kz @ fitc_w) with kz = k(Zq, S) carrying sf2."""
    import gp_drop_ref as D

    X, y = g["gp_Xtr"][:, GP_IDX[i]], g["gp_Ytr"][:, i]
    ell, sf2, sn2 = (float(v) for v in g["gp_hyp"][i])
    idx = np.asarray(g["fitc_idx"]).astype(np.int32)
    Zq = g["gp_Zq"][:, GP_IDX[i]]
    want = D.kernel64(X[idx], ell, sf2, Zq) @ g["fitc_w"][i]
    return X, y, (ell, sf2, sn2), idx, Zq, want


# (GP, jitter / outputscale, tolerance relative to the largest mean): the project's figures for this quantity
# (tests/test_cpu_host.py::test_fitc_weights_match_reference_fixture), taken norm-wise
FIXTURE = [(1, 0.0, 1e-8), (2, 0.0, 1e-8), (0, 1e-8, 1e-3)]


@pytest.mark.parametrize("i,jit,tol", FIXTURE, ids=["gp1", "gp2", "gp0-jitter"])
def test_model_on_the_reference_fixture(golden3d, i, jit, tol):
    X, y, (ell, sf2, sn2), idx, Zq, want = fixture_gp(golden3d, i)
    (S, w), ok = F.fitc(X, y, idx, ell, sf2, sn2, jitter=jit * sf2)
    assert ok
    got = F.evaluate(S, w, ell, Zq, sf2)["mean"]
    err = float(np.abs(got - want).max()) / float(np.abs(want).max())
    print(f"[gp-fitc model] fixture gp{i}: {err:.3e} of the largest mean")
    assert err <= tol, (i, err)


# ------------------------------------------------------------------------------- Python mirrors
class _Handle:
    """Stands in for BatchSolver: every call recorded in order."""

    def __init__(self, n, ok=1):
        self.n, self.ok, self.calls = n, ok, []
        self.fitc_sizes = [0, 0]
        self.love_ranks = [None, None]

    def gp_size(self, g):
        return self.n, 64

    def fitc_gp(self, g, idx, y, jitter=0.0):
        self.calls.append(("fitc", g, np.asarray(idx).copy(), y.clone(), jitter))
        if self.ok:
            self.fitc_sizes[g] = len(idx)
        return self.ok

    def drop_fitc(self, g):
        self.calls.append(("drop_fitc", g))
        self.fitc_sizes[g] = 0

    def append_gp(self, g, X, y):
        self.calls.append(("append", g, X.shape[0]))
        if g == 1:
            self.n += X.shape[0]
        return torch.ones(1, dtype=torch.int32)

    def drop_gp(self, g, m):
        self.calls.append(("drop", g, m))
        if g == 1:
            self.n -= m
        return torch.ones(1, dtype=torch.int32)

    def refactor_gp(self, g, y, ell, sf2, sn2):
        self.calls.append(("refactor", g))
        return torch.ones(1, dtype=torch.int32)


def _controller(n, fitc, seed=5, **kw):
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.models import get_spec

    spec = get_spec("quad2d")
    ctrl = object.__new__(GPMPC)   # (the constructor opens a solver handle on the GPU)
    ctrl.model, ctrl.sparse, ctrl.device, ctrl._requires_recompile = spec, True, "cpu", False
    if fitc is not None:
        ctrl.fitc = fitc
    ctrl.max_gp_samples = 8
    ctrl.np_random = np.random.default_rng(seed)
    ctrl.gp_idx = GPMPC._gp_columns(spec)
    ctrl.solver = _Handle(n, **kw)
    rng = np.random.default_rng(3)
    ctrl.gaussian_process = []
    for d in spec.gp_dims:
        X = rng.uniform(-1, 1, (n, d))
        gp = GaussianProcess(torch.tensor(X), torch.tensor(np.sin(3 * X.sum(1)) + 0.5))
        ctrl.gaussian_process.append(gp.set_hyperparameters(1.0 + 0.1 * d, 1.0, 1e-3))
    return ctrl


def test_class_defaults_are_the_host_mode():
    from gpmpc.gpmpc import GPMPC

    assert GPMPC.fitc == "host" and GPMPC.fitc_jitter == 0.0 and GPMPC.fitc_idx is None


def test_host_mode_refusals_are_unchanged():
    from gpmpc import _lib

    ctrl = _controller(20, None)   # (no fitc attribute set: the class default)
    X, y = np.zeros((2, 4)), np.zeros((2, 2))
    for name, call in (("append_data", lambda: ctrl.append_data(X, y)), ("drop_oldest", lambda: ctrl.drop_oldest(2)),
                       ("refresh_gps", ctrl.refresh_gps),
                       ("refit_hyperparameters", lambda: ctrl.refit_hyperparameters(0.01, 2))):
        with pytest.raises(_lib.GPMPCError, match=rf"^{name}: not available in sparse \(FITC\) mode$"):
            call()
    assert ctrl.solver.calls == []


def test_device_mode_drops_then_updates_then_rebuilds():
    ctrl = _controller(20, "device")
    ctrl.fitc_jitter = 1e-8
    ctrl.solver.fitc_sizes = [8, 8]
    rng = np.random.default_rng(11)
    flags = ctrl.append_data(rng.uniform(-1, 1, (6, 4)), rng.uniform(0, 1, (6, 2)))
    assert len(flags) == 2
    kinds = [c[0] for c in ctrl.solver.calls]
    assert kinds == ["drop_fitc", "drop_fitc", "append", "append", "fitc", "fitc"]
    # one draw for both GPs, from the controller's generator, over the rows after the update
    want = np.random.default_rng(5).choice(range(26), size=8, replace=False)
    for c, gp in zip(ctrl.solver.calls[4:], ctrl.gaussian_process):
        assert np.array_equal(c[2], want) and c[4] == 1e-8
        assert torch.equal(c[3], gp.train_targets) and c[3].shape[0] == 26
    assert np.array_equal(ctrl.fitc_idx, want)
    ctrl.solver.calls.clear()
    ctrl.drop_oldest(4)
    assert [c[0] for c in ctrl.solver.calls] == ["drop_fitc", "drop_fitc", "drop", "drop", "fitc", "fitc"]
    assert ctrl.fitc_idx.max() < 22 and len(ctrl.fitc_idx) == 8
    ctrl.solver.calls.clear()
    ctrl.refresh_gps()
    assert [c[0] for c in ctrl.solver.calls] == ["drop_fitc", "drop_fitc", "refactor", "refactor", "fitc", "fitc"]
    ctrl.solver.calls.clear()
    ctrl.refit_hyperparameters(0.05, 2)
    assert [c[0] for c in ctrl.solver.calls] == ["drop_fitc", "drop_fitc", "refactor", "refactor", "fitc", "fitc"]


def test_device_mode_uses_every_row_when_there_are_few():
    ctrl = _controller(5, "device")
    ctrl.refresh_gps()
    assert sorted(ctrl.fitc_idx.tolist()) == [0, 1, 2, 3, 4]
    assert [c[0] for c in ctrl.solver.calls] == ["refactor", "refactor", "fitc", "fitc"]   # (nothing installed: no drop)


def test_a_reported_zero_raises():
    from gpmpc import _lib

    ctrl = _controller(20, "device", ok=0)
    with pytest.raises(_lib.GPMPCError, match=r"GP 0: the FITC mean could not be built.*exact mean; try fitc_jitter > 0"):
        ctrl.refresh_gps()
    ctrl.fitc_jitter = 1e-8
    with pytest.raises(_lib.GPMPCError, match=r"GP 0: .*the GP is on the exact mean$"):
        ctrl.refresh_gps()


def test_constructor_rejects_device_fitc_without_sparse_before_anything_else():
    from gpmpc.gpmpc import GPMPC

    with pytest.raises(ValueError, match="sparse_gp=True"):
        GPMPC("quad2d", fitc="device", device="cpu")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        GPMPC("quad2d", sparse_gp=True, fitc="gpu", device="cpu")


# ------------------------------------------------------------------------------------- C ABI
def _decl(name):
    m = re.search(rf"gpmpc_status\s+{name}\(([^)]*)\)\s*;", HEADER.read_text())
    assert m, f"{name} is not declared in the header"
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_signature_table_lists_the_entry_points_with_the_header_types():
    from gpmpc import _lib

    P, I, Dd = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    assert _decl("gpmpc_gp_fitc") == ["gpmpc_handle*", "int32_t", "int32_t", "const int32_t*", "const double*", "double",
                                      "int32_t*", "void*"]
    res, table = _lib.SIGNATURES["gpmpc_gp_fitc"]
    assert res is I and table == [P, I, I, P, P, Dd, ctypes.POINTER(I), P]
    assert _decl("gpmpc_get_gp_fitc") == ["gpmpc_handle*", "int32_t", "int32_t*", "int32_t*", "double*", "void*"]
    res, table = _lib.SIGNATURES["gpmpc_get_gp_fitc"]
    assert res is I and table == [P, I, ctypes.POINTER(I), P, P, P]
    assert "gp_fitc.hip" in _lib.HASHED
    mk = (ROOT / "gp-mpc_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    hashed = re.search(r"^HASHED = (.*)$", mk, re.M).group(1).split()
    assert srcs[-1] == "gp_fitc.hip" and hashed == _lib.HASHED


def test_null_handle_is_refused_without_a_device():
    from gpmpc import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load(require_gpu=False)
    for st in (lib.gpmpc_gp_fitc(None, 0, 1, None, None, 0.0, None, None),
               lib.gpmpc_get_gp_fitc(None, 0, None, None, None, None)):
        assert st == -1   # GPMPC_ERR_ARG
        assert b"null handle" in lib.gpmpc_last_error()
