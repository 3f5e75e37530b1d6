"""Greedy choice of the FITC inducing rows (gpmpc_gp_inducing): what needs no GPU.

* The header declares the entry point with the issue's parameter list and no stream parameter, the ctypes table
  matches, and a null handle is refused without a device.
* The longdouble reference (tests/gp_inducing_ref.py) against itself: its residuals equal the direct formula
  sf2 - k(x_i, S) K_ss^-1 k(S, x_i), the Cholesky diagonal of K_ss in pick order is sqrt(gain sf2), and the first k
  picks of a run with M are those of a run with M = k.
* The float64 model of the kernel's summation order meets the criterion in every case, with the reference's
  picks; the worst ratio is recomputed and must not ask for a larger margin than the stored one (run with -s).
* The gap condition: at every step of every case the GPU test judges (the inert-row cases and the clustered rows
  included) the gap to the runner-up, and at the stop the distance of the last accepted gain and of the first
  refused score from tol, is at least GAP_FACTOR times the score error the criterion allows.
* The clustered rows: the picks come from at least six of the eight clusters for GP 1, every gain is above tol, the
  largest residual is below the last gain, and gp_fitc_ref's model of the FITC build at those picks with jitter 0
  goes through and meets test_gpu_gp_fitc.py's criterion.
* The same for the case that takes more picks than one chunk of the kernel's staged pivot row (264 > 256).
* The ordering test's lengthscale factor changes the reference's picks.
* ``GPMPC``'s arguments: "greedy" needs the device build.
"""

import ctypes
import functools
import math
import re
from pathlib import Path

import numpy as np
import pytest

import gp_fitc_ref as F
import gp_inducing_ref as I
import gp_ref as R
from gp_append_ref import worst_ratio

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmpc_mi355x.h"
extended = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")
RATIOS: dict = {}


def _decl(name):
    m = re.search(rf"gpmpc_status\s+{name}\(([^)]*)\)\s*;", HEADER.read_text())
    assert m, f"{name} is not declared in the header"
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).replace("\n", " ").split(",")], m.group(1)


def test_the_header_and_the_signature_table_agree():
    from gpmpc import _lib

    P, Ii, Dd = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    types, text = _decl("gpmpc_gp_inducing")
    assert types == ["gpmpc_handle*", "int32_t", "int32_t", "double", "int32_t*", "double*", "double*", "int32_t*"]
    assert [a.strip().split()[-1].lstrip("*") for a in text.replace("\n", " ").split(",")] == \
        ["h", "gp_id", "M", "tol", "idx_dev", "gain_dev", "resid_dev", "count_out"]
    assert "stream" not in text
    res, table = _lib.SIGNATURES["gpmpc_gp_inducing"]
    assert res is Ii and table == [P, Ii, Ii, Dd, P, P, P, ctypes.POINTER(Ii)]


def test_null_handle_is_refused_without_a_device():
    from gpmpc import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load(require_gpu=False)
    assert lib.gpmpc_gp_inducing(None, 0, 1, 0.0, None, None, None, None) == -1   # GPMPC_ERR_ARG
    assert b"null handle" in lib.gpmpc_last_error()


@extended
@pytest.mark.parametrize("n", I.NS)
def test_reference_residuals_pivots_and_prefixes(n):
    for g in range(2):
        gp = I.gp_of(n, g)
        ref = I.case_ref(n, g, n, I.TOL)
        direct, diag = I.direct_ld(gp["X"], gp["ell"], gp["sf2"], ref["picks"])
        assert float(np.abs(direct - ref["resid"]).max()) <= 1e-15 * gp["sf2"], (n, g)
        want = np.sqrt(ref["gains"].astype(I.LD) * I.LD(gp["sf2"]))
        assert float(np.abs(diag - want).max()) <= 1e-15 * math.sqrt(gp["sf2"]), (n, g)
        assert (ref["gains"] > I.TOL).all() and ref["gains"][0] == 1.0 and ref["picks"][0] == 0
        assert (np.diff(ref["gains"]) <= 0).all()
        assert float(ref["resid"].max()) / gp["sf2"] <= I.TOL or ref["count"] == n
        for M in I.ms_tol0(g, n):
            short = I.case_ref(n, g, M, 0.0)
            assert short["count"] == M
            k = min(M, ref["count"])
            assert short["picks"][:k].tolist() == ref["picks"][:k].tolist()
            assert np.array_equal(short["gains"][:k], ref["gains"][:k])


def test_counts_of_the_cases():
    counts = {n: tuple(I.case_ref(n, g, n, I.TOL)["count"] for g in range(2)) for n in I.NS}
    assert counts == {24: (6, 23), 40: (6, 33), 272: (6, 51)}, counts


@functools.lru_cache(maxsize=None)
def _model(case):
    n, g, M, tol = case
    gp = I.gp_of(n, g)
    return I.greedy_f64(gp["X"], gp["ell"], gp["sf2"], M, tol)


def _gap_condition(tag, sf2, ref, e):
    allowed = I.allowed_score_error(sf2, e)
    gaps = ref["gaps"][np.isfinite(ref["gaps"])]
    smallest = float(gaps.min()) if len(gaps) else np.inf
    print(f"[inducing gap] {tag}: count {ref['count']} e_full {e:.3e} allowed {allowed:.3e} smallest gap {smallest:.3e} "
          f"stop margins {ref['accepted']:.3e} / {ref['refused']:.3e}")
    assert np.isinf(ref["gaps"][0])   # (step 0: an exact tie, the index decides)
    assert smallest >= I.GAP_FACTOR * allowed, (tag, smallest, allowed)
    assert min(ref["accepted"], ref["refused"]) >= I.GAP_FACTOR * allowed, (tag, ref["accepted"], ref["refused"])


@extended
@pytest.mark.parametrize("case", I.CASES, ids=[f"n{n}-gp{g}-M{M}-tol{tol:g}" for n, g, M, tol in I.CASES])
def test_the_model_meets_the_criterion_and_the_gaps_hold(case):
    n, g, M, tol = case
    gp = I.gp_of(n, g)
    ref = I.case_ref(n, g, M, tol)
    e = I.case_e_full(n, g, M, tol)
    model = _model(case)
    assert model["picks"].tolist() == ref["picks"].tolist() and model["count"] == ref["count"]
    e_model = float(np.abs(model["resid"] - ref["resid"]).max())
    RATIOS[case] = e_model / e
    print(f"[inducing model] n {n} gp{g} M {M} tol {tol:g}: e_model {e_model:.3e} e_full {e:.3e} ratio {RATIOS[case]:.3f}")
    assert e_model <= I.MARGIN_INDUCING * e
    assert np.abs(model["gains"] - ref["gains"]).max() <= I.allowed_score_error(gp["sf2"], e)
    _gap_condition(f"n {n} gp{g} M {M} tol {tol:g}", gp["sf2"], ref, e)


@extended
def test_the_case_past_256_picks():
    n, g, M, tol, scale = I.DEEP
    gp = I.gp_of(n, g, scale)
    ref, e = I.case_ref(*I.DEEP), I.case_e_full(*I.DEEP)
    assert ref["count"] == M > 256
    model = I.greedy_f64(gp["X"], gp["ell"], gp["sf2"], M, tol)
    assert model["picks"].tolist() == ref["picks"].tolist()
    e_model = float(np.abs(model["resid"] - ref["resid"]).max())
    RATIOS[I.DEEP] = e_model / e
    print(f"[inducing model] deep: e_model {e_model:.3e} e_full {e:.3e} ratio {RATIOS[I.DEEP]:.3f}")
    assert e_model <= I.MARGIN_INDUCING * e
    _gap_condition("deep", gp["sf2"], ref, e)


@extended
def test_the_stored_margin_covers_the_measured_ratio():
    for case in I.CASES:   # (whatever the parametrised test above has not run in this process)
        if case not in RATIOS:
            n, g, M, tol = case
            RATIOS[case] = float(np.abs(_model(case)["resid"] - I.case_ref(n, g, M, tol)["resid"]).max()) / I.case_e_full(n, g, M, tol)
    worst = max(RATIOS.values())
    print(f"[inducing model] R_MODEL measured {worst:.3f}, stored {I.R_MODEL}")
    assert math.ceil(4 * worst) <= I.MARGIN_INDUCING == math.ceil(4 * I.R_MODEL)


@extended
@pytest.mark.parametrize("behind", (False, True))
def test_inert_rows_in_the_reference(behind):
    for g in range(2):
        X, live, _ = I.inert_case(g, behind)
        gp = I.gp_of(40, g)
        ref = I.greedy_ld(X, gp["ell"], gp["sf2"], int(live.sum()), I.TOL, live)
        assert live[ref["picks"]].all() and (ref["resid"][~live] == 0).all()
        # the live rows alone give the same picks, at their own indices
        alone = I.greedy_ld(X[live], gp["ell"], gp["sf2"], int(live.sum()), I.TOL)
        assert np.flatnonzero(live)[alone["picks"]].tolist() == ref["picks"].tolist()
        if behind:
            assert (ref["picks"] >= I.INERT_N + I.INERT_BLOCK).any()
        _gap_condition(f"inert gp{g} behind {behind}", gp["sf2"], ref, I.e_full(X, gp["ell"], gp["sf2"], ref, live))


@extended
def test_clustered_rows_through_the_references():
    for g, dg in enumerate(I.clustered()):
        n = len(dg["X"])
        ref = I.greedy_ld(dg["X"], dg["ell"], dg["sf2"], n, I.TOL)
        clusters = {I.cluster_of(j) for j in ref["picks"]}
        print(f"[inducing clustered] gp{g}: {ref['count']} picks from clusters {sorted(clusters)}, gains {ref['gains']}, "
              f"largest residual {float(ref['resid'].max()) / dg['sf2']:.3e} outputscales")
        assert len(clusters) == ref["count"]   # (never two rows of one cluster)
        if g == 1:
            assert len(clusters) >= 6
        assert (ref["gains"] > I.TOL).all()
        assert float(ref["resid"].max()) / dg["sf2"] < ref["gains"][-1]
        _gap_condition(f"clustered gp{g}", dg["sf2"], ref, I.e_full(dg["X"], dg["ell"], dg["sf2"], ref))
        # the FITC build at these picks with jitter 0: the reference goes through (it asserts its own pivots), and
        # the float64 model of the device build meets test_gpu_gp_fitc.py's criterion
        args = (dg["X"], dg["y"], ref["picks"], dg["ell"])
        want = F.reference(*args, dg["Z"], dg["sf2"], dg["sn2"], 0.0)
        full = F.numpy64(*args, dg["Z"], dg["sf2"], dg["sn2"], 0.0)
        (Sx, w), ok = F.fitc(*args, dg["sf2"], dg["sn2"], jitter=0.0)
        assert ok
        got = F.evaluate(Sx, w, dg["ell"], dg["Z"], dg["sf2"])
        for q in ("mean", "grad"):
            e_model, e_full, r = worst_ratio(got[q], full[q], want[q])
            print(f"[inducing clustered] gp{g} FITC {q}: e_model {e_model:.3e} e_full {e_full:.3e} ratio {r:.4f}")
            assert r <= F.MARGIN_FITC, (g, q, r)


@extended
def test_the_ordering_tests_lengthscale_changes_the_picks():
    n = 40
    a, b = I.case_ref(n, 0, n, I.TOL), I.case_ref(n, 0, n, I.TOL, I.ELL_SCALE)
    assert a["picks"].tolist() != b["picks"].tolist()
    gp = I.gp_of(n, 0, I.ELL_SCALE)
    _gap_condition("scaled lengthscale", gp["sf2"], b, I.e_full(gp["X"], gp["ell"], gp["sf2"], b))


def test_greedy_build_asks_the_handle_per_gp_and_draws_nothing():
    import torch

    from gpmpc.gpmpc import GPMPC
    from test_gp_fitc_cpu import _controller

    assert GPMPC.fitc_select == "random" and GPMPC.fitc_tol == 1e-4
    ctrl = _controller(20, "device")
    ctrl.fitc_select, ctrl.fitc_tol, ctrl.fitc_jitter = "greedy", 1e-3, 0.0
    picks = [np.array([0, 7, 3], dtype=np.int32), np.array([0, 11, 5, 2, 9], dtype=np.int32)]

    def inducing_gp(g, M, tol):
        ctrl.solver.calls.append(("inducing", g, M, tol))
        return torch.tensor(picks[g])

    ctrl.solver.inducing_gp = inducing_gp
    state = ctrl.np_random.bit_generator.state
    ctrl._build_fitc()
    calls = ctrl.solver.calls
    assert [c[:2] for c in calls] == [("inducing", 0), ("inducing", 1), ("fitc", 0), ("fitc", 1)]
    assert [c[2:] for c in calls[:2]] == [(8, 1e-3), (8, 1e-3)]   # (min(n, max_gp_samples), fitc_tol)
    for g in range(2):
        assert np.array_equal(calls[2 + g][2], picks[g]) and calls[2 + g][4] == 0.0
        assert np.array_equal(ctrl.fitc_idx[g], picks[g])
    assert ctrl.solver.fitc_sizes == [3, 5]
    assert ctrl.np_random.bit_generator.state == state   # (np_random is not consumed)


def test_greedy_needs_the_device_build():
    from gpmpc.gpmpc import GPMPC

    for kw in (dict(), dict(sparse_gp=True), dict(sparse_gp=True, fitc="host")):
        with pytest.raises(ValueError, match="fitc_select='greedy'"):
            GPMPC("quad2d", horizon=5, device="cpu", fitc_select="greedy", **kw)
    with pytest.raises(ValueError, match="'random' or 'greedy'"):
        GPMPC("quad2d", horizon=5, device="cpu", sparse_gp=True, fitc="device", fitc_select="best")
