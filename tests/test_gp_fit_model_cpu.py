"""The float64 numpy model of gpmpc_gp_mll (tests/gp_fit_ref.py) on the CPU: against the fit oracle at the
tolerances the torch product is held to (test_gp_fit_oracle.check_product_against_oracle), on live
subsets with inert rows and at the tile edge sizes; and the margin of the GPU test (R_MODEL) recomputed.
Run with -s for the figures."""

import math

import numpy as np
import pytest

import gp_fit_ref as FR
import gp_ref as R
from oracle import gp_fit_oracle as F
from test_gp_fit_oracle import CASES, RAWS, case_data

needs_ld = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")


def oracle_constrained(X, y, raw):
    """The oracle's MLL / n and its gradient with respect to (lengthscale, outputscale, noise)."""
    val, g = F.mll_grad(X, y, raw)
    return val, g / np.array([F.sigmoid(r) for r in raw])


def check(got, want, what):
    val, g = got
    wv, wg = want
    assert abs(val - wv) < 1e-11 * max(1.0, abs(wv)), (what, val, wv)
    np.testing.assert_allclose(g, wg, rtol=1e-9, atol=1e-12 * (1 + np.abs(wg).max()), err_msg=str(what))


@pytest.mark.parametrize("name,i,n", CASES)
def test_model_matches_the_oracle(name, i, n):
    X, y = case_data(name, i, n)
    for raw in RAWS:
        check(FR.tile_model(X, y, *F.constrained(raw)), oracle_constrained(X, y, raw), (name, i, raw))


@pytest.mark.parametrize("n", [5, 16, 17, 33])
def test_model_matches_the_oracle_at_the_tile_edges(n):
    for name, i, _ in CASES:
        X, y = case_data(name, i, 40)
        for raw in RAWS:
            check(FR.tile_model(X[:n], y[:n], *F.constrained(raw)), oracle_constrained(X[:n], y[:n], raw), (name, i, n, raw))


@pytest.mark.parametrize("name,i,n", CASES)
def test_inert_rows_are_not_counted(name, i, n):
    """Inert rows (stored input the origin, NaN target) among the live ones: the oracle on the live subset."""
    X, y = case_data(name, i, n)
    X = np.asarray(X, dtype=np.float64).reshape(n, -1)
    mask = np.zeros(n + 11, dtype=bool)
    mask[20:26] = True
    mask[n + 6:] = True
    Xa, ya = np.zeros((n + 11, X.shape[1])), np.full(n + 11, np.nan)
    Xa[~mask], ya[~mask] = X, y
    for raw in RAWS:
        check(FR.tile_model(Xa, ya, *F.constrained(raw), inert=mask), oracle_constrained(X, y, raw), (name, i, raw))


@needs_ld
def test_oracle_and_model_against_the_longdouble_recompute():
    """How much of rtol 1e-9 the float64 oracle itself uses (the issue's 1.3e-11), and the model."""
    worst_o = worst_m = 0.0
    for name, i, n in CASES:
        X, y = case_data(name, i, n)
        for raw in RAWS:
            hyp = F.constrained(raw)
            ref = FR.reference_ld(X, y, *hyp)
            refv = np.r_[ref[0], ref[1]]
            o, m = oracle_constrained(X, y, raw), FR.tile_model(X, y, *hyp)
            eo = float((FR.errors(*o, ref) / np.maximum(np.abs(refv), 1e-300)).max())
            em = float((FR.errors(*m, ref) / np.maximum(np.abs(refv), 1e-300)).max())
            print(f"[gp-fit] {name} gp{i} raw {raw}: oracle rel {eo:.2e}, model rel {em:.2e}")
            worst_o, worst_m = max(worst_o, eo), max(worst_m, em)
    print(f"[gp-fit] worst relative error: oracle {worst_o:.2e}, model {worst_m:.2e}")
    assert worst_o < 1e-10 and worst_m < 1e-10


@needs_ld
def test_margin_covers_the_model():
    worst = (0.0, None)
    for n, _ in FR.EDGE:
        for g, dg in enumerate(FR.edge_data(n)):
            yv, yg, hyp = FR.yardstick(dg["X"], dg["y"], dg["ell"], FR.SF2, FR.SN2)
            ref = FR.reference_ld(dg["X"], dg["y"], *hyp)
            e, ey, r = FR.ratios(*FR.tile_model(dg["X"], dg["y"], *hyp), (yv, yg), ref)
            up = FR.upload_state(dg["X"], dg["y"], dg["ell"], FR.SF2, FR.SN2)   # (not judged: the upload's own error)
            ru = FR.ratios(*FR.tile_model(dg["X"], dg["y"], *hyp, state=up), (yv, yg), ref)[2]
            print(f"[gp-fit] {n} rows gp{g} on an upload's state: ratios " + " ".join(f"{v:.2f}" for v in ru))
            for k, q in enumerate(FR.QUANT):
                print(f"[gp-fit] {n} rows gp{g} {q}: ref {np.r_[ref[0], ref[1]][k]:.6e} e_model {e[k]:.3e} "
                      f"e_yard {ey[k]:.3e} ratio {r[k]:.3f}")
                if r[k] > worst[0]:
                    worst = (float(r[k]), (n, g, q))
    print(f"[gp-fit] R_MODEL measured {worst[0]:.3f} at {worst[1]} (stored {FR.R_MODEL}, MARGIN_FIT {FR.MARGIN_FIT})")
    assert worst[0] <= FR.R_MODEL
    assert FR.MARGIN_FIT == math.ceil(4 * FR.R_MODEL)
