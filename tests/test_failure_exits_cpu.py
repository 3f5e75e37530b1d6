"""The failure script (tests/failure_cases.py) on the C++ restatement alone: the verdicts below are
conditions on the script's INPUTS, which tests/test_gpu_failure_exits.py then holds every compiled
variant of the SQP kernel to.

Failing solve, per shape: A is refused before the SQP loop (4, no iteration); B+ and B- end their
first QP as a QP failure (4, sqp_iter 0) at an IPM iteration that the IPM limit does not reach -- the
same one with qp_max_iter 50 and 200 (but B+ of cartpole H = 32, refused at iteration 53); C and D -- a
NaN in the stored iterate -- are GPMPC_NAN (1) at the first residual test, whichever variable holds it.
Case E is cartpole H = 32 pushed against the cart position's bounds, where the refusal lies between the
two limits and 50 ends every QP at the limit (status 2, 5 SQP iterations, 250 IPM iterations).
A failed instance keeps its iterate (NaN included), its multipliers are zeroed, it has no previous
solution, u0 is the kept first input; the next solve recovers A and B+-, C and D stay failed until the
iterate is set, and then solve.

The residual norms are maxima, and a maximum drops a NaN operand: before the finiteness flag beside
them, C and D reached the QP (status 4), and a NaN in a converged iterate that still had its
multipliers was reported as status 0 with a NaN first input (test_nan_beside_converged_multipliers).
"""

import numpy as np
import pytest

import failure_cases as fc

pytestmark = pytest.mark.skipif(not fc.cpu_ref_built(), reason="oracle/lib/libcpuref.so not built (make -C oracle)")

# IPM iteration at which the first QP of B+ / B- is refused.  The quadrotors' position cases: the ranges
# the issue measured (here 35, 37, 38 and 37, 40, 41).  The cartpole's cases are other inputs (the pole
# angle, failure_cases.py), so those ranges do not apply to them: measured 31 and 32 at H = 4, 53 and 49
# at H = 32, and held to 30 .. 60 -- one IPM iteration below the smallest count that any refusal took in
# the grid of profiles/r23/README.md, and far below the IPM limit of 200 that the case must not reach
QP_RANGE = {fc.BP: (35, 45), fc.BM: (34, 42)}
QP_RANGE_CARTPOLE = (30, 60)
FAILED = (fc.A, fc.BP, fc.BM, fc.C, fc.D)
ids = [fc.shape_id(s) for s in fc.SHAPES]


def verdict(o, b):
    return int(o["status"][b]), int(o["sqp_iter"][b]), int(o["qp_iter"][b])


def assert_kept(o, b, at):
    """Instance b of a failed solve's outputs: iterate kept bit for bit, multipliers zero, no previous solution."""
    xb, ub = o["before"]
    np.testing.assert_array_equal(o["x"][b], xb[b], err_msg=str(at))
    np.testing.assert_array_equal(o["u"][b], ub[b], err_msg=str(at))
    np.testing.assert_array_equal(o["u0"][b], ub[b, 0], err_msg=str(at))
    assert not o["pi"][b].any() and not o["ll"][b].any() and not o["lu"][b].any(), at
    assert o["has_prev"][b] == 0, at


@pytest.mark.parametrize("shape", fc.SHAPES, ids=ids)
@pytest.mark.parametrize("plant", fc.PLANTS)
def test_verdicts(shape, plant):
    out = fc.planted_run(shape, plant)
    clean = fc.clean_run(shape)[0]
    for s in (0, 1):
        assert (out[s]["status"] == 0).all(), (s, out[s]["status"])
    f = out[fc.FAILING]
    assert verdict(f, fc.A) == (4, 0, 0)
    for b in (fc.BP, fc.BM):
        st, it, qp = verdict(f, b)
        lo, hi = QP_RANGE_CARTPOLE if shape[0] == "cartpole" else QP_RANGE[b]
        print(f"{fc.shape_id(shape)} {'B+' if b == fc.BP else 'B-'}: status {st}, sqp_iter {it}, IPM stops at {qp}")
        assert (st, it) == (4, 0) and lo <= qp <= hi, (b, st, it, qp)
    assert verdict(f, fc.C) == (1, 0, 0)
    assert verdict(f, fc.D) == (1, 0, 0)
    assert np.isnan(f["before"][1][fc.C]).sum() == 1
    assert np.isnan(f["before"][0][fc.D]).sum() + np.isnan(f["before"][1][fc.D]).sum() == 1
    for b in FAILED:
        assert_kept(f, b, (plant, b))
    n = out[fc.NEXT]
    assert [int(n["status"][b]) for b in FAILED] == [0, 0, 0, 1, 1], n["status"]
    for b in (fc.C, fc.D):          # the iterate stays non-finite until it is set
        assert verdict(n, b) == (1, 0, 0)
        np.testing.assert_array_equal(n["x"][b], f["x"][b])
        np.testing.assert_array_equal(n["u"][b], f["u"][b])
    h = out[fc.HEALED]
    assert (h["status"] == 0).all(), h["status"]
    assert np.isfinite(h["x"]).all() and np.isfinite(h["u"]).all() and np.isfinite(h["u0"]).all()
    # instances are independent: the clean ones are the clean run's, bit for bit, at every solve
    for s in range(5):
        for k in ("u0", "status", "sqp_iter", "qp_iter", "x", "u"):
            np.testing.assert_array_equal(out[s][k][list(fc.CLEAN)], clean[s][k][list(fc.CLEAN)], err_msg=f"solve {s}: {k}")


@pytest.mark.parametrize("shape", fc.SHAPES, ids=ids)
def test_ipm_limit_is_out_of_reach(shape):
    """B+-: qp_max_iter 50 and 200 give the same status at the same IPM iteration (cartpole H = 32, where
    the horizon slows the IPM's divergence: B- the same, B+ is refused at iteration 53 of 200, and 50 is
    therefore not compared)."""
    f200, f50 = fc.planted_run(shape)[fc.FAILING], fc.planted_run(shape, "u0", fc.OPTS_50)[fc.FAILING]
    for b in (fc.BP, fc.BM):
        if shape == fc.CASE_E_SHAPE and b == fc.BP:
            assert verdict(f200, b)[:2] == (4, 0) and 50 < verdict(f200, b)[2] <= QP_RANGE_CARTPOLE[1], verdict(f200, b)
        else:
            assert verdict(f200, b) == verdict(f50, b), (b, verdict(f200, b), verdict(f50, b))


def test_case_e_every_qp_ends_at_the_ipm_limit():
    """cartpole H = 32 pushed against the cart position's bounds: the IPM of the infeasible QP is refused
    only between the two limits (measured: 125 and 115), so qp_max_iter 50 never reports a QP failure."""
    for opts, want in ((fc.Options(b_state=0), None), (fc.Options(qp_max_iter=50, b_state=0), (2, 25, 25 * 50))):
        f = fc.planted_run(fc.CASE_E_SHAPE, "u0", opts)[fc.FAILING]
        for b in (fc.BP, fc.BM):
            st, it, qp = verdict(f, b)
            assert ((st, it) == (4, 0) and 50 < qp < 200) if want is None else (st, it, qp) == want, (b, st, it, qp)
    out = fc.planted_run(fc.CASE_E_SHAPE, "u0", fc.OPTS_E)
    f = out[fc.FAILING]
    for b in (fc.BP, fc.BM):
        assert verdict(f, b) == (2, 5, 250)
        assert f["has_prev"][b] == 1 and np.isfinite(f["x"][b]).all() and np.isfinite(f["u"][b]).all()
    assert (out[fc.HEALED]["status"] == 0).all(), out[fc.HEALED]["status"]


@pytest.mark.parametrize("shape", fc.SHAPES, ids=ids)
@pytest.mark.parametrize("tighten", (True, False), ids=("tightened", "untightened"))
@pytest.mark.parametrize("plant", fc.PLANTS)
def test_nan_beside_converged_multipliers(shape, tighten, plant):
    """A converged solve repeated at the same observation and reference index, with one NaN written
    into the stored iterate and the multipliers left as the solve stored them (acados memory edited in
    place; gpmpc_set_iterate would zero them): every finite residual term is below the tolerance, so
    norms that drop the NaN report status 0, sqp_iter 0 and a NaN first input.  It is GPMPC_NAN."""
    _, obs, phase = fc.clean_run(shape, fc.OPTS, tighten)
    be = fc.CpuBackend(shape, fc.OPTS, tighten)
    for _ in range(8):     # (the tightening follows the stored solution, so the first repeats still move)
        o = be.solve(obs[0], phase)
        if (o["sqp_iter"] == 0).all():
            break
    assert (o["status"] == 0).all() and (o["sqp_iter"] == 0).all()      # converged: a repeat takes no step
    x, u = fc.plant_nan(o["x"], o["u"], plant)
    be.ref.x[fc.D], be.ref.u[fc.D] = x[fc.D], u[fc.D]
    o = be.solve(obs[0], phase)
    assert verdict(o, fc.D) == (1, 0, 0), verdict(o, fc.D)
    np.testing.assert_array_equal(o["x"][fc.D], x[fc.D])
    np.testing.assert_array_equal(o["u"][fc.D], u[fc.D])
    assert (np.delete(o["status"], fc.D) == 0).all()


def test_inf_in_the_iterate_is_nan_status_too():
    """An Inf in x_2 makes a residual Inf, not NaN; it is a non-finite iterate all the same (status 1
    at the residual test, before it: the QP's failure, 4)."""
    shape = fc.SHAPES[0]
    _, obs, phase = fc.clean_run(shape)
    be = fc.CpuBackend(shape)
    o = be.solve(obs[0], phase)
    x, u = o["x"].copy(), o["u"].copy()
    x[fc.D, 2, 0] = np.inf
    be.set_iterate(x, u)
    o = be.solve(obs[1], phase + 1)
    assert verdict(o, fc.D) == (1, 0, 0)
    assert (np.delete(o["status"], fc.D) == 0).all()
