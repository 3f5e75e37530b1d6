"""The cases of tests/test_gpu_var_trim.py, built without a GPU: every reference variance is at
least sf2 / 2 (so sqrt(var) of the tightening stays real and the bound tol_var is far below the
effect of a dropped or doubled product), the cases reach every quad count at both of its ends, and
the trimmed products are zeros of the operand the handle is given."""

import numpy as np
import pytest

import gp_ref as R
import var_trim_cases as C

pytestmark = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")


def _check_state(case, what):
    xs, us, gps = case
    assert xs.shape == (C.B, C.H + 1, C.spec().nx) and us.shape == (C.B, C.H, C.spec().nu)
    for g, c in enumerate(gps):
        n = c["gp"]["n"]
        assert c["var"].shape == (C.B * C.H,) and c["Linv"].shape == (n, n), (what, g)
        assert c["var"].min() >= 0.5 * C.SF2, (what, g, c["var"].min())
        assert (c["tol"] < 1e-9 * C.SF2).all(), (what, g, c["tol"].max())   # the bound is below the mutual tolerance
        assert not np.triu(c["Linv"], 1).any(), (what, g)                    # L^-1 lower triangular: L^-T upper


@pytest.mark.parametrize("nt,r", C.HANDLE_CASES)
def test_handle_case_reference(nt, r):
    _check_state(C.handle_case(nt, r), f"NT={nt} r={r}")


@pytest.mark.parametrize("n0,n1", C.MIXED_CASES)
def test_mixed_case_reference(n0, n1):
    _check_state(C.mixed_case(n0, n1), f"mixed {n0},{n1}")


@pytest.mark.parametrize("n", C.FREE_NS)
def test_free_case_reference(n):
    c = C.free_case(n)
    assert c["npad"] == 208 and c["var"].min() >= 0.5 * c["gp"]["sf2"], (n, c["var"].min())
    assert not c["linvT"][n:].any() and not c["linvT"][:, n:].any() and not np.tril(c["linvT"], -1).any()


def test_append_case_reference():
    xs, us, data, refs = C.append_case()
    assert len(refs) == len(C.APPEND_BLOCKS)
    for per_gp in refs:
        for v in per_gp:
            assert v.shape == (C.B * C.H,) and v.min() >= 0.5 * C.APPEND_SN2


def test_cases_reach_every_quad_count_at_both_ends():
    got = {(nt, C.quads(16 * (nt - 1) + r)) for nt, r in C.HANDLE_CASES}
    assert got == {(nt, q) for nt in C.NTS for q in (0, 1, 2)}
    assert [C.quads(16 * 12 + r) for r in C.RS] == [1, 1, 2, 2, 0, 0]
    assert {16 * 12 + r for r in C.RS} >= {196, 200}
    assert [tuple(C.quads(n) for n in ns) for ns in C.MIXED_CASES] == [(1, 2), (2, 0)]
    sizes = np.cumsum((C.APPEND_N0,) + C.APPEND_BLOCKS).tolist()
    assert sizes == [196, 200, 204, 205, 213] and [C.quads(n) for n in sizes] == [1, 2, 0, 0, 2]
    assert C.APPEND_CAP >= sizes[-1]
