"""The triangular variance kernel with its ragged last column tile on four-column quads
(gp_var_tri_kernel<NT, FROM_STATE, NQ>, GPMPC_TUNE_VAR_TRIM; csrc/gp_kernels.hip), MI355X only.

Cases, operands and references come from tests/var_trim_cases.py (tests/gp_ref.py underneath); the
CPU test tests/test_var_trim_cpu.py builds all of them and makes the reference-only assertions.
Every case asserts that its reference variance is >= sf2 / 2 before any GPU call (the append case:
>= sn2 / 2, the guard of the fitted-GP reference it shares with tests/test_gpu_gp_append.py, whose
factor comes from the data and cannot be scaled), pre-fills its outputs with NaN and keeps 64
sentinels past their end.

Handle-based cases force var_split = 1, so the launch is gp_var_tri_kernel<NT, true, NQ>, and run
the same iterate at var_trim = 1 and var_trim = 0.  Both are checked against the reference within
its worst-case bound tol_var; their mutual difference is checked at 1e-9 sf2, the tolerance of
test_tightening_variance_matches_oracle for this kernel.  The largest |trim - full| / sf2 is
printed per case (run with -s).  Measured on MI355X: 1.1e-16 sf2 at most over all cases (one unit
in the last place of the variance; 0 to 16 of a case's 70 values differ, none where NQ = 0), and
both runs stay below 1e-3 of tol_var.  Appended against fresh: error ratios 0.66 .. 1.04.
"""

import numpy as np
import pytest

import gp_ref as R
import var_trim_cases as C
from gp_append_ref import MARGIN, worst_ratio
from helpers import initial_states, lqr

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

GUARD = 64
SENTINEL = -7.25e77
MUTUAL = 1e-9          # x sf2
_SOLVERS: dict = {}
WORST = [0.0]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _guarded(P):
    torch = _torch()
    t = torch.full((P + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    t[P:] = SENTINEL
    return t


def _read(t, P, what):
    a = t.cpu().numpy()
    assert (a[P:] == SENTINEL).all(), f"{what}: wrote past the end of the output"
    assert not np.isnan(a[:P]).any(), f"{what}: {int(np.isnan(a[:P]).sum())} of {P} outputs not written"
    return a[:P].copy()


def _within(got, want, tol, what):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    ratio = float((np.abs(got - want) / tol).max())
    print(f"[var-trim] {what:52s} max(err/tol) = {ratio:.3e}")
    assert ratio <= 1.0, (what, ratio)


def _mutual(trim, full, sf2, what):
    d = float(np.abs(trim - full).max() / sf2)
    WORST[0] = max(WORST[0], d)
    print(f"[var-trim] {what:52s} max|trim - full| / sf2 = {d:.3e}, {int((trim != full).sum())} of {trim.size} "
          f"values differ   (worst so far {WORST[0]:.3e})")
    assert d <= MUTUAL, (what, d)


def _solver(key):
    """One quad2d BatchSolver (H = 7, B = 5, tightening on) per key, shared by the cases."""
    _torch()
    from gpmpc.solver import BatchSolver

    if key not in _SOLVERS:
        s = BatchSolver(C.spec(), C.H, C.B)
        s.set_tightening(True, 0.95, *lqr(C.spec()))
        _SOLVERS[key] = s
    return _SOLVERS[key]


def _state_variance(s, xs, us, what):
    """solve, set_iterate(xs, us), solve, gpmpc_get_variance into a guarded buffer -> (B H, n_gp)."""
    torch = _torch()
    from gpmpc import _lib

    _lib.check(s.lib.gpmpc_use_gp(s._h, 1))
    Bn, Hn, ngp = s.batch, s.H, s.spec.n_gp
    x0, ph = initial_states(s.spec, s.spec.reference_trajectory(), Bn)
    obs = torch.tensor(x0, device="cuda")
    ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
    s.reset(reset_iterate=True)
    s.solve(obs, ts)                                    # marks a previous solution
    s.set_iterate(torch.tensor(xs, device="cuda"), torch.tensor(us, device="cuda"))
    s.solve(obs, ts)                                    # variance launch at (xs, us)
    v = _guarded(Bn * Hn * ngp)
    _lib.check(s.lib.gpmpc_get_variance(s._h, Bn, v.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return _read(v, Bn * Hn * ngp, what).reshape(Bn * Hn, ngp)


def _trim_and_full(s, xs, us, what):
    """The variance launch at (xs, us) with var_trim = 1 and 0, var_split = 1."""
    out = {}
    try:
        s.set_tuning(var_split=1)
        for trim in (1, 0):
            s.set_tuning(var_trim=trim)
            out[trim] = _state_variance(s, xs, us, f"{what} var_trim={trim}")
    finally:
        s.set_tuning(var_split=0, var_trim=1)
    return out[1], out[0]


def _run_state(case, what):
    from gpmpc import _lib

    xs, us, gps = case
    for g, c in enumerate(gps):
        assert c["var"].min() >= 0.5 * C.SF2, (what, g, c["var"].min())    # before any GPU call
    s = _solver("synthetic")
    for g, c in enumerate(gps):
        gp = c["gp"]
        alpha = np.zeros(gp["n"])                                          # the dynamics stay the prior's
        _lib.check(s.lib.gpmpc_set_gp(s._h, g, gp["n"], gp["d"], c["X"].ctypes.data, alpha.ctypes.data, 0, None,
                                      c["Linv"].ctypes.data, gp["ell"], gp["sf2"], gp["sn2"]))
    trim, full = _trim_and_full(s, xs, us, what)
    for g, c in enumerate(gps):
        _within(trim[:, g], c["var"] + C.SN2, c["tol"], f"{what} gp{g} n={c['gp']['n']} trim")
        _within(full[:, g], c["var"] + C.SN2, c["tol"], f"{what} gp{g} n={c['gp']['n']} full")
    _mutual(trim, full, C.SF2, what)


@pytest.mark.parametrize("nt,r", C.HANDLE_CASES)
def test_state_variance_trim_matches_full(nt, r):
    """Both GPs n = 16 (NT - 1) + r: NQ = 1 (r = 1, 4), NQ = 2 (r = 5, 8), the full tile (r = 9, 16)."""
    _run_state(C.handle_case(nt, r), f"NT={nt} r={r} NQ={C.quads(16 * (nt - 1) + r)}")


@pytest.mark.parametrize("n0,n1", C.MIXED_CASES)
def test_state_variance_mixed_quads(n0, n1):
    """The GPs of one launch disagree on NQ: 196 | 200 (1 and 2: the launch takes 2, exact for both)
    and 200 | 205 (2 and the full tile: the launch takes the full tile)."""
    _run_state(C.mixed_case(n0, n1), f"mixed n=({n0},{n1}) NQ=({C.quads(n0)},{C.quads(n1)})")


@pytest.mark.parametrize("n", C.FREE_NS)
def test_posterior_variance_only_trimmed(n):
    """gpmpc_gp_posterior, variance only, NT = 13, just enough points to turn the column split off
    (2 ceil(P / 128) > CUs): gp_var_tri_kernel<13, false, NQ>, NQ = 1 (n = 196) and 2 (n = 200).
    The P points cycle through 193 distinct ones with stride 7."""
    torch = _torch()
    from gpmpc import _lib

    c = C.free_case(n)
    gp = c["gp"]
    assert c["var"].min() >= 0.5 * gp["sf2"], (n, c["var"].min())          # before any GPU call
    ncu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    P = 128 * (ncu // 2) + 1
    assert 2 * ((P + 127) // 128) > ncu
    idx = (7 * np.arange(P)) % C.FREE_POINTS
    rows, linvT = torch.tensor(c["rows"], device="cuda"), torch.tensor(c["linvT"], device="cuda")
    Zt = torch.tensor(np.ascontiguousarray(c["Z"][idx]), device="cuda")
    v = _guarded(P)
    _lib.check(_lib.load().gpmpc_gp_posterior(gp["n"], gp["d"], c["npad"], _lib.ptr(rows), _lib.ptr(linvT), gp["ell"],
                                              gp["sf2"], gp["sn2"], _lib.ptr(Zt), P, None, _lib.ptr(v), 1,
                                              _lib.stream_ptr(Zt.device)))
    torch.cuda.synchronize()
    got = _read(v, P, f"free n={n}")
    _within(got, c["var"][idx] + gp["sn2"], c["tol"][idx], f"handle-free n={n} NQ={C.quads(n)} P={P}")
    # a point's variance does not depend on where it sits in its 16-point tile (193 is odd, so every
    # point comes round at every position): the overlapped halves of a step rely on it
    first = np.full(C.FREE_POINTS, np.nan)
    first[idx[:C.FREE_POINTS]] = got[:C.FREE_POINTS]
    assert {int(i) % 16 for i in np.nonzero(idx == 0)[0]} == set(range(16))
    assert np.array_equal(got, first[idx]), f"n={n}: {int((got != first[idx]).sum())} copies differ from their point's first"


def test_variance_after_append_crosses_quad_counts():
    """n = 196 uploaded with capacity 224, then appends of 4, 4, 1 and 8 rows: 200 (NQ 1 -> 2), 204,
    205 (the full tile), 213 (NT = 14, NQ = 2; the factor has moved to its second buffer).  After
    each, the appended handle's variance launch (var_trim = 1) against a fresh upload of the same
    rows run with var_trim = 0: worst error against the extended-precision refit at most 8 x the
    fresh upload's, the criterion of tests/test_gpu_gp_append.py for the appended factor."""
    torch = _torch()
    from gpmpc.gp import GaussianProcess

    xs, us, data, refs = C.append_case()                                   # (asserts var >= sn2 / 2)

    def gps(n):
        out = []
        for dg in data:
            gp = GaussianProcess(torch.tensor(dg["X"][:n]), torch.tensor(dg["y"][:n]))
            gp.set_hyperparameters(dg["ell"], C.APPEND_SF2, C.APPEND_SN2)
            out.append(gp)
        return out

    sa, sb = _solver("appended"), _solver("fresh")
    sa.set_gps(gps(C.APPEND_N0))
    for g in range(2):
        sa.reserve_gp(g, C.APPEND_CAP)
    at = C.APPEND_N0
    try:
        sa.set_tuning(var_split=1, var_trim=1)
        sb.set_tuning(var_split=1, var_trim=0)
        for step, m in enumerate(C.APPEND_BLOCKS):
            for g, dg in enumerate(data):
                Xb, yb = dg["X"][at:at + m].copy(), dg["y"][at:at + m].copy()      # (the case's arrays are read-only)
                assert sa.append_gp(g, Xb, yb).cpu().tolist() == [1], (at, m, g)
            at += m
            assert [sa.gp_size(g) for g in range(2)] == [(at, C.APPEND_CAP)] * 2
            app = _state_variance(sa, xs, us, f"appended n={at}")
            sb.set_gps(gps(at))
            full = _state_variance(sb, xs, us, f"fresh n={at}")
            for g in range(2):
                e_app, e_full, ratio = worst_ratio(app[:, g], full[:, g], refs[step][g])
                print(f"[var-trim] append n={at} NQ={C.quads(at)} gp{g}: e_app {e_app:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
                assert ratio <= MARGIN, (at, g, e_app, e_full)
    finally:
        sa.set_tuning(var_split=0, var_trim=1)
        sb.set_tuning(var_split=0, var_trim=1)
