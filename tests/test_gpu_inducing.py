"""gpmpc_gp_inducing on the MI355X: up to M of a GP's n training rows picked greedily as FITC inducing rows.

quad2d handle with H = 5, GPs of 24, 40 and 272 training rows (a ragged row block, a full one, more than 16 row
blocks and more than 32 picks; at 0.4 of GP 1's lengthscale also more than 256 picks), the outputscales not 1.  The picks and the count must equal the longdouble
reference's (tests/gp_inducing_ref.py; the CPU test asserts that every gap to the runner-up and both distances
from tol at the stop are 1000 times what rounding can move), the residuals must lie within MARGIN_INDUCING of the
error of a float64 Cholesky of k(S, S) on the same picks.  Every output is pre-filled and followed by sentinels
(gp_update_util.guarded).  The call takes no stream and writes its outputs on a stream of the handle's own, so the
helpers synchronise after staging them, except where the ordering is the thing under test."""

import ctypes

import numpy as np
import pytest

import gp_drop_ref as D
import gp_fitc_ref as F
import gp_inducing_ref as I
import gp_ref as R
import gp_select_ref as S
import gp_update_util as U
from gp_append_ref import worst_ratio

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

OWNER = "inducing"


def _hyps(data):
    return [(dg["ell"], sf2, D.SN2) for dg, sf2 in zip(data, I.SF2)]


def _solver(n, rows=None, key="A", extra=16):
    """Handle `key` with the first `rows` (default n) rows of the n-row case data uploaded, room for `extra` more."""
    s = U.solver(OWNER, key, H=5)
    data = S.case_data(n)
    rows = n if rows is None else rows
    U.upload(s, data, slice(0, rows), capacity=rows + extra, hyps=_hyps(data))
    return s, data


def _stage(M, n):
    torch = U.gpu_torch()
    return dict(M=M, n=n, idx=U.guarded(M, torch.int32), gain=U.guarded(M), resid=U.guarded(n), count=ctypes.c_int32(-5))


def _call(s, g, tol, b, gains=True, resid=True, count=True):
    return s.lib.gpmpc_gp_inducing(s._h, g, b["M"], tol, b["idx"].data_ptr(), b["gain"].data_ptr() if gains else None,
                                   b["resid"].data_ptr() if resid else None, ctypes.byref(b["count"]) if count else None)


def _read(b, gains=True, resid=True, count=True):
    """picks (count,), gains (count,), resid (n,), count: the tails written, nothing past the ends."""
    M, n = b["M"], b["n"]
    idx, gn, rs = b["idx"].cpu().numpy(), b["gain"].cpu().numpy(), b["resid"].cpu().numpy()
    assert (idx[M:] == -99).all() and (gn[M:] == U.SENTINEL).all() and (rs[n:] == U.SENTINEL).all(), "wrote past an end"
    c = b["count"].value if count else int((idx[:M] >= 0).sum())
    assert 0 <= c <= M and (idx[:c] >= 0).all() and (idx[:c] < n).all() and (idx[c:M] == -1).all(), (c, idx[:M])
    assert len(set(idx[:c].tolist())) == c
    if gains:
        assert np.isfinite(gn[:c]).all() and np.isnan(gn[c:M]).all()
    else:
        assert np.isnan(gn[:M]).all()
    assert not np.isnan(rs[:n]).any() if resid else np.isnan(rs[:n]).all()
    return dict(picks=idx[:c].copy(), gains=gn[:c].copy(), resid=rs[:n].copy(), count=c)


def _inducing(s, g, M, tol, n, **kw):
    from gpmpc import _lib

    torch = U.gpu_torch()
    b = _stage(M, n)
    torch.cuda.synchronize()   # (the outputs are idle when the call is made)
    _lib.check(_call(s, g, tol, b, **kw))
    return _read(b, **kw)      # (no synchronise: the call returns with its work completed)


def _judge(tag, out, ref, e_full, sf2, live=None):
    want = ref["resid"].astype(np.float64)
    e = float(np.abs(out["resid"] - want).max())
    e_pick = float(np.abs(out["resid"][out["picks"]]).max())
    e_gain = float(np.abs(out["gains"] - ref["gains"]).max())
    print(f"[inducing] {tag}: count {out['count']} e {e:.3e} e_full {e_full:.3e} ratio {e / e_full:.3f} "
          f"picked rows {e_pick:.3e} gains {e_gain:.3e}")
    assert out["picks"].tolist() == ref["picks"].tolist() and out["count"] == ref["count"], tag
    assert out["gains"][0] == 1.0 and (np.diff(out["gains"]) <= 0).all(), tag
    assert e_gain <= I.allowed_score_error(sf2, e_full), tag
    assert e <= I.MARGIN_INDUCING * e_full, (tag, e, e_full)
    assert e_pick <= I.MARGIN_INDUCING * e_full, (tag, e_pick, e_full)
    if live is not None:
        assert (out["resid"][~live] == 0).all() and live[out["picks"]].all(), tag


@pytest.mark.parametrize("n", I.NS)
def test_picks_count_and_residuals_against_the_reference(n):
    s, _ = _solver(n)
    for g in range(2):
        sf2 = I.SF2[g]
        out = _inducing(s, g, n, I.TOL, n)
        _judge(f"n {n} gp{g} tol {I.TOL:g}", out, I.case_ref(n, g, n, I.TOL), I.case_e_full(n, g, n, I.TOL), sf2)
        assert (out["gains"] > I.TOL).all() and out["resid"].max() <= I.TOL * sf2
        for m in I.ms_tol0(g, n):
            out = _inducing(s, g, m, 0.0, n)
            assert out["count"] == m
            _judge(f"n {n} gp{g} m {m} tol 0", out, I.case_ref(n, g, m, 0.0), I.case_e_full(n, g, m, 0.0), sf2)


def test_more_picks_than_one_chunk_of_the_pivot_row():
    """264 picks: steps 257 .. 263 stage the pivot row in two chunks of 256 columns."""
    n, g, M, tol, scale = I.DEEP
    s = U.solver(OWNER, "A", H=5)
    data = S.case_data(n)
    hyps = [(dg["ell"] * (scale if k == g else 1.0), sf2, D.SN2) for k, (dg, sf2) in enumerate(zip(data, I.SF2))]
    U.upload(s, data, slice(0, n), capacity=n, hyps=hyps)
    out = _inducing(s, g, M, tol, n)
    assert out["count"] == M
    _judge("deep", out, I.case_ref(*I.DEEP), I.case_e_full(*I.DEEP), I.SF2[g])


def test_reproducible_prefixes_and_optional_outputs():
    n = 40
    s, data = _solver(n)
    for g in range(2):
        out = _inducing(s, g, n, I.TOL, n)
        again = _inducing(s, g, n, I.TOL, n)
        for k in ("picks", "gains", "resid"):
            assert out[k].tobytes() == again[k].tobytes(), (g, k)
        # the first k picks and gains of a call with M are those of a call with M = k
        for k in (1, 5, out["count"]):
            short = _inducing(s, g, k, I.TOL, n)
            assert short["count"] == k and short["picks"].tolist() == out["picks"][:k].tolist()
            assert short["gains"].tobytes() == out["gains"][:k].tobytes()
        bare = _inducing(s, g, n, I.TOL, n, gains=False, resid=False, count=False)
        assert bare["picks"].tolist() == out["picks"].tolist()
        # a LOVE root and a FITC mean are no obstacle and change nothing; the wrapper returns the same
        rank, ok = s.love_root_gp(g, rank=8)
        assert ok == 1 and s.fitc_gp(g, out["picks"], data[g]["y"][:n], 0.0) == 1
        try:
            under = _inducing(s, g, n, I.TOL, n)
            idx, gn, rs = s.inducing_gp(g, n, I.TOL, gains=True, resid=True)
            only = s.inducing_gp(g, n, I.TOL)
        finally:
            s.drop_love_root(g)
            s.drop_fitc(g)
        for k in ("picks", "gains", "resid"):
            assert out[k].tobytes() == under[k].tobytes(), (g, k)
        torch = U.gpu_torch()
        assert idx.dtype == torch.int32 and idx.cpu().numpy().tolist() == out["picks"].tolist() == only.cpu().numpy().tolist()
        assert gn.cpu().numpy().tobytes() == out["gains"].tobytes() and rs.cpu().numpy().tobytes() == out["resid"].tobytes()


@pytest.mark.parametrize("behind", (False, True))
def test_inert_rows_are_never_picked(behind):
    s, data = _solver(40, rows=I.INERT_N, extra=I.INERT_BLOCK + I.INERT_NEW)
    for g, dg in enumerate(data):
        X, live, new = I.inert_case(g, behind)
        U.nan_block(s, g, dg["d"], I.INERT_BLOCK, seed=7 + g)
        if behind:
            assert s.append_gp(g, *new).cpu().tolist() == [1]
        n = len(X)
        assert s.gp_size(g)[0] == n
        ref = I.greedy_ld(X, dg["ell"], I.SF2[g], int(live.sum()), I.TOL, live)
        out = _inducing(s, g, int(live.sum()), I.TOL, n)
        _judge(f"inert gp{g} behind {behind}", out, ref, I.e_full(X, dg["ell"], I.SF2[g], ref, live), I.SF2[g], live)
        if behind:
            assert (out["picks"] >= I.INERT_N + I.INERT_BLOCK).any()


def test_clustered_rows_give_a_fitc_mean_without_jitter():
    data = I.clustered()
    n = len(data[0]["X"])
    s = U.solver(OWNER, "A", H=5)
    s.set_gps(U.gp_objects(data, slice(None), hyps=[(dg["ell"], dg["sf2"], dg["sn2"]) for dg in data]))
    for g, dg in enumerate(data):
        s.reserve_gp(g, n)
        ref = I.greedy_ld(dg["X"], dg["ell"], dg["sf2"], n, I.TOL)
        out = _inducing(s, g, n, I.TOL, n)
        _judge(f"clustered gp{g}", out, ref, I.e_full(dg["X"], dg["ell"], dg["sf2"], ref), dg["sf2"])
        assert len({I.cluster_of(j) for j in out["picks"]}) == out["count"]
        assert s.fitc_gp(g, out["picks"], dg["y"], 0.0) == 1 and s.fitc_size(g) == out["count"]
        got = U.outputs(s, g, dg["Z"], f"clustered gp{g}")
        want = F.reference(dg["X"], dg["y"], out["picks"], dg["ell"], dg["Z"], dg["sf2"], dg["sn2"], 0.0)
        full = F.numpy64(dg["X"], dg["y"], out["picks"], dg["ell"], dg["Z"], dg["sf2"], dg["sn2"], 0.0)
        for q in ("mean", "tmean", "grad"):
            e_got, e_full, ratio = worst_ratio(got[q], full[U.REFKEY[q]], want[U.REFKEY[q]])
            print(f"[inducing] clustered gp{g} FITC {q}: e {e_got:.3e} e_full {e_full:.3e} ratio {ratio:.4f} (bound {F.MARGIN_FITC:g})")
            assert ratio <= F.MARGIN_FITC, (g, q, ratio)
        s.drop_fitc(g)


def test_the_call_waits_for_the_handles_last_call_on_another_stream():
    """A delay and a gpmpc_gp_refactor of GP 0 at a scaled lengthscale on stream A, then the call: when it returns
    the delay has ended, and its picks are those of the serial run behind the refactorisation."""
    from gpmpc import _lib
    from stream_order_util import DELAY_FLOOR_MS, Delay

    torch = U.gpu_torch()
    n, g = 40, 0
    s, data = _solver(n)
    ell = data[g]["ell"] * I.ELL_SCALE
    y = torch.tensor(data[g]["y"][:n], device="cuda")
    ok = torch.full((1,), -77, dtype=torch.int32, device="cuda")

    def refactor(stream):
        _lib.check(s.lib.gpmpc_gp_refactor(s._h, g, y.data_ptr(), ell, I.SF2[g], D.SN2, ok.data_ptr(), stream))

    before = _inducing(s, g, n, I.TOL, n)
    refactor(s._stream())
    torch.cuda.synchronize()
    serial = _inducing(s, g, n, I.TOL, n)
    assert ok.cpu().tolist() == [1]
    assert serial["picks"].tolist() == I.case_ref(n, g, n, I.TOL, I.ELL_SCALE)["picks"].tolist() != before["picks"].tolist()
    # the same on two streams: everything staged, then the delay, the writer and the call with no synchronise between
    s, data = _solver(n)
    A, delay, b = torch.cuda.Stream(), Delay(torch), _stage(n, n)
    torch.cuda.synchronize()
    delay.queue(A, DELAY_FLOOR_MS)
    end = torch.cuda.Event()
    end.record(A)
    refactor(A.cuda_stream)
    pending = not end.query()
    status = _call(s, g, I.TOL, b)
    done = end.query()
    torch.cuda.synchronize()
    _lib.check(status)
    assert pending, "the delay had ended before the call was made: it showed nothing"
    assert done, "the call returned while the delay ahead of the refactorisation still ran: it did not wait"
    out = _read(b)
    for k in ("picks", "gains", "resid"):
        assert out[k].tobytes() == serial[k].tobytes(), k


def test_refusals():
    torch = U.gpu_torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    n = 40
    s, data = _solver(n)
    b = _stage(n + 1, n + 1)
    torch.cuda.synchronize()

    def call(h, g=1, M=8, tol=I.TOL, idx=True):
        return s.lib.gpmpc_gp_inducing(h, g, M, tol, b["idx"].data_ptr() if idx else None, b["gain"].data_ptr(),
                                       b["resid"].data_ptr(), ctypes.byref(b["count"]))

    for kw, cause in ((dict(M=0), b"M must be 1 .. n"), (dict(M=-3), b"M must be"), (dict(M=n + 1), b"M must be 1 .. n"),
                      (dict(tol=-1e-9), b"tol"), (dict(tol=float("nan")), b"tol"), (dict(tol=float("inf")), b"tol"),
                      (dict(idx=False), b"idx_dev"), (dict(g=2), b"gp_id")):
        assert call(s._h, **kw) == -1 and cause in s.lib.gpmpc_last_error(), kw
    fresh = BatchSolver(get_spec("quad2d"), 5, 2)
    assert call(fresh._h) == -3 and b"GP not set" in s.lib.gpmpc_last_error()
    fresh.set_gps(U.gp_objects(data, slice(0, n)), with_variance=False)
    assert call(fresh._h) == -3 and b"Linv" in s.lib.gpmpc_last_error()
    fdata, fidx = F.case_data(40, 16)
    (Sx, w), ok = F.fitc(fdata[1]["X"], fdata[1]["y"], fidx, fdata[1]["ell"], jitter=F.JITTER)
    fresh.set_gps(U.gp_objects(fdata, slice(0, 40)), fitc=[None, (Sx, w)])
    assert call(fresh._h) == -3 and b"FITC upload" in s.lib.gpmpc_last_error()
    fresh.set_gps(U.gp_objects(data, slice(0, n)))   # no gpmpc_gp_reserve since gpmpc_set_gp
    assert call(fresh._h) == -3 and b"gpmpc_gp_reserve first" in s.lib.gpmpc_last_error()
    torch.cuda.synchronize()
    assert (b["idx"].cpu().numpy()[:n + 1] == -77).all() and b["count"].value == -5
    assert np.isnan(b["gain"].cpu().numpy()[:n + 1]).all() and np.isnan(b["resid"].cpu().numpy()[:n + 1]).all()
    # and the same call goes through once the GP is reserved
    fresh.reserve_gp(1, n)
    assert call(fresh._h) == 0 and b["count"].value == 8


def test_controller_picks_its_inducing_rows_greedily():
    torch = U.gpu_torch()
    from gpmpc.gpmpc import GPMPC
    from gpmpc.synthetic import initial_states
    from helpers import problem, product_gps

    B = 16
    spec, data, hyp = problem("quad2d", 48)
    first = [(X[:40], y[:40]) for X, y in data]
    inputs = np.hstack([X[40:] for X, _ in data])
    targets = np.column_stack([y[40:] for _, y in data])
    kw = dict(horizon=10, batch=B, sparse_gp=True, gp_capacity=64, max_gp_samples=30, variance="exact", fitc="device")
    ctrl = GPMPC("quad2d", fitc_select="greedy", **kw)
    ctrl.set_gaussian_processes(product_gps(first, hyp))
    ctrl.reset()
    s = ctrl.solver

    def check(n):
        assert s.gp_size(0) == (n, 64) and isinstance(ctrl.fitc_idx, list) and len(ctrl.fitc_idx) == 2
        for g in range(2):
            want = s.inducing_gp(g, min(n, 30), ctrl.fitc_tol).cpu().numpy()
            assert 1 <= len(want) <= 30 and np.array_equal(ctrl.fitc_idx[g], want)
            assert s.fitc_sizes[g] == s.fitc_size(g) == len(want) and np.array_equal(s.fitc_mean(g)[0], want)

    check(40)
    x0, phase = initial_states(spec, ctrl.traj, B)
    obs = torch.tensor(x0, device="cuda")
    ts = torch.tensor(phase, dtype=torch.int32, device="cuda")
    ctrl.select_action_batch(obs, ts, check=True)
    flags = ctrl.append_data(inputs, targets)
    assert [f.cpu().tolist() for f in flags] == [[1], [1]]
    check(48)
    u = ctrl.select_action_batch(obs, ts, check=True)
    assert torch.isfinite(u).all() and np.isin(s.status.cpu().numpy(), (0, 2)).all()
    assert ctrl.np_random.bit_generator.state == np.random.default_rng(1337).bit_generator.state   # (nothing drawn)
    # the default draws what it drew before (16 rows and a jitter, as test_gpu_gp_fitc.py's controller)
    rnd = GPMPC("quad2d", fitc_jitter=1e-8, **dict(kw, max_gp_samples=16))
    rnd.set_gaussian_processes(product_gps(first, hyp))
    rnd.reset()
    assert rnd.fitc_select == "random"
    assert np.array_equal(rnd.fitc_idx, np.random.default_rng(1337).choice(range(40), size=16, replace=False))
    assert rnd.solver.fitc_sizes == [16, 16]
