"""gpmpc_gp_informative on the MI355X: the m of P points where the GPs are least certain.

quad2d handle with H = 5 and B = 130 (P = 130 is past two wavefronts and more than one workgroup of the score
and rank kernels), GPs of 24 and 40 training rows.  The scores must be bit-equal to
max_g gp_predict(g, inputs_g, with_noise=False).var / outputscale_g from the same handle, and the picks equal to
the numpy rank rule (tests/observe_ref.py) applied to the device's own scores.  Among the points are two duplicated
transitions (a tie: the lower index first) and one with a NaN (its score is NaN and it ranks last)."""

import numpy as np
import pytest

import gp_drop_ref as D
import gp_update_util as U
import observe_ref as OR

pytestmark = pytest.mark.gpu

OWNER = "informative"
BMAX = 130
DUP, NANROW = (3, 7), 5   # transition 7 repeats transition 3; transition 5 holds a NaN
SF2 = (2.5, 0.7)          # outputscales that are not 1, so the division shows


def _solver(n):
    s = U.solver(OWNER, "A", H=5, B=BMAX)
    data = D.data(n, seed=40 + n)
    U.upload(s, data, slice(0, n), capacity=n + 16, hyps=[(dg["ell"], sf2, D.SN2) for dg, sf2 in zip(data, SF2)])
    return s, data


def _points(s, P):
    """P transitions' (x, u) with the duplicate and the NaN (where P has room for them)."""
    x, u = OR.transitions(s.spec, P, seed=5)
    if P > max(DUP):
        x[DUP[1]], u[DUP[1]] = x[DUP[0]], u[DUP[0]]
        x[NANROW, 4] = np.nan
    return x, u


def _inputs(s, x, u):
    z = np.hstack([x, u])
    return np.hstack([z[:, list(idx)] for idx in s.spec.gp_inputs])


def _expected_scores(s, x, u):
    """max_g of gp_predict's noise-free variance over the outputscale, from the same P points in one call per GP
    (the launch gpmpc_gp_informative makes); NaN at a point with a non-finite input."""
    torch = U.gpu_torch()
    inputs = _inputs(s, x, u)
    var, col = [], 0
    for g, d in enumerate(s.spec.gp_dims):
        Z = torch.tensor(np.ascontiguousarray(inputs[:, col:col + d]), device="cuda")
        var.append(s.gp_predict(g, Z, with_noise=False, mean=False)[1].cpu().numpy())
        col += d
    return OR.score(np.array(var), SF2, inputs)


def _informative(s, x, u, m, scores=True):
    torch = U.gpu_torch()
    from gpmpc import _lib

    P = len(x)
    xt, ut = torch.tensor(x, device="cuda"), torch.tensor(u, device="cuda")
    pk, sc = U.guarded(m, torch.int32), U.guarded(P)
    _lib.check(s.lib.gpmpc_gp_informative(s._h, P, xt.data_ptr(), ut.data_ptr(), m, pk.data_ptr(),
                                          sc.data_ptr() if scores else None, s._stream()))
    torch.cuda.synchronize()
    pick = U.read(pk, m, "picks")
    a = sc.cpu().numpy()
    assert (a[P:] == U.SENTINEL).all(), "wrote past the end of the scores"
    return pick, a[:P].copy()


@pytest.mark.parametrize("n", [24, 40])
@pytest.mark.parametrize("P", [1, 40, 130])
def test_scores_are_gp_predict_and_picks_follow_the_rank_rule(n, P):
    s, _ = _solver(n)
    x, u = _points(s, P)
    want = _expected_scores(s, x, u)
    for m in sorted({1, min(17, P), P}):
        pick, score = _informative(s, x, u, m)
        np.testing.assert_array_equal(score, want)   # (bit for bit; NaN at the NaN point on both sides)
        assert pick.tolist() == OR.rank(score, m).tolist(), (n, P, m)
        assert ((pick >= 0) & (pick < P)).all() and len(set(pick.tolist())) == m
        if P > max(DUP):
            assert np.isnan(score[NANROW]) and np.isfinite(np.delete(score, NANROW)).all()
            assert score[DUP[0]] == score[DUP[1]]
            if m == P:
                assert pick[-1] == NANROW
                order = pick.tolist()
                assert order.index(DUP[0]) + 1 == order.index(DUP[1])   # the tie: neighbours, lower index first
    # without a score buffer, and through the wrapper
    pick, untouched = _informative(s, x, u, min(17, P), scores=False)
    assert np.isnan(untouched).all() and pick.tolist() == OR.rank(want, min(17, P)).tolist()
    torch = U.gpu_torch()
    pk, sc = s.informative(torch.tensor(x, device="cuda"), torch.tensor(u, device="cuda"), min(17, P), scores=True)
    assert pk.dtype == torch.int32 and pk.cpu().numpy().tolist() == pick.tolist()
    np.testing.assert_array_equal(sc.cpu().numpy(), want)


def test_a_love_root_leaves_the_scores_unchanged():
    s, _ = _solver(40)
    x, u = _points(s, 40)
    pick0, score0 = _informative(s, x, u, 40)
    for g in range(2):
        rank, ok = s.love_root_gp(g, rank=8)
        assert ok == 1 and rank >= 1
    try:
        pick1, score1 = _informative(s, x, u, 40)
    finally:
        for g in range(2):
            s.drop_love_root(g)
    np.testing.assert_array_equal(score1, score0)
    assert pick1.tolist() == pick0.tolist()


def test_refusals():
    torch = U.gpu_torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    s, _ = _solver(24)
    x, u = OR.transitions(s.spec, BMAX + 1, seed=5)
    xt, ut = torch.tensor(x, device="cuda"), torch.tensor(u, device="cuda")
    pk, sc = U.guarded(BMAX + 1, torch.int32), U.guarded(BMAX + 1)

    def call(h, P, m, xp=xt.data_ptr(), up=ut.data_ptr(), pp=pk.data_ptr()):
        return s.lib.gpmpc_gp_informative(h, P, xp, up, m, pp, sc.data_ptr(), s._stream())

    for P, m in ((0, 1), (BMAX + 1, 1), (40, 0), (40, 41)):
        assert call(s._h, P, m) == -1, (P, m)
    assert call(s._h, 40, 8, xp=None) == -1 and call(s._h, 40, 8, up=None) == -1 and call(s._h, 40, 8, pp=None) == -1
    fresh = BatchSolver(get_spec("quad2d"), 5, 40)
    assert call(fresh._h, 40, 8) == -3 and b"GP not set" in s.lib.gpmpc_last_error()
    fresh.set_gps(U.gp_objects(D.data(24, seed=3), slice(0, 24)), with_variance=False)
    assert call(fresh._h, 40, 8) == -3 and b"Linv" in s.lib.gpmpc_last_error()
    torch.cuda.synchronize()
    assert (pk.cpu().numpy()[:BMAX + 1] == -77).all() and np.isnan(sc.cpu().numpy()[:BMAX + 1]).all()
