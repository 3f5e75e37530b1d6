"""gpmpc_gp_select on the MI355X: m of P candidates picked greedily by conditional variance.

quad2d handle with H = 5 and B = 130, GPs of 24, 40 and 272 training rows (a ragged last tile on quads, a full last
tile, npad past 256 so the V kernel changes column group), P = 1, 40 and 130 candidates (the smallest pool, partial
point tiles, more than one workgroup of every kernel), m = 1, 17 and min(P, 33).  Among the candidates transition 7
duplicates transition 3 and transition 5 holds a NaN; the outputscales are not 1.  The picks must equal the
longdouble reference's (tests/gp_select_ref.py; the CPU test asserts that every gap between the best candidate and
the runner-up is 1000 times what rounding can move), pick 0 and its gain gpmpc_gp_informative's, bit for bit, and the
residual variances within MARGIN_SELECT of the error of the upload path for the GP with the picks appended."""

import numpy as np
import pytest

import gp_append_ref as A
import gp_drop_ref as D
import gp_select_ref as S
import gp_update_util as U
import observe_ref as OR

pytestmark = pytest.mark.gpu

OWNER = "select"
BMAX = 130


def _hyps(data):
    return [(dg["ell"], sf2, D.SN2) for dg, sf2 in zip(data, S.SF2)]


def _solver(n, key="A", extra=16):
    s = U.solver(OWNER, key, H=5, B=BMAX)
    data = S.case_data(n)
    U.upload(s, data, slice(0, n), capacity=n + extra, hyps=_hyps(data))
    return s, data


def _tensors(x, u):
    torch = U.gpu_torch()
    return torch.tensor(x, device="cuda"), torch.tensor(u, device="cuda")


def _select(s, x, u, m, gains=True, resid=True, ok=True):
    """The raw call with guarded outputs: picks, gains (m,), resid (n_gp, P), ok; nothing past their ends."""
    torch = U.gpu_torch()
    from gpmpc import _lib

    P, ngp = len(x), s.spec.n_gp
    xt, ut = _tensors(x, u)
    pk, gn, rs, okt = U.guarded(m, torch.int32), U.guarded(m), U.guarded(ngp * P), U.guarded(1, torch.int32)
    _lib.check(s.lib.gpmpc_gp_select(s._h, P, xt.data_ptr(), ut.data_ptr(), m, pk.data_ptr(),
                                     gn.data_ptr() if gains else None, rs.data_ptr() if resid else None,
                                     okt.data_ptr() if ok else None, s._stream()))
    torch.cuda.synchronize()
    out = dict(picks=U.read(pk, m, "picks"))
    g, r, o = gn.cpu().numpy(), rs.cpu().numpy(), okt.cpu().numpy()
    assert (g[m:] == U.SENTINEL).all() and (r[ngp * P:] == U.SENTINEL).all() and (o[1:] == -99).all(), "wrote past an end"
    out["gains"], out["resid"], out["ok"] = g[:m].copy(), r[:ngp * P].reshape(ngp, P).copy(), int(o[0])
    if not gains:
        assert np.isnan(out["gains"]).all()
    if not resid:
        assert np.isnan(out["resid"]).all()
    assert out["ok"] == (1 if ok else -77)
    return out


def _informative_top(s, x, u):
    torch = U.gpu_torch()
    pk, sc = s.informative(*_tensors(x, u), 1, scores=True)
    torch.cuda.synchronize()
    j = int(pk.cpu().numpy()[0])
    return j, sc.cpu().numpy()[j]


def _predict(s, Zs, finite):
    """Noise-free variances (n_gp, P) of the handle's GPs at the finite candidates, NaN elsewhere."""
    torch = U.gpu_torch()
    out = np.full((len(Zs), len(finite)), np.nan)
    for g, Z in enumerate(Zs):
        Zt = torch.tensor(np.ascontiguousarray(Z[finite]), device="cuda")
        out[g, finite] = s.gp_predict(g, Zt, with_noise=False, mean=False)[1].cpu().numpy()
    return out


def _full(gps, Zs, picks, finite):
    """The yardstick: the upload path (a host float64 recompute through set_gps) for the GPs with the picked rows
    appended, and gp_predict(with_noise=False) at the candidates."""
    fresh = U.solver(OWNER, "F", H=5, B=BMAX)
    Xs = S.appended(gps, Zs, picks, finite)
    data = [dict(X=X, y=D.targets(X), ell=gp["ell"]) for X, gp in zip(Xs, gps)]
    fresh.set_gps(U.gp_objects(data, slice(None), hyps=[(gp["ell"], gp["sf2"], gp["sn2"]) for gp in gps]))
    return _predict(fresh, Zs, finite)


def _check_accuracy(tag, got, full, ref, finite, sel=None):
    sel = finite if sel is None else sel
    for g in range(got.shape[0]):
        want = ref["resid"][g, sel].astype(np.float64)
        e_sel, e_full, ratio = A.worst_ratio(got[g, sel], full[g, sel], want)
        print(f"[select] {tag} gp{g}: e_sel {e_sel:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
        assert e_sel <= S.MARGIN_SELECT * e_full, (tag, g, e_sel, e_full)


@pytest.mark.parametrize("n", S.NS)
@pytest.mark.parametrize("P", S.PS)
def test_picks_gains_and_residuals_against_the_reference(n, P):
    s, _ = _solver(n)
    gps, Zs, _, finite = S.case_base(n, P)
    x, u = S.points(s.spec, P)
    top, top_score = _informative_top(s, x, u)
    for m in S.ms_for(P):
        ref = S.case_ref(n, P, m)
        out = _select(s, x, u, m)
        assert out["picks"].tolist() == ref["picks"].tolist(), (n, P, m)
        # step 0 is gpmpc_gp_informative's top pick and score, bit for bit
        assert out["picks"][0] == top and out["gains"][0] == top_score
        assert np.isfinite(out["gains"]).all() and (np.diff(out["gains"]) <= 0).all()
        if P > max(S.DUP):
            order = out["picks"].tolist()
            assert S.NANROW not in order   # (m < P here)
            if S.DUP[0] in order and S.DUP[1] in order:
                assert abs(order.index(S.DUP[0]) - order.index(S.DUP[1])) > 1
            # duplicated candidates carry equal bits
            assert (out["resid"][:, S.DUP[0]] == out["resid"][:, S.DUP[1]]).all()
        assert np.isfinite(out["resid"][:, finite]).all()
        _check_accuracy(f"n {n} P {P} m {m}", out["resid"], _full(gps, Zs, out["picks"], finite), ref, finite)
        # two calls give the same bits; without the optional outputs the picks are the same
        again = _select(s, x, u, m)
        for k in ("picks", "gains"):
            np.testing.assert_array_equal(again[k], out[k])
        np.testing.assert_array_equal(again["resid"][:, finite], out["resid"][:, finite])
        bare = _select(s, x, u, m, gains=False, resid=False, ok=False)
        assert bare["picks"].tolist() == out["picks"].tolist()


def test_every_candidate_picked_puts_the_nan_last():
    n, P = 24, 40
    s, _ = _solver(n)
    x, u = S.points(s.spec, P)
    gps, Zs, prep, finite = S.case_base(n, P)
    ref = S.greedy_from(prep, finite, Zs, P)
    out = _select(s, x, u, P)
    assert out["picks"].tolist() == ref["picks"].tolist() and sorted(out["picks"].tolist()) == list(range(P))
    assert out["picks"][-1] == S.NANROW and np.isnan(out["gains"][-1]) and np.isfinite(out["gains"][:-1]).all()
    _check_accuracy(f"n {n} P {P} m {P}", out["resid"], _full(gps, Zs, out["picks"], finite), ref, finite)
    # the wrapper returns the same
    torch = U.gpu_torch()
    pk, gn, rs, ok = s.select(*_tensors(x, u), P, gains=True, resid=True)
    assert pk.dtype == torch.int32 and pk.cpu().numpy().tolist() == out["picks"].tolist() and ok.cpu().tolist() == [1]
    np.testing.assert_array_equal(gn.cpu().numpy(), out["gains"])
    np.testing.assert_array_equal(rs.cpu().numpy()[:, finite], out["resid"][:, finite])
    assert len(s.select(*_tensors(x, u), 3)) == 2


def test_a_love_root_and_an_inert_block_change_nothing():
    n, P, m = 24, 40, 17
    s, data = _solver(n, extra=48)
    x, u = S.points(s.spec, P)
    ref = S.case_ref(n, P, m)
    out0 = _select(s, x, u, m)
    for g in range(2):
        rank, ok = s.love_root_gp(g, rank=8)
        assert ok == 1 and rank >= 1
    try:
        out1 = _select(s, x, u, m)
    finally:
        for g in range(2):
            s.drop_love_root(g)
    out2 = _select(s, x, u, m)
    for o in (out1, out2):
        assert o["picks"].tolist() == out0["picks"].tolist()
        np.testing.assert_array_equal(o["gains"], out0["gains"])
    # one rejected append per GP: 16 inert rows, npad 32 -> 48; the picks are still those of the live rows
    for g, dg in enumerate(data):
        U.nan_block(s, g, dg["d"], 16, seed=7 + g)
    assert [s.gp_size(g)[0] for g in range(2)] == [n + 16] * 2
    out3 = _select(s, x, u, m)
    assert out3["picks"].tolist() == ref["picks"].tolist() == out0["picks"].tolist()
    gps, Zs, _, finite = S.case_base(n, P)
    _check_accuracy("inert block", out3["resid"], _full(gps, Zs, out3["picks"], finite), ref, finite)


def test_appending_the_picks_gives_the_residual_variances():
    torch = U.gpu_torch()
    n, P, m = 40, 40, 17
    s, _ = _solver(n)
    x, u = S.points(s.spec, P)
    gps, Zs, _, finite = S.case_base(n, P)
    ref = S.case_ref(n, P, m)
    out = _select(s, x, u, m)
    s2, _ = _solver(n, key="B", extra=48)
    xt, ut = _tensors(x, u)
    xn = s2.plant_step(xt.nan_to_num(), ut.clone())
    inputs, _, accepted, _ = s2.observe(xt, ut, xn, pick=torch.tensor(out["picks"], device="cuda"))
    torch.cuda.synchronize()
    assert accepted.cpu().numpy().min() == 1 and s2.gp_size(0)[0] == n + m
    np.testing.assert_array_equal(inputs.cpu().numpy(), np.hstack(Zs)[out["picks"]])
    unpicked = finite.copy()
    unpicked[out["picks"]] = False
    _check_accuracy("appended", out["resid"], _predict(s2, Zs, finite), ref, finite, sel=unpicked)


def test_greedy_observe_and_online_episode():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.learning import run_online_episode
    from gpmpc.synthetic import DEFAULT_HYPERS, initial_states, make_training_data

    B, H, steps, cap = 16, 10, 5, 56
    ctrl = GPMPC("quad2d", horizon=H, batch=B, gp_capacity=cap)
    gps = []
    for i, (X, y) in enumerate(make_training_data(ctrl.model, 40, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS["quad2d"][i])
        gps.append(gp)
    ctrl.set_gaussian_processes(gps)
    x0, phase = initial_states(ctrl.model, ctrl.traj, B)
    out = run_online_episode(ctrl, x0, steps, append_per_step=8, seed=11, tstep0=phase, sliding=True,
                             device_data=True, select="greedy")
    assert np.isin(out["status"], [0, 2]).all(), np.unique(out["status"])
    assert out["n_train"].tolist() == [48] + [56] * (steps - 1)
    for step, pick in enumerate(out["pick"]):
        assert pick.shape == (8,) and len(set(pick.tolist())) == 8 and ((pick >= 0) & (pick < B)).all(), (step, pick)
    # GPMPC.observe(select="greedy") makes the same choice itself: the rows it returns are select's picks
    x, u, xn = (torch.tensor(a, device="cuda") for a in (out["obs"][-2], out["action"][-1], out["obs"][-1]))
    want = ctrl.solver.select(x, u, 4)[0]
    inputs, targets, accepted, dropped_ok = ctrl.observe(x, u, xn, m=4, select="greedy", evict_oldest=True)
    ref_inputs, ref_targets = ctrl.solver.preprocess(x, u, xn, pick=want)
    np.testing.assert_array_equal(inputs.cpu().numpy(), ref_inputs.cpu().numpy())
    np.testing.assert_array_equal(targets.cpu().numpy(), ref_targets.cpu().numpy())
    assert accepted.cpu().numpy().tolist() == [[1], [1]] and dropped_ok.cpu().numpy().tolist() == [[1], [1]]
    assert [ctrl.solver.gp_size(g) for g in range(2)] == [(cap, cap)] * 2
    with pytest.raises(ValueError, match="pass m, not pick"):
        ctrl.observe(x, u, xn, pick=want, select="greedy")


def test_refusals():
    torch = U.gpu_torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    s, _ = _solver(24)
    x, u = OR.transitions(s.spec, 300, seed=5)
    xt, ut = _tensors(x, u)
    pk, gn, rs, ok = U.guarded(300, torch.int32), U.guarded(300), U.guarded(600), U.guarded(1, torch.int32)

    def call(h, P, m, xp=xt.data_ptr(), up=ut.data_ptr(), pp=pk.data_ptr()):
        return s.lib.gpmpc_gp_select(h, P, xp, up, m, pp, gn.data_ptr(), rs.data_ptr(), ok.data_ptr(), s._stream())

    for P, m in ((0, 1), (BMAX + 1, 1), (40, 0), (40, 41), (300, 257)):
        assert call(s._h, P, m) == -1, (P, m)
    big = BatchSolver(get_spec("quad2d"), 5, 300)   # m > 256 alone
    big.set_gps(U.gp_objects(S.case_data(24), slice(0, 24)))
    assert call(big._h, 300, 257) == -1 and b"256" in s.lib.gpmpc_last_error()
    assert call(s._h, 40, 8, xp=None) == -1 and call(s._h, 40, 8, up=None) == -1 and call(s._h, 40, 8, pp=None) == -1
    fresh = BatchSolver(get_spec("quad2d"), 5, 40)
    assert call(fresh._h, 40, 8) == -3 and b"GP not set" in s.lib.gpmpc_last_error()
    fresh.set_gps(U.gp_objects(S.case_data(24), slice(0, 24)), with_variance=False)
    assert call(fresh._h, 40, 8) == -3 and b"Linv" in s.lib.gpmpc_last_error()
    torch.cuda.synchronize()
    assert (pk.cpu().numpy()[:300] == -77).all() and (ok.cpu().numpy()[:1] == -77).all()
    assert np.isnan(gn.cpu().numpy()[:300]).all() and np.isnan(rs.cpu().numpy()[:600]).all()
