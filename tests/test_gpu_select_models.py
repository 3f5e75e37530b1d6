"""The row-selection calls on models other than quad2d, MI355X only: gpmpc_gp_informative, gpmpc_gp_select and
gpmpc_gp_redundant loop over every GP of the model inside one launch, with a run-time n_gp and per-GP hyperparameters,
strides and scratch regions.

quad3d: three GPs (input dimensions 1, 3, 3 of a gathered row of 7 columns) that differ in everything: 24 rows (npad
32), 272 rows (npad past 256, the V kernel's second column group) and 40 rows (npad 48) reserved to 56, with their own
lengthscale, outputscale and noise.  cartpole: two GPs of 24 and 40 rows that read the same three columns of z (zcol 0
and 3 of a gathered row of 6) and share nothing else.  Handles of H = 5 and max_batch 130, pools of 40 and 130
candidates (and one of 1) with a duplicated transition, a NaN in a state column a GP reads and a NaN in a state column
no GP reads.  tests/test_gp_select_cpu.py and tests/test_gp_redundant_cpu.py hold the references of these cases to the
gap condition and show that every GP decides a pick: a kernel that leaves a GP out, or reads another GP's outputscale,
noise or size for it, cannot give the reference's picks."""

import numpy as np
import pytest

import gp_append_ref as A
import gp_drop_ref as D
import gp_drop_rows_ref as DR
import gp_ref as R
import gp_select_ref as S
import gp_update_util as U
import observe_ref as OR
import test_gpu_informative as TI
import test_gpu_redundant as TR
import test_gpu_select as TS

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

OWNER = "select_models"
BMAX = 130
CAPS = {"quad3d": (None, None, 56), "cartpole": (None, None)}
POOLS = [("quad3d", 40), ("quad3d", 130), ("cartpole", 40)]


def _hyps(data):
    return [(dg["ell"], dg["sf2"], dg["sn2"]) for dg in data]


def _handle(name, key="A", rows=None, caps=None, B=BMAX):
    s = U.solver(OWNER, key, H=5, B=B, model=name)
    data = S.model_data(name, rows)
    U.upload(s, data, slice(None), capacity=CAPS[name] if caps is None else caps, hyps=_hyps(data))
    return s, data


def _expected_scores(s, data, x, u):
    """max_g of gp_predict's noise-free variance over the outputscale, one call per GP on its columns of z."""
    torch = U.gpu_torch()
    Zs = S.gp_inputs(s.spec, x, u)
    var = [s.gp_predict(g, torch.tensor(Z, device="cuda"), with_noise=False, mean=False)[1].cpu().numpy()
           for g, Z in enumerate(Zs)]
    return OR.score(np.array(var), [dg["sf2"] for dg in data], np.hstack(Zs))


def _full(name, gps, Zs, picks, finite):
    """The yardstick: the upload path for the GPs with the picked rows appended, gp_predict(with_noise=False)."""
    fresh = U.solver(OWNER, "F", H=5, B=BMAX, model=name)
    Xs = S.appended(gps, Zs, picks, finite)
    data = [dict(X=X, y=D.targets(X)) for X in Xs]
    fresh.set_gps(U.gp_objects(data, slice(None), hyps=_hyps(gps)))
    return TS._predict(fresh, Zs, finite)


def _check_accuracy(tag, got, full, ref, finite, margin):
    assert got.shape == ref["resid"].shape == full.shape
    for g in range(got.shape[0]):
        want = ref["resid"][g, finite].astype(np.float64)
        e_sel, e_full, ratio = A.worst_ratio(got[g, finite], full[g, finite], want)
        print(f"[select models] {tag} gp{g}: e_sel {e_sel:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
        assert e_sel <= margin * e_full, (tag, g, e_sel, e_full)


def _check_select(name, s, P, ms, tag=""):
    """Every assertion of a pool: the reference's picks, informative's first pick, the residuals, the NaNs."""
    gps, Zs, _, finite = S.model_base(name, P)
    x, u = S.model_points(s.spec, P)
    top, top_score = TS._informative_top(s, x, u)
    for m in ms:
        ref = S.model_ref(name, P, m)
        out = TS._select(s, x, u, m)
        assert out["picks"].tolist() == ref["picks"].tolist(), (name, P, m)
        assert out["picks"][0] == top and out["gains"][0] == top_score
        assert np.isfinite(out["gains"]).all() and (np.diff(out["gains"]) <= 0).all()
        assert out["resid"].shape == (s.spec.n_gp, P) and np.isfinite(out["resid"][:, finite]).all()
        if P > S.NANROW2:
            assert S.NANROW not in out["picks"].tolist()   # (m < P here)
            assert (out["resid"][:, S.DUP[0]] == out["resid"][:, S.DUP[1]]).all()
            # the NaN in a column no GP reads changes nothing: the same bits as without it
            clean = TS._select(s, *S.model_points(s.spec, P, unread_nan=False), m)
            for k in ("picks", "gains"):
                np.testing.assert_array_equal(clean[k], out[k])
            np.testing.assert_array_equal(clean["resid"][:, finite], out["resid"][:, finite])
            assert finite[S.NANROW2] and np.isfinite(out["resid"][:, S.NANROW2]).all()
        if name == "cartpole":   # the same columns, other rows and hyperparameters: one GP evaluated twice would show
            assert (out["resid"][0, finite] != out["resid"][1, finite]).all()
        _check_accuracy(f"{tag}{name} P {P} m {m}", out["resid"], _full(name, gps, Zs, out["picks"], finite), ref, finite,
                        S.margin_for(P))
        again = TS._select(s, x, u, m)
        for k in ("picks", "gains"):
            np.testing.assert_array_equal(again[k], out[k])
        np.testing.assert_array_equal(again["resid"][:, finite], out["resid"][:, finite])
        bare = TS._select(s, x, u, m, gains=False, resid=False, ok=False)
        assert bare["picks"].tolist() == out["picks"].tolist()


@pytest.mark.parametrize("name,P", POOLS + [("quad3d", 1)])
def test_informative_scores_are_gp_predict_and_picks_follow_the_rank_rule(name, P):
    s, data = _handle(name)
    assert [s.gp_size(g) for g in range(s.spec.n_gp)] == [(n, n if c is None else c) for n, c in zip(S.M_ROWS[name], CAPS[name])]
    x, u = S.model_points(s.spec, P)
    want = _expected_scores(s, data, x, u)
    for m in sorted({1, min(17, P), P}):
        pick, score = TI._informative(s, x, u, m)
        np.testing.assert_array_equal(score, want)   # (bit for bit; NaN at the NaN candidate on both sides)
        assert pick.tolist() == OR.rank(score, m).tolist(), (name, P, m)
        assert ((pick >= 0) & (pick < P)).all() and len(set(pick.tolist())) == m
        if P > S.NANROW2:
            assert np.isnan(score[S.NANROW]) and np.isfinite(np.delete(score, S.NANROW)).all()
            assert score[S.DUP[0]] == score[S.DUP[1]]
            if m == P:
                assert pick[-1] == S.NANROW
    if P > S.NANROW2:
        # the NaN in a column no GP reads: the same scores as without it, and the candidate ranks where its score puts it
        _, clean = TI._informative(s, *S.model_points(s.spec, P, unread_nan=False), P)
        np.testing.assert_array_equal(clean, want)
        assert S.NANROW2 in OR.rank(want, P)[:P - 1].tolist()


@pytest.mark.parametrize("name,P", POOLS)
def test_select_picks_gains_and_residuals_against_the_reference(name, P):
    s, _ = _handle(name)
    _check_select(name, s, P, S.ms_for(P))


def test_select_of_a_single_candidate():
    s, _ = _handle("quad3d")
    _check_select("quad3d", s, 1, [1])


@pytest.mark.parametrize("name", ["quad3d", "cartpole"])
def test_every_candidate_picked_takes_the_unread_nan_and_puts_the_read_nan_last(name):
    P = 40
    s, _ = _handle(name)
    x, u = S.model_points(s.spec, P)
    out = TS._select(s, x, u, P)
    order = out["picks"].tolist()
    assert sorted(order) == list(range(P)) and order[-1] == S.NANROW
    assert np.isnan(out["gains"][-1]) and np.isfinite(out["gains"][:-1]).all() and (np.diff(out["gains"][:-1]) <= 0).all()
    assert order.index(S.NANROW2) < P - 1
    # the steps the CPU test holds to the gap condition
    m = S.ms_for(P)[-1]
    assert order[:m] == S.model_ref(name, P, m)["picks"].tolist()


def test_select_after_one_gp_has_grown_past_its_scratch_region():
    """The select scratch is carved from every GP's own padded rows: a first call with GP 1 at 24 rows, then GP 1 alone
    comes back at 272 and its V region must be made again."""
    name, P = "quad3d", 130
    s, _ = _handle(name, key="G", rows=(24, 24, 40), caps=(None, None, None))
    x, u = S.model_points(s.spec, P)
    small = TS._select(s, x, u, 33)
    assert np.isfinite(small["gains"]).all() and (np.diff(small["gains"]) <= 0).all() and len(set(small["picks"].tolist())) == 33
    s, _ = _handle(name, key="G", caps=(None, None, None))
    assert [s.gp_size(g)[0] for g in range(3)] == list(S.M_ROWS[name])
    _check_select(name, s, P, [17, 33], tag="regrown ")
    assert TS._select(s, x, u, 33)["picks"].tolist() != small["picks"].tolist()


# ------------------------------------------------------------------------------------------------ gpmpc_gp_redundant
RED_CAPS = (40, 56, 96)


def _red_handle(n, caps):
    s = U.solver(OWNER, "R", H=5, B=2, model="quad3d")
    data = DR.model_red_data()
    U.upload(s, data, slice(0, n), capacity=caps, hyps=[(dg["ell"], sf2, sn2) for dg, (sf2, sn2) in zip(data, DR.M_RED_HYP)])
    return s, data


def _snapshot(s, data):
    torch = U.gpu_torch()
    out = []
    for g, dg in enumerate(data):
        out += [t.cpu().numpy() for t in s.gp_predict(g, torch.tensor(dg["Z"], device="cuda"), with_noise=True)]
    return out


def _check_redundant(s, c, ms, tag):
    model, ref = c["model"], c["ref"]
    for m in ms:
        picks, scores, ok = TR._redundant(s, m, f"{tag} m {m}")
        allowed = ref["gaps"][:m] / DR.GAP_FACTOR
        assert ok == 1 and picks.tolist() == model["picks"][:m].tolist(), (tag, m, picks.tolist())
        err = np.abs(scores - model["scores"][:m])
        print(f"[redundant quad3d] {tag} m {m}: worst score difference to the model {err.max():.3e}, least allowed "
              f"{allowed.min():.3e}")
        assert (err <= allowed).all(), (tag, m)
        assert (np.diff(scores) >= 0).all() and (scores > 0).all()
        again = TR._redundant(s, m, f"{tag} m {m} again")
        assert np.array_equal(picks, again[0]) and np.array_equal(scores, again[1]) and again[2] == 1
    return picks, scores


def test_redundant_picks_of_three_gps_with_their_own_hyperparameters_and_strides():
    n = DR.M_RED_N
    s, data = _red_handle(n, RED_CAPS)
    assert [s.gp_size(g) for g in range(3)] == [(n, cap) for cap in RED_CAPS]
    before = _snapshot(s, data)
    _check_redundant(s, DR.model_red_case(), [1, 17, DR.M_RED_M], "three GPs")
    after = _snapshot(s, data)
    assert len(before) == len(after) == 6 and all(np.array_equal(a, b) for a, b in zip(before, after))
    assert [s.gp_size(g) for g in range(3)] == [(n, cap) for cap in RED_CAPS]


def test_a_row_inert_in_one_gp_only_is_ranked_by_the_others():
    g_in, row = DR.M_INERT
    s, data = _red_handle(row, (56, 56, 56))
    for g, dg in enumerate(data):
        if g == g_in:
            U.nan_block(s, g, dg["d"], 1, 3)
        else:
            assert s.append_gp(g, dg["X"][row:row + 1], dg["y"][row:row + 1]).cpu().tolist() == [1]
    assert [s.gp_size(g)[0] for g in range(3)] == [row + 1] * 3
    c = DR.model_red_case(inert=True)
    picks, scores = _check_redundant(s, c, [17, DR.M_RED_M], "inert in GP 1")
    # not forced out first with score 0: its score is the largest over the GPs in which it is live
    at = picks.tolist().index(row)
    assert at == c["model"]["picks"].tolist().index(row) and at > 0 and scores[at] > 0


# ---------------------------------------------------------------------------------------------- the Python surface
def test_quad3d_episode_with_greedy_selection_and_eviction_by_choice():
    torch = U.gpu_torch()
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.learning import run_online_episode
    from gpmpc.synthetic import DEFAULT_HYPERS, initial_states, make_training_data

    B, steps, cap = 16, 5, 56
    ctrl = GPMPC("quad3d", horizon=5, batch=B, gp_capacity=cap)
    gps = []
    for i, (X, y) in enumerate(make_training_data(ctrl.model, 40, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS["quad3d"][i])
        gps.append(gp)
    assert len(gps) == 3
    ctrl.set_gaussian_processes(gps)
    x0, phase = initial_states(ctrl.model, ctrl.traj, B)
    out = run_online_episode(ctrl, x0, steps, append_per_step=8, seed=11, tstep0=phase, sliding=True, device_data=True,
                             select="greedy", evict="redundant")
    assert np.isin(out["status"], [0, 2]).all(), np.unique(out["status"])
    assert out["n_train"].tolist() == [48] + [cap] * (steps - 1)
    assert len(out["pick"]) == steps
    for step, pick in enumerate(out["pick"]):
        assert pick.shape == (8,) and len(set(pick.tolist())) == 8 and ((pick >= 0) & (pick < B)).all(), (step, pick)
    assert [ctrl.solver.gp_size(g) for g in range(3)] == [(cap, cap)] * 3
