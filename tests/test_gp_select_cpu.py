"""Greedy conditional-variance selection (gpmpc_gp_select), the parts that need no GPU: the longdouble reference
against a refactorised GP with the picks appended, the float64 model's ratio (R_MODEL), the gap condition of every
case of the GPU test, the clustered pool against the rank rule, and the build and Python plumbing; for the cases on
quad3d and cartpole (tests/test_gpu_select_models.py) also that every GP decides a pick and that the picks change
when a GP is left out or borrows another's outputscale and noise."""

import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import gp_append_ref as A
import gp_ref as R
import gp_select_ref as S
import observe_ref as OR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmpc_mi355x.h"
LD = R.LD

pytestmark = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64 here")


def _appended_ld(gps, Xs, Zs, finite):
    """sf2 - |L'^-1 k|^2 of the GPs on rows Xs at the finite candidates, in longdouble: (n_gp, P), NaN elsewhere."""
    out = np.full((len(gps), len(finite)), np.nan, dtype=LD)
    for g, (gp, X, Z) in enumerate(zip(gps, Xs, Zs)):
        K = R.kernel_ld(X, gp["ell"], gp["sf2"], X) + LD(float(gp["sn2"])) * np.eye(len(X), dtype=LD)
        v = A.solve_lower_ld(A.chol_ld(K), R.kernel_ld(X, gp["ell"], gp["sf2"], Z[finite]).T.copy())
        out[g, finite] = LD(float(gp["sf2"])) - (v * v).sum(0)
    return out


@pytest.mark.parametrize("n,P,m", [(24, 40, 17), (40, 40, 33), (40, 130, 17), (24, 40, 40)])
def test_residuals_are_the_variances_of_the_gp_with_the_picks_appended(n, P, m):
    gps, Zs, prep, finite = S.case_base(n, P)
    ref = S.greedy_from(prep, finite, Zs, m)
    want = _appended_ld(gps, S.appended(gps, Zs, ref["picks"], finite), Zs, finite)
    picked = np.zeros(P, dtype=bool)
    picked[ref["picks"]] = True
    for name, sel in (("unpicked", finite & ~picked), ("picked", finite & picked)):
        if not sel.any():   # (m = P: no finite candidate is left unpicked)
            assert m == P and name == "unpicked"
            continue
        err = float(np.abs(ref["resid"][:, sel] - want[:, sel]).max())
        print(f"[select ld] n {n} P {P} m {m} {name}: worst difference {err:.3e}")
        # both sides are longdouble sums of n + m terms of size sf2 at most: 4 (n + m) eps_ld sf2 bounds their difference
        assert err <= 4 * (n + m) * float(np.finfo(LD).eps) * max(S.SF2), (name, err)
    assert len(set(ref["picks"].tolist())) == m
    if m == P:   # the NaN candidate last, with a NaN gain
        assert ref["picks"][-1] == S.NANROW and np.isnan(ref["gains"][-1]) and np.isfinite(ref["gains"][:-1]).all()
    else:
        assert S.NANROW not in ref["picks"]
        order = ref["picks"].tolist()   # the twins are never neighbours
        if S.DUP[0] in order and S.DUP[1] in order:
            assert abs(order.index(S.DUP[0]) - order.index(S.DUP[1])) > 1


def test_gains_do_not_increase():
    for n, P, m in S.CASES:
        g = S.case_ref(n, P, m)["gains"]
        assert np.isfinite(g).all() and (np.diff(g) <= 0).all(), (n, P, m)


def _e_full(gps, Zs, ref):
    finite = ref["finite"]
    full = S.full64(gps, S.appended(gps, Zs, ref["picks"], finite), Zs, finite)
    return [float(np.abs(full[g, finite] - ref["resid"][g, finite].astype(np.float64)).max()) for g in range(len(gps))], full


def test_every_gpu_case_meets_the_gap_condition_and_the_model_its_margin():
    worst_ratio, worst_factor, least_gap = 0.0, np.inf, np.inf
    for n, P, m in S.CASES:
        gps, Zs, _, finite = S.case_base(n, P)
        ref = S.case_ref(n, P, m)
        e_full, full = _e_full(gps, Zs, ref)
        allowed = S.allowed_score_error(gps, e_full)
        gap = float(ref["gaps"].min())
        step = int(ref["gaps"].argmin())
        print(f"[select gap] n {n} P {P} m {m}: least gap {gap:.3e} (step {step}), allowed score error {allowed:.3e}, "
              f"factor {gap / allowed:.3e}")
        assert gap >= S.GAP_FACTOR * allowed, (n, P, m, gap, allowed)
        worst_factor, least_gap = min(worst_factor, gap / allowed), min(least_gap, gap)
        model = S.greedy_f64(gps, Zs, m)
        assert model["ok"] == 1 and model["picks"].tolist() == ref["picks"].tolist(), (n, P, m)
        for g in range(len(gps)):
            want = ref["resid"][g, finite].astype(np.float64)
            e_model, e_f, ratio = A.worst_ratio(model["resid"][g, finite], full[g, finite], want)
            print(f"[select model] n {n} P {P} m {m} gp{g}: e_model {e_model:.3e} e_full {e_f:.3e} ratio {ratio:.3f}")
            worst_ratio = max(worst_ratio, ratio)
    print(f"[select] R_MODEL measured {worst_ratio:.3f}; least gap {least_gap:.3e}, least factor {worst_factor:.3e}")
    assert worst_ratio <= S.R_MODEL, worst_ratio
    assert S.MARGIN_SELECT == float(np.ceil(4 * S.R_MODEL))


# ------------------------------------------------------------------ quad3d (three unequal GPs), cartpole (shared inputs)
def test_model_cases_share_nothing_but_cartpoles_input_columns():
    from gpmpc.models import get_spec

    assert get_spec("quad3d").gp_inputs == ((12,), (6, 9, 13), (7, 10, 14)) and get_spec("cartpole").gp_inputs[0] == \
        get_spec("cartpole").gp_inputs[1] == (2, 3, 4)
    for name, rows in S.M_ROWS.items():
        gps = S.model_data(name)
        assert [len(gp["X"]) for gp in gps] == list(rows)
        hyp = [(gp["ell"], gp["sf2"], gp["sn2"]) for gp in gps]
        for k in range(3):
            assert len({h[k] for h in hyp}) == len(gps), (name, k)
        spec = get_spec(name)
        Zs = S.gp_inputs(spec, *S.model_points(spec, 40))
        finite = S.finite_mask(Zs)
        # the NaN in a column a GP reads marks its candidate, the NaN in a column none reads does not
        assert np.flatnonzero(~finite).tolist() == [S.NANROW] and np.isnan(S.model_points(spec, 40)[0][S.NANROW2, S.UNREAD_COL])
        assert S.UNREAD_COL not in {c for idx in spec.gp_inputs for c in idx}
        if name == "quad3d":   # read by GP 2 alone
            assert [S.READ_COL[name] in idx for idx in spec.gp_inputs] == [False, False, True]
        for g, (gp, (lo, hi)) in enumerate(zip(gps, S.input_box(name))):
            # the training rows lie where the candidates do, and the start scores spread
            assert (gp["X"] >= lo).all() and (gp["X"] <= hi).all()
            inside = ((Zs[g][finite] >= lo) & (Zs[g][finite] <= hi)).all(1).mean()
            assert inside >= 0.9, (name, g, inside)
        _, _, prep, _ = S.model_base(name, 40)
        start = np.max(np.stack([(p["d"] / p["sf2"]).astype(np.float64) for p in prep]), axis=0)[finite]
        print(f"[select models] {name}: start scores {start.min():.3e} .. {np.median(start):.3e} .. {start.max():.3e}")
        assert start.max() < 0.5 and start.max() >= 10 * start.min()
    a, b = S.model_data("cartpole")
    assert a["X"].shape[1] == b["X"].shape[1] == 3 and not np.array_equal(a["X"], b["X"][:len(a["X"])])


@pytest.mark.parametrize("name,P,m", [("quad3d", 40, 33), ("quad3d", 130, 17), ("cartpole", 40, 33), ("cartpole", 40, 40)])
def test_model_residuals_are_the_variances_of_the_gps_with_the_picks_appended(name, P, m):
    gps, Zs, prep, finite = S.model_base(name, P)
    ref = S.greedy_from(prep, finite, Zs, m)
    want = _appended_ld(gps, S.appended(gps, Zs, ref["picks"], finite), Zs, finite)
    err = float(np.abs(ref["resid"][:, finite] - want[:, finite]).max())
    n = max(S.M_ROWS[name])
    print(f"[select ld] {name} P {P} m {m}: worst difference {err:.3e}")
    assert err <= 4 * (n + m) * float(np.finfo(LD).eps) * max(S.M_SF2), err
    assert len(set(ref["picks"].tolist())) == m and ref["resid"].shape == (len(gps), P)
    if m == P:
        assert ref["picks"][-1] == S.NANROW and np.isnan(ref["gains"][-1]) and np.isfinite(ref["gains"][:-1]).all()
    else:
        assert S.NANROW not in ref["picks"]


def test_every_model_case_meets_the_gap_condition_and_the_model_its_margin():
    worst, worst_factor, least_gap = {False: (0.0, None), True: (0.0, None)}, np.inf, np.inf
    for name, P, m in S.M_CASES:
        gps, Zs, _, finite = S.model_base(name, P)
        ref = S.model_ref(name, P, m)
        e_full, full = _e_full(gps, Zs, ref)
        allowed = S.allowed_score_error(gps, e_full)
        gap, step = float(ref["gaps"].min()), int(ref["gaps"].argmin())
        print(f"[select gap] {name} P {P} m {m}: least gap {gap:.3e} (step {step}), allowed score error {allowed:.3e}, "
              f"factor {gap / allowed:.3e}")
        assert (ref["gaps"] >= S.GAP_FACTOR * allowed).all(), (name, P, m, gap, allowed)
        worst_factor, least_gap = min(worst_factor, gap / allowed), min(least_gap, gap)
        model = S.greedy_f64(gps, Zs, m)
        assert model["ok"] == 1 and model["picks"].tolist() == ref["picks"].tolist(), (name, P, m)
        for g in range(len(gps)):
            want = ref["resid"][g, finite].astype(np.float64)
            e_model, e_f, ratio = A.worst_ratio(model["resid"][g, finite], full[g, finite], want)
            print(f"[select model] {name} P {P} m {m} gp{g}: e_model {e_model:.3e} e_full {e_f:.3e} ratio {ratio:.3f}")
            if ratio > worst[P == 1][0]:
                worst[P == 1] = (ratio, (name, P, m, g))
    print(f"[select models] e_model / e_full at worst {worst[False][0]:.3f} {worst[False][1]} over the pools of 40 and 130, "
          f"{worst[True][0]:.3f} {worst[True][1]} with one candidate; least gap {least_gap:.3e}, least factor {worst_factor:.3e}")
    # the pools stay within R_MODEL, so their GPU tests use MARGIN_SELECT; the single candidate has its own constant
    assert worst[False][0] <= S.R_MODEL, worst[False]
    assert worst[True][0] <= S.R_MODEL_ONE, worst[True]
    assert S.margin_for(40) == S.margin_for(130) == S.MARGIN_SELECT and S.margin_for(1) == float(np.ceil(4 * S.R_MODEL_ONE))


def _first_difference(a, b):
    return next((t for t in range(len(a)) if a[t] != b[t]), None)


@pytest.mark.parametrize("name,P,m", [(name, P, m) for name in S.M_ROWS for P in S.M_PS[name] for m in (17, 33)])
def test_every_gp_decides_a_pick_of_every_model_case(name, P, m):
    """What makes equal picks on the device mean that every GP was evaluated with its own data: each GP decides at
    least one step (its term is the largest at the pick, by more than the allowed error both ways), and the picks
    change when it is left out and when it borrows GP 0's outputscale and noise in the loop.  (The m = 1 cases are
    prefixes of these runs.)"""
    gps, Zs, prep, finite = S.model_base(name, P)
    ref = S.model_ref(name, P, m)
    e_full, _ = _e_full(gps, Zs, ref)
    allowed = S.allowed_score_error(gps, e_full)
    decided = S.decided_by(prep, ref, allowed)
    print(f"[select decides] {name} P {P} m {m}: steps decided per GP {[len(d) for d in decided]}, first {[d[:1] for d in decided]}")
    picks = ref["picks"].tolist()
    for g in range(len(gps)):
        assert decided[g], (name, P, m, g)
        rest = [q for q in range(len(gps)) if q != g]
        without = S.greedy_from([prep[q] for q in rest], finite, [Zs[q] for q in rest], m)["picks"].tolist()
        assert without != picks, (name, P, m, g)
        if g:
            borrowed = list(prep)
            borrowed[g] = dict(prep[g], sf2=prep[0]["sf2"], sn2=prep[0]["sn2"])
            other = S.greedy_from(borrowed, finite, Zs, m)["picks"].tolist()
            assert other != picks, (name, P, m, g)
            print(f"[select decides] gp{g}: first other pick without it at step {_first_difference(without, picks)}, "
                  f"with GP 0's sf2 and sn2 at step {_first_difference(other, picks)}")


def test_greedy_beats_the_rank_rule_on_a_clustered_pool():
    from gpmpc.models import get_spec

    spec = get_spec("quad2d")
    gps = S.gps_of(S.case_data(40), 40)
    Zs = S.gp_inputs(spec, *S.clustered_pool(spec))
    prep, finite = S.prepare_ld(gps, Zs)
    assert finite.all()
    m = 16
    greedy = S.greedy_from(prep, finite, Zs, m)
    start = OR.score(np.stack([p["d"] for p in prep]).astype(np.float64), S.SF2)
    ranked = S.greedy_from(prep, finite, Zs, m, forced=OR.rank(start, m))

    def left(r):
        return float(np.max(r["resid"].astype(np.float64) / np.array(S.SF2)[:, None]))

    clusters = lambda p: sorted(set((np.asarray(p) // S.COPIES).tolist()))   # noqa: E731
    print(f"[select pool] largest residual score after {m} picks: greedy {left(greedy):.3e} (transitions "
          f"{clusters(greedy['picks'])}), rank rule {left(ranked):.3e} (transitions {clusters(ranked['picks'])}), "
          f"ratio {left(greedy) / left(ranked):.3e}")
    assert left(greedy) < left(ranked)
    assert len(clusters(greedy["picks"])) > len(clusters(ranked["picks"]))


def _decl(name):
    m = re.search(rf"gpmpc_status\s+{name}\(([^)]*)\)\s*;", HEADER.read_text())
    assert m, f"{name} is not declared in the header"
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_header_signature_table_and_python_surface():
    from gpmpc import _lib
    from gpmpc.gpmpc import GPMPC
    from gpmpc.learning import run_online_episode
    from gpmpc.solver import BatchSolver

    P, I = ctypes.c_void_p, ctypes.c_int32
    cd = "const double*"
    assert _decl("gpmpc_gp_select") == ["gpmpc_handle*", "int32_t", cd, cd, "int32_t", "int32_t*", "double*", "double*",
                                        "int32_t*", "void*"]
    assert _lib.SIGNATURES["gpmpc_gp_select"] == (I, [P, I, P, P, I, P, P, P, P, P])
    assert list(inspect.signature(BatchSolver.select).parameters)[1:] == ["x", "u", "m", "gains", "resid"]
    assert "'greedy'" in inspect.getsource(GPMPC.observe) and "'greedy'" in inspect.getsource(run_online_episode)
    with pytest.raises(ValueError, match="device_data=True"):
        run_online_episode(None, None, 1, 1, 0, select="greedy")
    with pytest.raises(ValueError, match="select must be"):
        run_online_episode(None, None, 1, 1, 0, select="nearest")
