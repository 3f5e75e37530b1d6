"""The rows the GPs would miss least (gpmpc_gp_redundant), the parts that need no GPU: the float64 model in the
kernel's summation order against the longdouble reference (the same picks, with the gap condition at every step),
non-decreasing scores, the final p against the leave-one-out variances of the reduced GPs, and what the rule is worth
on a window with clustered newest rows; for quad3d's three GPs with their own hyperparameters (and a row inert in one
of them only) also the scores against leave-one-out variances computed afresh, and that every GP decides a pick."""

import numpy as np
import pytest

import gp_append_ref as A
import gp_drop_rows_ref as DR
import gp_ref as R

LD = R.LD
pytestmark = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64 here")


@pytest.mark.parametrize("n,m", DR.RED_CASES + DR.GPU_RED_CASES)
def test_model_picks_the_reference_rows_and_every_step_meets_the_gap_condition(n, m):
    c = DR.red_case(n, m)
    model, ref = c["model"], c["ref"]
    assert model["ok"] == 1
    least, worst = np.inf, 0.0
    for t in range(m):
        err = DR.score_error(model["tables"][t], ref["tables"][t])
        if DR.structural_tie(n, m, t):   # two rows left: equal scores up to rounding, either may leave
            left = np.flatnonzero(~np.isnan(ref["tables"][t].astype(np.float64)))
            assert len(left) == 2 and ref["gaps"][t] <= 64 * (n * DR.SF2 / DR.SN2) * R.EPS64 * float(ref["scores"][t])
            assert model["picks"][t] in left
            continue
        least, worst = min(least, ref["gaps"][t]), max(worst, err)
        # the pick is decided by scores that differ by much more than either side's error
        assert ref["gaps"][t] >= DR.GAP_FACTOR * err, (n, m, t, ref["gaps"][t], err)
        assert model["picks"][t] == ref["picks"][t], (n, m, t)
    print(f"[redundant] n {n} m {m}: least gap {least:.3e}, worst score error {worst:.3e}, picks {ref['picks'].tolist()}")
    assert len(set(ref["picks"].tolist())) == m


@pytest.mark.parametrize("n,m", DR.RED_CASES)
def test_scores_do_not_decrease(n, m):
    c = DR.red_case(n, m)
    for run in (c["model"], c["ref"]):
        s = np.asarray(run["scores"], dtype=np.float64)
        assert np.isfinite(s).all() and (np.diff(s) >= 0).all(), (n, m)
        assert (s > 0).all()   # a leave-one-out variance


@pytest.mark.parametrize("n,m", DR.RED_CASES)
def test_final_p_gives_the_leave_one_out_variances_of_the_reduced_gp(n, m):
    """1 / p - sn2 after the picks against 1 / diag((K[k, k] + sn2 I)^-1) - sn2 computed afresh in longdouble.  Both
    sides are longdouble evaluations of a quantity whose condition is that of K + sn2 I, at most n sf2 / sn2."""
    c = DR.red_case(n, m)
    kept = np.flatnonzero(c["ref"]["open"])
    assert len(kept) == n - m
    for g, dg in enumerate(c["data"]):
        want = LD(1) / np.diag(DR.precision_ld(dg["X"][kept], dg["ell"])) - LD(DR.SN2)
        got = LD(1) / c["ref"]["p"][g][kept] - LD(DR.SN2)
        rel = float(np.abs(got / want - 1).max())
        bound = 64 * n * (n * DR.SF2 / DR.SN2) * float(np.finfo(LD).eps)
        print(f"[redundant loo] n {n} m {m} gp{g}: worst relative difference {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound
        # and the float64 model's p is the reference's to the factor's rounding (cond(K) eps64)
        rel64 = float(np.abs(c["model"]["p"][g][kept] / c["ref"]["p"][g][kept].astype(np.float64) - 1).max())
        assert rel64 <= 64 * (n * DR.SF2 / DR.SN2) * R.EPS64, rel64


def test_an_inert_row_scores_zero_and_is_picked_first():
    import gp_drop_ref as D

    dat = DR.data(21)
    states = [D.with_inert(D.upload_state(dg["X"], dg["y"], dg["ell"]), 9, 1) for dg in dat]
    out = DR.redundant_f64([s[1] for s in states], [(DR.SF2, DR.SN2)] * 2, 3)
    assert out["ok"] == 1 and out["picks"][0] == 9 and out["scores"][0] == 0.0 and (out["scores"][1:] > 0).all()
    # inert in one GP only: the other GP's term decides
    states[1] = D.upload_state(np.insert(dat[1]["X"], 9, 0.3, axis=0), np.insert(dat[1]["y"], 9, 0.1), dat[1]["ell"])
    out = DR.redundant_f64([s[1] for s in states], [(DR.SF2, DR.SN2)] * 2, 1)
    assert out["ok"] == 1 and out["scores"][0] > 0


# ------------------------------------------------------- quad3d: three GPs, each with its own outputscale and noise
@pytest.mark.parametrize("inert", [False, True], ids=["every row live", "a row inert in one GP"])
def test_three_gp_model_picks_the_reference_rows_and_every_step_meets_the_gap_condition(inert):
    c = DR.model_red_case(inert=inert)
    model, ref, m = c["model"], c["ref"], DR.M_RED_M
    assert model["ok"] == 1 and len({h for h in c["hyp"]}) == 3 and len({dg["ell"] for dg in c["data"]}) == 3
    errs = np.array([DR.score_error(model["tables"][t], ref["tables"][t]) for t in range(m)])
    factor = ref["gaps"] / errs
    print(f"[redundant quad3d] inert {inert}: least gap {ref['gaps'].min():.3e}, worst score error {errs.max():.3e}, "
          f"least factor {factor.min():.3e} (step {int(factor.argmin())}), picks {ref['picks'].tolist()}")
    assert (ref["gaps"] >= DR.GAP_FACTOR * errs).all(), (ref["gaps"], errs)
    assert model["picks"].tolist() == ref["picks"].tolist() and len(set(ref["picks"].tolist())) == m
    s = np.asarray(ref["scores"], dtype=np.float64)
    assert (np.diff(s) >= 0).all() and (s > 0).all()
    if inert:
        # the row is live in GPs 0 and 2: its score is theirs, it is not forced out first with score 0
        g, row = DR.M_INERT
        at = ref["picks"].tolist().index(row)
        assert at > 0 and s[at] > 0 and not c["live"][g][row] and c["states"][g][1][row, row] == 0.0
        rest = [q for q in range(3) if q != g]
        alone = DR.redundant_ld([c["Ps"][q] for q in rest], [c["hyp"][q] for q in rest], 1, forced=[row])
        assert float(ref["tables"][0][row]) == float(alone["scores"][0])


def _loo_scores(data, hyp, rows):
    """max_g of row i's latent leave-one-out variance over sf2_g among `rows`, each from a factorisation of the other
    rows (nothing shared with the recursion): sf2 - k_i^T (K_-i + sn2 I)^-1 k_i."""
    out = np.zeros((len(data), len(rows)), dtype=LD)
    for g, (dg, (sf2, sn2)) in enumerate(zip(data, hyp)):
        X = dg["X"][rows]
        for i in range(len(rows)):
            rest = np.delete(np.arange(len(rows)), i)
            K = R.kernel_ld(X[rest], dg["ell"], sf2, X[rest]) + LD(sn2) * np.eye(len(rest), dtype=LD)
            v = A.solve_lower_ld(A.chol_ld(K), R.kernel_ld(X[rest], dg["ell"], sf2, X[i:i + 1]).T.copy())
            out[g, i] = (LD(sf2) - (v * v).sum()) / LD(sf2)
    return out.max(0)


def test_three_gp_scores_are_the_leave_one_out_variances_with_each_gps_own_noise():
    c = DR.model_red_case()
    ref, n = c["ref"], DR.M_RED_N
    cond = max(n * sf2 / sn2 for sf2, sn2 in c["hyp"])
    for t in (0, 16):   # the start, and with 16 rows gone
        rows = np.flatnonzero(~np.isnan(ref["tables"][t].astype(np.float64)))
        assert len(rows) == n - t
        want = _loo_scores(c["data"], c["hyp"], rows)
        rel = float(np.abs(ref["tables"][t][rows] / want - 1).max())
        print(f"[redundant quad3d loo] step {t}: worst relative difference {rel:.3e}")
        # longdouble evaluations of a quantity whose condition is that of K + sn2 I (the bound of the test above)
        assert rel <= 64 * n * cond * float(np.finfo(LD).eps), rel


@pytest.mark.parametrize("inert", [False, True], ids=["every row live", "a row inert in one GP"])
@pytest.mark.parametrize("m", [17, 33])
def test_every_gp_decides_a_pick_of_the_three_gp_cases(m, inert):
    """Each GP's term is the score of at least one picked row, by more than the model's score error both ways, and the
    picks change when it is left out and when the loop reads GP 0's outputscale and noise for it: a device kernel with
    either defect cannot give the model's picks.  (m = 1 is a prefix of these runs.)"""
    c = DR.model_red_case(inert=inert)
    ref, model = c["ref"], c["model"]
    picks = ref["picks"][:m].tolist()
    err = max(DR.score_error(model["tables"][t], ref["tables"][t]) for t in range(m))
    decided = DR.red_decided_by(c["Ps"], c["hyp"], c["live"], picks, err)
    print(f"[redundant decides] m {m} inert {inert}: steps decided per GP {[len(d) for d in decided]}, first {[d[:1] for d in decided]}")
    for g in range(3):
        assert decided[g], (m, inert, g)
        rest = [q for q in range(3) if q != g]
        without = DR.redundant_ld([c["Ps"][q] for q in rest], [c["hyp"][q] for q in rest], m, live=[c["live"][q] for q in rest])
        assert without["picks"].tolist() != picks, (m, inert, g)
        if g:
            hyp = list(c["hyp"])
            hyp[g] = hyp[0]
            assert DR.redundant_ld(c["Ps"], hyp, m, live=c["live"])["picks"].tolist() != picks, (m, inert, g)


def _posterior_var_ld(X, ell, Z):
    K = R.kernel_ld(X, ell, DR.SF2, X) + LD(DR.SN2) * np.eye(len(X), dtype=LD)
    v = A.solve_lower_ld(A.chol_ld(K), R.kernel_ld(X, ell, DR.SF2, Z).T.copy())
    return LD(DR.SF2) - (v * v).sum(0)


def test_evicting_the_redundant_rows_keeps_more_of_the_window_than_evicting_the_oldest():
    """A full window of 48 rows in d = 1 (lengthscale 0.15, sf2 = 1, sn2 = 1e-3: d = 1 and a short lengthscale make
    the gap clear): the oldest 16 rows spread evenly over [-1, 1], the newest 32 four clusters of eight near-copies
    (1e-3 perturbations).  Sixteen rows leave.  By age the spread rows go and four spots are all that is left; by
    redundancy every pick is a cluster row and the window still covers the interval."""
    ell, m = 0.15, 16
    rng = np.random.default_rng(5)
    spread = np.linspace(-1.0, 1.0, 16)
    clusters = np.repeat(np.array([-0.63, -0.21, 0.19, 0.61]), 8) + 1e-3 * rng.uniform(-1, 1, 32)
    X = np.r_[spread, clusters][:, None]
    Z = np.linspace(-1.0, 1.0, 201)[:, None]
    ref = DR.redundant_ld([DR.precision_ld(X, ell)], [(DR.SF2, DR.SN2)], m)
    picks = ref["picks"]
    assert (picks >= 16).all(), picks                       # every pick is a cluster row
    assert np.bincount((picks - 16) // 8, minlength=4).max() <= 7   # and no cluster is emptied
    left_red = float(_posterior_var_ld(X[np.setdiff1d(np.arange(48), picks)], ell, Z).max())
    left_old = float(_posterior_var_ld(X[16:], ell, Z).max())
    print(f"[redundant window] largest posterior variance over the probes after {m} evictions: redundant "
          f"{left_red:.3e}, oldest {left_old:.3e}, ratio {left_red / left_old:.3e}; picks {picks.tolist()}")
    assert left_red < left_old
