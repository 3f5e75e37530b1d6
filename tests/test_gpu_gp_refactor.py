"""Refactorising an uploaded GP on the device (gpmpc_gp_refactor; csrc/gp_refactor.hip), MI355X only.

Setting, reference and yardstick are those of tests/test_gpu_gp_append.py and test_gpu_gp_drop.py: a
quad2d BatchSolver (GP 0 has d = 1, GP 1 has d = 3), data from tests/gp_ref.py with sf2 = 1,
sn2 = 1e-3 and targets sin(3 sum x) + 0.5 (gp_drop_ref.data); the reference is the np.longdouble
recompute (gp_append_ref.reference, which asserts var >= sn2 / 2 before any GPU call); the yardstick
is a second handle given a fresh set_gps with the same rows and hyperparameters, whose worst error
over the case's 64 points is e_full per quantity (gp_predict mean and predictive variance,
gp_mean_grad mean and gradient).

Criterion.  The refactorised handle's worst error is at most MARGIN_REFACTOR e_full
(gp_refactor_ref.py: four times the worst ratio of the float64 numpy model of the blocked
algorithm, measured on the CPU over the same cases).  The measured ratios are printed per case (run
with -s).

The handle's buffers cannot be read through the C ABI, so what a refactorisation leaves in them is
judged by its effect on the predictions.  Every output is pre-filled with NaN and followed by 64
sentinels.  Every refresh first refactorises with other hyperparameters and other targets,
so a call that left any part of the GP as it found it would not pass.
"""

import numpy as np
import pytest

import gp_drop_ref as D
import gp_ref as R
import gp_refactor_ref as G
import gp_update_util as U
from gp_append_ref import MARGIN, reference, worst_ratio
from gp_update_util import GUARD, QUANT, REFKEY, SF2, SN2

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

RATIOS: dict = {}
_torch = U.gpu_torch
_gp_objects = U.gp_objects
_guarded = U.guarded
_hyp = U.hyp
_nan_block = U.nan_block
_outputs = U.outputs
_upload = U.upload


def _solver(key):
    return U.solver(__name__, key)


def _refactor(s, g, y, hyp, what):
    """gpmpc_gp_refactor of GP g with a guarded status word; returns the flag (host)."""
    torch = _torch()
    from gpmpc import _lib

    yt = torch.tensor(np.ascontiguousarray(y, dtype=np.float64), device="cuda")
    fl = _guarded(1, torch.int32)
    _lib.check(s.lib.gpmpc_gp_refactor(s._h, g, yt.data_ptr(), *[float(v) for v in hyp], fl.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return int(U.read(fl, 1, what + " flag")[0])


def _scramble(s, g, y, hyp):
    """Leave GP g with another factor, other weights and another tile pack than the ones wanted."""
    ell, sf2, sn2 = hyp
    assert s.refactor_gp(g, 2.0 - np.asarray(y), 1.3 * ell, 3.0 * sf2, 10.0 * sn2).cpu().tolist() == [1]


def _compare(case, g, got, full, ref, bound=None, record=True):
    """The handle's worst error <= bound * the fresh upload's, per quantity (default MARGIN_REFACTOR)."""
    bound = G.MARGIN_REFACTOR if bound is None else bound
    ratios = {}
    for q in QUANT:
        e_got, e_full, ratios[q] = worst_ratio(got[q], full[q], ref[REFKEY[q]])
        if record:
            RATIOS[(case, g, q)] = ratios[q]
        print(f"[gp-refactor] {case} gp{g} {q}: e {e_got:.3e} e_full {e_full:.3e} ratio {ratios[q]:.3f} (bound {bound:g})")
    for q in QUANT:
        assert ratios[q] <= bound, (case, g, q, ratios[q], bound)


@pytest.mark.parametrize("n,cap", G.REFRESH, ids=G.REFRESH_IDS)
def test_refresh_matches_full_recompute(n, cap):
    torch = _torch()
    data = D.data(n, seed=G.seed_for(n))
    refs = [reference(dg["X"], dg["y"], *_hyp(dg), dg["Z"]) for dg in data]
    sa, sb = _solver("A"), _solver("B")
    _upload(sa, data, slice(0, n), capacity=cap)
    _upload(sb, data, slice(0, n))
    for g, dg in enumerate(data):
        _scramble(sa, g, dg["y"], _hyp(dg))
        fl = sa.refactor_gp(g, dg["y"], *_hyp(dg))
        assert fl.shape == (1,) and fl.dtype == torch.int32 and fl.is_cuda
        assert fl.cpu().tolist() == [1]
        assert sa.gp_size(g) == (n, cap)
        _compare(f"refresh {n}", g, _outputs(sa, g, dg["Z"], f"refresh {n} gp{g}"),
                 _outputs(sb, g, dg["Z"], f"refresh {n} full gp{g}"), refs[g])


@pytest.mark.parametrize("n", G.NEW_ROWS)
def test_new_hyperparameters_match_a_fresh_upload(n):
    """ell' = 0.8 ell, sf2' = 2, sn2' = 5e-3 against a fresh upload with the same values (the stats
    slot 9 check of a solve that follows is in test_closed_loop_after_new_hyperparameters)."""
    data = D.data(n, seed=G.seed_for(n))
    hyps = [G.new_hypers(dg) for dg in data]
    refs = [reference(dg["X"], dg["y"], *hyps[g], dg["Z"]) for g, dg in enumerate(data)]
    sa, sb = _solver("A"), _solver("B")
    _upload(sa, data, slice(0, n), capacity=n)
    _upload(sb, data, slice(0, n), hyps=hyps)
    for g, dg in enumerate(data):
        assert _refactor(sa, g, dg["y"], hyps[g], "new hyperparameters") == 1
        _compare(f"new hyperparameters {n}", g, _outputs(sa, g, dg["Z"], f"new {n} gp{g}"),
                 _outputs(sb, g, dg["Z"], f"new {n} full gp{g}"), refs[g])


def _drop(s, g, m):
    assert s.drop_gp(g, m).cpu().tolist() == [1] * ((m + 15) // 16)


def test_restores_the_yardstick_after_drift():
    """Capacity 64 filled, six rounds of drop 16 / append 16 (held to MARGIN_DROP, as the drop tests
    do), then one refactorisation: back within MARGIN_REFACTOR of a fresh upload."""
    data = D.data(64 + 96, seed=800)
    last = slice(96, 160)
    refs = [reference(dg["X"][last], dg["y"][last], *_hyp(dg), dg["Z"]) for dg in data]
    sa, sb = _solver("A"), _solver("B")
    _upload(sa, data, slice(0, 64), capacity=64)
    _upload(sb, data, last)
    for g, dg in enumerate(data):
        for r in range(6):
            lo = 64 + 16 * r
            _drop(sa, g, 16)
            assert sa.append_gp(g, dg["X"][lo:lo + 16], dg["y"][lo:lo + 16]).cpu().tolist() == [1]
        full = _outputs(sb, g, dg["Z"], f"drift full gp{g}")
        _compare("before the refresh", g, _outputs(sa, g, dg["Z"], f"drifted gp{g}"), full, refs[g],
                 bound=D.MARGIN_DROP, record=False)
        assert _refactor(sa, g, dg["y"][last], _hyp(dg), "after drift") == 1
        assert sa.gp_size(g) == (64, 64)
        _compare("after drift", g, _outputs(sa, g, dg["Z"], f"refreshed gp{g}"), full, refs[g])


def test_inert_rows_stay_inert():
    """20 rows, a rejected block of 6 (NaN target), an accepted block of 8, a rejected block of 5,
    then a refactorisation whose targets are NaN at the 11 inert rows: status 1, and the predictions
    (at the case's points, the live rows themselves and the inert rows' stored input, the origin)
    are those of the 28 accepted rows.  An append of 16 and a drop of 16 that follow keep their own
    margins."""
    data, mask, live = G.inert_case()
    sa, sb = _solver("A"), _solver("B")
    pts = [np.vstack([dg["Z"], dg["X"][:28], np.zeros((1, dg["d"]))]) for dg in data]
    refs = [reference(dg["X"][:28], dg["y"][:28], *_hyp(dg), Z) for dg, Z in zip(data, pts)]
    refs2 = [reference(dg["X"][:44], dg["y"][:44], *_hyp(dg), Z) for dg, Z in zip(data, pts)]
    refs3 = [reference(dg["X"][16:44], dg["y"][16:44], *_hyp(dg), Z) for dg, Z in zip(data, pts)]
    _upload(sa, data, slice(0, 20), capacity=64)
    for g, dg in enumerate(data):
        _nan_block(sa, g, dg["d"], 6, 21 + g)
        assert sa.append_gp(g, dg["X"][20:28], dg["y"][20:28]).cpu().tolist() == [1]
        _nan_block(sa, g, dg["d"], 5, 23 + g)
        assert sa.gp_size(g) == (39, 64)
        y = np.full(39, np.nan)
        y[live] = dg["y"][:28]
        _scramble(sa, g, np.where(mask, np.nan, 1.0 + np.arange(39.0)), _hyp(dg))
        assert _refactor(sa, g, y, _hyp(dg), "inert") == 1
        assert sa.gp_size(g) == (39, 64)
    _upload(sb, data, slice(0, 28))
    for g, dg in enumerate(data):
        _compare("inert rows", g, _outputs(sa, g, pts[g], f"inert gp{g}"), _outputs(sb, g, pts[g], f"inert full gp{g}"),
                 refs[g])
    for g, dg in enumerate(data):
        assert sa.append_gp(g, dg["X"][28:44], dg["y"][28:44]).cpu().tolist() == [1]
        assert sa.gp_size(g) == (55, 64)
    _upload(sb, data, slice(0, 44))
    for g, dg in enumerate(data):
        _compare("inert rows, then append", g, _outputs(sa, g, pts[g], f"inert + gp{g}"),
                 _outputs(sb, g, pts[g], f"inert + full gp{g}"), refs2[g], bound=MARGIN, record=False)
    for g, dg in enumerate(data):
        _drop(sa, g, 16)
        assert sa.gp_size(g) == (39, 64)
    _upload(sb, data, slice(16, 44))
    for g, dg in enumerate(data):
        _compare("inert rows, then drop", g, _outputs(sa, g, pts[g], f"inert - gp{g}"),
                 _outputs(sb, g, pts[g], f"inert - full gp{g}"), refs3[g], bound=D.MARGIN_BULK, record=False)


def test_append_and_drop_after_a_refactorisation():
    data = D.data(48 + 16, seed=1600)
    refs = [reference(dg["X"], dg["y"], *_hyp(dg), dg["Z"]) for dg in data]
    refs2 = [reference(dg["X"][16:], dg["y"][16:], *_hyp(dg), dg["Z"]) for dg in data]
    sa, sb = _solver("A"), _solver("B")
    _upload(sa, data, slice(0, 48), capacity=64)
    for g, dg in enumerate(data):
        _scramble(sa, g, dg["y"][:48], _hyp(dg))
        assert _refactor(sa, g, dg["y"][:48], _hyp(dg), "48 of 64") == 1
        assert sa.append_gp(g, dg["X"][48:], dg["y"][48:]).cpu().tolist() == [1]
        assert sa.gp_size(g) == (64, 64)
    _upload(sb, data, slice(0, 64))
    for g, dg in enumerate(data):
        _compare("then append", g, _outputs(sa, g, dg["Z"], f"then append gp{g}"),
                 _outputs(sb, g, dg["Z"], f"then append full gp{g}"), refs[g], bound=MARGIN, record=False)
        _drop(sa, g, 16)
        assert sa.gp_size(g) == (48, 64)
    _upload(sb, data, slice(16, 64))
    for g, dg in enumerate(data):
        _compare("then drop", g, _outputs(sa, g, dg["Z"], f"then drop gp{g}"),
                 _outputs(sb, g, dg["Z"], f"then drop full gp{g}"), refs2[g], bound=D.MARGIN_DROP, record=False)


def test_two_handles_end_bit_identical():
    data = D.data(56, seed=900)
    outs = []
    for key in ("A", "B"):
        s = _solver(key)
        _upload(s, data, slice(0, 40), capacity=64)
        res = []
        for g, dg in enumerate(data):
            assert s.append_gp(g, dg["X"][40:56], dg["y"][40:56]).cpu().tolist() == [1]
            _drop(s, g, 7)
            assert _refactor(s, g, dg["y"][7:56], G.new_hypers(dg), "det") == 1
            assert s.gp_size(g) == (49, 64)
            res.append(_outputs(s, g, dg["Z"], f"det {key} gp{g}"))
        outs.append(res)
    for g in range(2):
        for q in QUANT:
            assert np.array_equal(outs[0][g][q], outs[1][g][q]), (g, q)


def test_guard_reports_a_nan_target():
    data = D.data(33, seed=G.seed_for(33))
    s = _solver("A")
    _upload(s, data, slice(0, 33), capacity=40)
    for g, dg in enumerate(data):
        y = dg["y"].copy()
        y[17] = np.nan
        assert _refactor(s, g, y, _hyp(dg), "guard") == 0
        assert s.gp_size(g) == (33, 40)


def _refused(s, g, dg, code, cause, y="targets", hyp=None, var=True):
    """refactor_gp is refused with `code` and a message naming `cause`; size and predictions unchanged."""
    torch = _torch()
    from gpmpc import _lib

    fl = _guarded(1, torch.int32)
    hyp = _hyp(dg) if hyp is None else hyp
    with U.refused(s, g, dg, code, cause, var) as size:
        yt = None if y is None else torch.tensor(dg["y"][:size[0]], device="cuda")
        _lib.check(s.lib.gpmpc_gp_refactor(s._h, g, None if yt is None else yt.data_ptr(), *[float(v) for v in hyp],
                                           fl.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    assert (fl.cpu().numpy() == np.r_[-77, [-99] * GUARD]).all()   # nothing was queued


def test_refusals_leave_the_gp_unchanged():
    from gpmpc import _lib

    data = D.data(24, seed=500)
    s = _solver("A")
    gps = _gp_objects(data, slice(0, 24))
    s.set_gps(gps)
    for g, dg in enumerate(data):
        _refused(s, g, dg, -3, "gpmpc_gp_reserve")   # no second factor buffer yet
        s.reserve_gp(g, 24)
        _refused(s, g, dg, -1, "no targets", y=None)
        ell = dg["ell"]
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            _refused(s, g, dg, -1, "finite and positive", hyp=(bad, SF2, SN2))
            _refused(s, g, dg, -1, "finite and positive", hyp=(ell, bad, SN2))
            _refused(s, g, dg, -1, "finite and positive", hyp=(ell, SF2, bad))
        assert s.refactor_gp(g, dg["y"], *_hyp(dg)).cpu().tolist() == [1]   # and the valid call goes through
    # no Linv
    s.set_gps(gps, with_variance=False)
    for g, dg in enumerate(data):
        s.reserve_gp(g, 40)
        _refused(s, g, dg, -3, "Linv", var=False)
    # FITC upload
    s.set_gps(gps, fitc=[(dg["X"][:8], np.linspace(0.5, 1.5, 8)) for dg in data])
    for g, dg in enumerate(data):
        _refused(s, g, dg, -3, "FITC")
    # LOVE root installed; removing it lets the call through
    s.set_gps(gps, variance="love", love_rank=8, love_force=True)
    for g, dg in enumerate(data):
        s.reserve_gp(g, 40)
        _refused(s, g, dg, -3, "LOVE root")
        _lib.check(s.lib.gpmpc_set_gp_variance_root(s._h, g, 0, 0, None))
        assert s.refactor_gp(g, dg["y"], *_hyp(dg)).cpu().tolist() == [1]
        assert s.gp_size(g) == (24, 40)
    # a GP that was never set
    torch = _torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    fresh = BatchSolver(get_spec("quad2d"), 5, 2)
    yt = torch.zeros(4, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.GPMPCError, match=r"error -3: GP not set"):
        _lib.check(fresh.lib.gpmpc_gp_refactor(fresh._h, 0, yt.data_ptr(), 1.0, 1.0, 1e-3, None, fresh._stream()))


def test_closed_loop_after_new_hyperparameters():
    """quad2d H = 5, B = 8, NLP tolerance 1e-9, QP tolerance 1e-11.  Handle A: 64 rows uploaded with
    the default hyperparameters, then refactorised with (0.8 ell, 2 sf2, 5 sn2); handle B: set_gps
    with those.  Three closed-loop steps each (solve, plant_step): identical statuses; x, u and
    variance() agree within 1e-6 (1 + |.|), the append's and the drop's closed-loop bound.  A step of
    handle A that follows a refactorisation computes its first linearisation afresh (stats slot 9
    advances by sqp_iter + 1, against sqp_iter for a cache hit)."""
    loop = U.ClosedLoop(64)
    data, hyp = loop.data, loop.hyp
    new = [(0.8 * h[0], 2.0 * h[1], 5.0 * h[2]) for h in hyp]
    sa, sb = loop.handle(data, hyp), loop.handle(data, new)
    loop.start(sa, sb)
    for g in range(2):
        sa.reserve_gp(g, 64)
        assert sa.refactor_gp(g, data[g][1], *new[g]).cpu().tolist() == [1]
    assert [sa.gp_size(g) for g in range(2)] == [(64, 64)] * 2
    loop.three_steps()
    for g in range(2):
        assert sa.refactor_gp(g, data[g][1], *hyp[g]).cpu().tolist() == [1]
    loop.step_after_update()


def test_zz_report_ratios():
    """Largest measured ratio per quantity over the refactorised states above (the figures DESIGN records)."""
    if not RATIOS:   # (run on its own: nothing to report)
        return
    for q in QUANT:
        k = max((k for k in RATIOS if k[2] == q), key=lambda k: RATIOS[k])
        print(f"[gp-refactor] worst {q}: {RATIOS[k]:.3f} ({k[0]}, gp{k[1]})")
    print(f"[gp-refactor] worst ratio overall: {max(RATIOS.values()):.3f} (MARGIN_REFACTOR {G.MARGIN_REFACTOR})")
    assert max(RATIOS.values()) <= G.MARGIN_REFACTOR
