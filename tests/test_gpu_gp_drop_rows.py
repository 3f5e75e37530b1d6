"""Dropping arbitrary GP training rows on the device (gpmpc_gp_drop_rows; csrc/gp_drop.hip), MI355X only.

Setting, reference and yardstick are those of tests/test_gpu_gp_drop.py: a quad2d BatchSolver, gp_drop_ref.data
(sf2 = 1, sn2 = 1e-3), the np.longdouble recompute of the kept rows as reference and a second handle given a fresh
set_gps of the kept rows as yardstick.  Criterion: the dropped handle's worst error is at most gp_drop_rows_ref.MARGIN
times the yardstick's per quantity (MARGIN_ONE where one row is kept); the ratios are printed (-s).  Every output is
pre-filled with NaN (or -77) and followed by 64 sentinels."""

import numpy as np
import pytest

import gp_drop_ref as D
import gp_drop_rows_ref as DR
import gp_ref as R
import gp_update_util as U
from gp_append_ref import reference, worst_ratio
from gp_update_util import QUANT, REFKEY, SF2, SN2

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

RATIOS: dict = {}
_torch = U.gpu_torch


def _solver(key):
    return U.solver(__name__, key)


def _reference(dg, rows, Z=None):
    return reference(dg["X"][rows], dg["y"][rows], dg["ell"], SF2, SN2, dg["Z"] if Z is None else Z)


def _drop(s, g, idx, what):
    """gpmpc_gp_drop_rows with guarded outputs; returns (dropped, ok) on the host."""
    torch = _torch()
    from gpmpc import _lib

    m = len(idx)
    it = torch.tensor(np.asarray(idx, dtype=np.int32), device="cuda")
    dr, ok = U.guarded(m, torch.int32), U.guarded(1, torch.int32)
    _lib.check(s.lib.gpmpc_gp_drop_rows(s._h, g, m, it.data_ptr(), dr.data_ptr(), ok.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return U.read(dr, m, what + " dropped").tolist(), int(U.read(ok, 1, what + " ok")[0])


def _compare(case, g, got, full, ref, n_kept):
    for q in QUANT:
        e_drop, e_full, ratio = worst_ratio(got[q], full[q], ref[REFKEY[q]])
        RATIOS[(case, g, q)] = ratio
        print(f"[gp-drop-rows] {case} gp{g} {q}: e_drop {e_drop:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
    for q in QUANT:
        assert RATIOS[(case, g, q)] <= DR.margin(n_kept), (case, g, q, RATIOS[(case, g, q)])


@pytest.mark.parametrize("order", ["ascending", "permuted"])
@pytest.mark.parametrize("case,n,rows", DR.CASES, ids=DR.CASE_IDS)
def test_drop_matches_full_recompute(case, n, rows, order):
    idx = rows if order == "ascending" else DR.permuted(rows)
    kept = np.setdiff1d(np.arange(n), rows)
    data = DR.data(n)
    refs = [_reference(dg, kept) for dg in data]
    sa, sb = _solver("A"), _solver("B")
    U.upload(sa, data, slice(0, n), capacity=n)
    U.upload(sb, data, kept)
    for g, dg in enumerate(data):
        dropped, ok = _drop(sa, g, idx, f"{case} gp{g}")
        assert dropped == sorted(rows) and ok == 1, (case, g, dropped, ok)
        assert sa.gp_size(g) == (len(kept), n)
        got = U.outputs(sa, g, dg["Z"], f"{case} dropped gp{g}")
        full = U.outputs(sb, g, dg["Z"], f"{case} full gp{g}")
        _compare(f"{case} ({order})", g, got, full, refs[g], len(kept))


def test_python_call_and_the_invalid_index_rule():
    """BatchSolver.drop_rows returns device tensors; duplicates and indices out of range give the documented set and
    ok 0, and the GP is then what a valid call for that set leaves, bit for bit."""
    torch = _torch()
    data = DR.data(21)
    outs = []
    for key, idx in (("A", [7, 7, 30, -1]), ("B", [0, 1, 2, 7])):
        s = _solver(key)
        U.upload(s, data, slice(0, 21), capacity=24)
        res = []
        for g, dg in enumerate(data):
            dropped, ok = s.drop_rows(g, torch.tensor(idx, dtype=torch.int64) if g else idx)
            assert dropped.is_cuda and ok.is_cuda and dropped.dtype == ok.dtype == torch.int32 and ok.shape == (1,)
            assert dropped.cpu().tolist() == [0, 1, 2, 7] and ok.cpu().tolist() == [1 if key == "B" else 0]
            assert DR.normalise(idx, 21) == ([0, 1, 2, 7], 1 if key == "B" else 0)
            assert s.gp_size(g) == (17, 24)
            res.append(U.outputs(s, g, dg["Z"], f"index rule {key} gp{g}"))
        outs.append(res)
    for g in range(2):
        for q in QUANT:
            assert np.array_equal(outs[0][g][q], outs[1][g][q]), (g, q)
    # outputs that are not asked for are not written
    from gpmpc import _lib

    s = _solver("A")
    it = torch.tensor([3], dtype=torch.int32, device="cuda")
    _lib.check(s.lib.gpmpc_gp_drop_rows(s._h, 0, 1, it.data_ptr(), None, None, s._stream()))
    torch.cuda.synchronize()
    assert s.gp_size(0) == (16, 24)


def test_inert_rows_are_dropped_and_kept():
    """36 live rows and two rejected append blocks of 6 (rows 20..25 and 35..40 of 48); the drop takes inert rows 21,
    22, 23 and 36 with live rows around them and keeps the other eight.  The predictions at the case's points, at the
    kept live rows and at the inert rows' stored input (the origin) hold the ratio; one more append and one more drop
    (which takes two more inert rows) still do."""
    rows = (3, 19, 21, 22, 23, 26, 36, 47)
    data = D.data(36 + 5, seed=700)
    inert_old = np.r_[np.arange(20, 26), np.arange(35, 41)]
    orig = np.full(48, -1)
    orig[np.setdiff1d(np.arange(48), inert_old)] = np.arange(36)
    kept = np.setdiff1d(np.arange(48), rows)
    live = orig[kept[~np.isin(kept, inert_old)]]
    assert len(live) == 32
    pts = [np.vstack([dg["Z"], dg["X"][live], np.zeros((1, dg["d"]))]) for dg in data]
    refs = [_reference(dg, live, Z) for dg, Z in zip(data, pts)]
    sa, sb = _solver("A"), _solver("B")
    U.upload(sa, data, slice(0, 20), capacity=64)
    for g, dg in enumerate(data):
        U.nan_block(sa, g, dg["d"], 6, 11 + g)
        assert sa.append_gp(g, dg["X"][20:29], dg["y"][20:29]).cpu().tolist() == [1]
        U.nan_block(sa, g, dg["d"], 6, 13 + g)
        assert sa.append_gp(g, dg["X"][29:36], dg["y"][29:36]).cpu().tolist() == [1]
        assert sa.gp_size(g) == (48, 64)
        assert _drop(sa, g, rows, "inert") == (list(rows), 1)
        assert sa.gp_size(g) == (40, 64)
    U.upload(sb, data, live)
    for g, dg in enumerate(data):
        _compare("inert rows", g, U.outputs(sa, g, pts[g], f"inert dropped gp{g}"),
                 U.outputs(sb, g, pts[g], f"inert full gp{g}"), refs[g], 32)
    # kept rows 18 and 19 are old rows 20 and 24 (inert), kept row 0 is live row 0
    live2 = np.r_[live[1:], np.arange(36, 41)]
    refs2 = [_reference(dg, live2, Z) for dg, Z in zip(data, pts)]
    for g, dg in enumerate(data):
        assert sa.append_gp(g, dg["X"][36:41], dg["y"][36:41]).cpu().tolist() == [1]
        assert _drop(sa, g, (19, 0, 18), "inert, second drop") == ([0, 18, 19], 1)
        assert sa.gp_size(g) == (42, 64)
    U.upload(sb, data, live2)
    for g, dg in enumerate(data):
        _compare("inert rows, append and drop", g, U.outputs(sa, g, pts[g], f"inert 2 dropped gp{g}"),
                 U.outputs(sb, g, pts[g], f"inert 2 full gp{g}"), refs2[g], 36)


def test_two_handles_end_bit_identical():
    data = D.data(61, seed=900)
    outs = []
    for key in ("A", "B"):
        s = _solver(key)
        U.upload(s, data, slice(0, 40), capacity=64)
        res = []
        for g, dg in enumerate(data):
            assert _drop(s, g, (31, 2, 17, 16, 39), "det") == ([2, 16, 17, 31, 39], 1)
            assert s.append_gp(g, dg["X"][40:56], dg["y"][40:56]).cpu().tolist() == [1]
            assert _drop(s, g, tuple(range(1, 51, 3)) + (50,), "det")[1] == 1          # 18 rows: two blocks
            assert s.drop_gp(g, 5).cpu().tolist() == [1]
            assert s.gp_size(g) == (28, 64)
            res.append(U.outputs(s, g, dg["Z"], f"det {key} gp{g}"))
        outs.append(res)
    for g in range(2):
        for q in QUANT:
            assert np.array_equal(outs[0][g][q], outs[1][g][q]), (g, q)


def _refused(s, g, dg, idx, code, cause, var=True):
    with U.refused(s, g, dg, code, cause, var):
        s.drop_rows(g, idx)


def test_refusals_leave_the_gp_unchanged():
    from gpmpc import _lib

    data = D.data(24, seed=500)
    s = _solver("A")
    gps = U.gp_objects(data, slice(0, 24))
    s.set_gps(gps)
    for g, dg in enumerate(data):
        _refused(s, g, dg, [1], -3, "gpmpc_gp_reserve")   # no second factor buffer yet
        s.reserve_gp(g, 24)
        _refused(s, g, dg, [], -1, "no rows")
        _refused(s, g, dg, list(range(24)), -1, "at least one row stays")
        _refused(s, g, dg, list(range(25)), -1, "at least one row stays")
    # no Linv
    s.set_gps(gps, with_variance=False)
    for g, dg in enumerate(data):
        s.reserve_gp(g, 40)
        _refused(s, g, dg, [1], -3, "Linv", var=False)
    # FITC upload
    s.set_gps(gps, fitc=[(dg["X"][:8], np.linspace(0.5, 1.5, 8)) for dg in data])
    for g, dg in enumerate(data):
        _refused(s, g, dg, [1], -3, "FITC")
    # LOVE root installed; removing it lets the drop through
    s.set_gps(gps, variance="love", love_rank=8, love_force=True)
    for g, dg in enumerate(data):
        s.reserve_gp(g, 40)
        _refused(s, g, dg, [1], -3, "LOVE root")
        _lib.check(s.lib.gpmpc_set_gp_variance_root(s._h, g, 0, 0, None))
        assert s.drop_rows(g, [1])[1].cpu().tolist() == [1]
        assert s.gp_size(g) == (23, 40)
    # a GP that was never set
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    fresh = BatchSolver(get_spec("quad2d"), 5, 2)
    with pytest.raises(_lib.GPMPCError, match=r"error -3: GP not set"):
        fresh.drop_rows(0, [1])


def test_tightening_and_solve_after_a_scattered_drop():
    """U.ClosedLoop on 64 rows: handle A drops 16 scattered rows, handle B is a set_gps of the kept ones.  Identical
    statuses, 1e-6 agreement, and A's first step computes its linearisation afresh; so does the step after one more
    drop."""
    rows = np.array([0, 3, 7, 15, 16, 17, 22, 30, 31, 32, 40, 47, 48, 55, 62, 63])
    kept = np.setdiff1d(np.arange(64), rows)
    loop = U.ClosedLoop(64)
    sa = loop.handle(loop.data, loop.hyp)
    sb = loop.handle([(X[kept], y[kept]) for X, y in loop.data], loop.hyp)
    loop.start(sa, sb)
    for g in range(2):
        sa.reserve_gp(g, 64)
        dropped, ok = sa.drop_rows(g, rows[::-1].copy())
        assert dropped.cpu().tolist() == rows.tolist() and ok.cpu().tolist() == [1]
    assert [sa.gp_size(g) for g in range(2)] == [(48, 64)] * 2
    loop.three_steps()
    for g in range(2):
        assert sa.drop_rows(g, [5, 40])[1].cpu().tolist() == [1]
    loop.step_after_update()


def test_sliding_window_at_full_capacity():
    """Capacity 64 filled to the last row, then six rounds of redundant(16) + drop_rows + append 16 on both GPs; the
    Python side keeps the surviving rows from `dropped`.  The handle holds the margin against an upload of them."""
    torch = _torch()
    data = D.data(64 + 96, seed=800)
    sa, sb = _solver("A"), _solver("B")
    U.upload(sa, data, slice(0, 64), capacity=64)
    have = np.arange(64)
    for r in range(6):
        lo = 64 + 16 * r
        pick = sa.redundant(16)
        for g, dg in enumerate(data):
            dropped, ok = sa.drop_rows(g, pick)
            assert ok.cpu().tolist() == [1] and sa.gp_size(g) == (48, 64)
            assert sorted(pick.cpu().tolist()) == dropped.cpu().tolist()
            assert sa.append_gp(g, dg["X"][lo:lo + 16], dg["y"][lo:lo + 16]).cpu().tolist() == [1]
            assert sa.gp_size(g) == (64, 64)
        have = np.r_[np.delete(have, dropped.cpu().numpy()), np.arange(lo, lo + 16)]
    torch.cuda.synchronize()
    assert len(have) == 64 and len(set(have.tolist())) == 64
    print(f"[gp-drop-rows] sliding window: {int((have < 64).sum())} of the first 64 rows survive six rounds")
    refs = [_reference(dg, have) for dg in data]
    U.upload(sb, data, have)
    for g, dg in enumerate(data):
        _compare("sliding window", g, U.outputs(sa, g, dg["Z"], f"slide gp{g}"),
                 U.outputs(sb, g, dg["Z"], f"slide full gp{g}"), refs[g], 64)


def test_zz_report_ratios():
    """Largest measured e_drop / e_full per quantity over the tests above (the figures DESIGN records)."""
    if not RATIOS:   # (run on its own: nothing to report)
        return
    for q in QUANT:
        k = max((k for k in RATIOS if k[2] == q), key=lambda k: RATIOS[k])
        print(f"[gp-drop-rows] worst {q}: {RATIOS[k]:.3f} ({k[0]}, gp{k[1]})")
    bulk = [v for k, v in RATIOS.items() if not k[0].startswith("one row left")]
    if bulk:
        print(f"[gp-drop-rows] worst ratio with two rows or more kept: {max(bulk):.3f} (MARGIN {DR.MARGIN})")
    print(f"[gp-drop-rows] worst ratio overall: {max(RATIOS.values()):.3f} (MARGIN_ONE {DR.MARGIN_ONE})")
