"""Dropping the oldest GP training rows on the device (gpmpc_gp_drop_oldest; csrc/gp_drop.hip),
MI355X only.

Setting, reference and yardstick are those of tests/test_gpu_gp_append.py: a quad2d BatchSolver
(GP 0 has d = 1, GP 1 has d = 3), data from tests/gp_ref.py with sf2 = 1, sn2 = 1e-3 and targets
sin(3 sum x) + 0.5 (gp_drop_ref.data); the reference is the np.longdouble recompute of the kept
rows (gp_append_ref.reference, which asserts var >= sn2 / 2 before any GPU call); the yardstick is a
second handle given a fresh set_gps of the kept rows, whose worst error over the case's 64 points is
e_full per quantity (gp_predict mean and predictive variance, gp_mean_grad mean and gradient).

Criterion.  The dropped handle's worst error is at most MARGIN_DROP e_full (gp_drop_ref.py: four
times the worst ratio of the float64 numpy model of the update, measured on the CPU over the same
cases), and, whenever at least two rows are kept, at most MARGIN_BULK e_full, the same rule without
the one case whose yardstick is exact to an ulp (17 - 16).  The measured ratios are printed per
case (run with -s).

The handle's buffers cannot be read through the C ABI, so what a drop leaves in them is judged by
its effect on the predictions (the numpy model's inert rows are checked to be exact zeros in
tests/test_gp_drop_cpu.py).  Every output is pre-filled with NaN and followed by 64 sentinels.
"""

import numpy as np
import pytest

import gp_drop_ref as D
import gp_ref as R
import gp_update_util as U
from gp_append_ref import reference, worst_ratio
from gp_update_util import QUANT, REFKEY, SF2, SN2

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

RATIOS: dict = {}
_torch = U.gpu_torch
_gp_objects = U.gp_objects
_nan_block = U.nan_block
_outputs = U.outputs
_upload = U.upload


def _solver(key):
    return U.solver(__name__, key)


def _reference(dg, rows, Z=None):
    return reference(dg["X"][rows], dg["y"][rows], dg["ell"], SF2, SN2, dg["Z"] if Z is None else Z)


def _drop(s, g, m, what):
    """gpmpc_gp_drop_oldest of m rows of GP g with a guarded status array; returns the flags (host)."""
    torch = _torch()
    from gpmpc import _lib

    nb = (m + 15) // 16
    fl = U.guarded(nb, torch.int32)
    _lib.check(s.lib.gpmpc_gp_drop_oldest(s._h, g, m, fl.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return U.read(fl, nb, what + " flags").tolist()


def _compare(case, g, got, full, ref, n_kept):
    """Dropped handle's worst error <= margin * the fresh upload's, per quantity."""
    for q in QUANT:
        e_drop, e_full, ratio = worst_ratio(got[q], full[q], ref[REFKEY[q]])
        RATIOS[(case, g, q)] = ratio
        print(f"[gp-drop] {case} gp{g} {q}: e_drop {e_drop:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
    bound = D.margin(n_kept)
    for q in QUANT:
        assert RATIOS[(case, g, q)] <= bound <= D.MARGIN_DROP, (case, g, q, RATIOS[(case, g, q)], bound)


@pytest.mark.parametrize("case,n,drops", D.CASES, ids=D.CASE_IDS)
def test_drop_matches_full_recompute(case, n, drops):
    torch = _torch()
    kept = slice(sum(drops), n)
    data = D.data(n, seed=600 + n)
    refs = [_reference(dg, kept) for dg in data]
    sa, sb = _solver("A"), _solver("B")
    _upload(sa, data, slice(0, n), capacity=n)
    _upload(sb, data, kept)
    for g, dg in enumerate(data):
        left = n
        for m in drops:
            fl = sa.drop_gp(g, m)
            assert fl.shape == ((m + 15) // 16,) and fl.dtype == torch.int32 and fl.is_cuda
            assert fl.cpu().tolist() == [1] * ((m + 15) // 16), (case, g, m)
            left -= m
            assert sa.gp_size(g) == (left, n)
        got = _outputs(sa, g, dg["Z"], f"{case} dropped gp{g}")
        full = _outputs(sb, g, dg["Z"], f"{case} full gp{g}")
        _compare(case, g, got, full, refs[g], left)


def test_inert_rows_are_dropped_and_kept():
    """36 live rows and two rejected append blocks of 6 (NaN target): rows 20..25 and 35..40 of 48.
    Dropping 28 rows takes the first inert block (inside the call's second 16-row block) and keeps
    the second one as rows 7..12 of 20.  The predictions at the case's points, at the kept live
    rows themselves and at the inert rows' stored input (the origin) hold the ratio against a fresh
    upload of live rows 22..35; one more valid append and one more drop still do."""
    data = D.data(36 + 5, seed=700)
    sa, sb = _solver("A"), _solver("B")
    live = slice(22, 36)
    pts = [np.vstack([dg["Z"], dg["X"][live], np.zeros((1, dg["d"]))]) for dg in data]
    refs = [_reference(dg, live, Z) for dg, Z in zip(data, pts)]
    refs2 = [_reference(dg, slice(25, 41), Z) for dg, Z in zip(data, pts)]
    _upload(sa, data, slice(0, 20), capacity=64)
    for g, dg in enumerate(data):
        _nan_block(sa, g, dg["d"], 6, 11 + g)
        assert sa.append_gp(g, dg["X"][20:29], dg["y"][20:29]).cpu().tolist() == [1]
        _nan_block(sa, g, dg["d"], 6, 13 + g)
        assert sa.append_gp(g, dg["X"][29:36], dg["y"][29:36]).cpu().tolist() == [1]
        assert sa.gp_size(g) == (48, 64)
        assert _drop(sa, g, 28, "inert") == [1, 1]
        assert sa.gp_size(g) == (20, 64)
    _upload(sb, data, live)
    for g, dg in enumerate(data):
        _compare("inert rows", g, _outputs(sa, g, pts[g], f"inert dropped gp{g}"),
                 _outputs(sb, g, pts[g], f"inert full gp{g}"), refs[g], 14)
    # the kept inert rows stay inert under a following append and leave with a following drop
    for g, dg in enumerate(data):
        assert sa.append_gp(g, dg["X"][36:41], dg["y"][36:41]).cpu().tolist() == [1]
        assert _drop(sa, g, 3, "inert, second drop") == [1]
        assert sa.gp_size(g) == (22, 64)
    _upload(sb, data, slice(25, 41))
    for g, dg in enumerate(data):
        _compare("inert rows, append and drop", g, _outputs(sa, g, pts[g], f"inert 2 dropped gp{g}"),
                 _outputs(sb, g, pts[g], f"inert 2 full gp{g}"), refs2[g], 16)


def test_sliding_window_at_full_capacity():
    """Capacity 64 filled to the last row, then six rounds of drop 16 / append 16: no original row is
    left, the size reads 64 / 64 after every round."""
    data = D.data(64 + 96, seed=800)
    last = slice(96, 160)
    refs = [_reference(dg, last) for dg in data]
    sa, sb = _solver("A"), _solver("B")
    _upload(sa, data, slice(0, 64), capacity=64)
    _upload(sb, data, last)
    for g, dg in enumerate(data):
        assert sa.gp_size(g) == (64, 64)
        for r in range(6):
            lo = 64 + 16 * r
            assert _drop(sa, g, 16, f"slide {r}") == [1]
            assert sa.gp_size(g) == (48, 64)
            assert sa.append_gp(g, dg["X"][lo:lo + 16], dg["y"][lo:lo + 16]).cpu().tolist() == [1]
            assert sa.gp_size(g) == (64, 64)
        _compare("sliding window", g, _outputs(sa, g, dg["Z"], f"slide gp{g}"),
                 _outputs(sb, g, dg["Z"], f"slide full gp{g}"), refs[g], 64)


def test_two_handles_end_bit_identical():
    data = D.data(61, seed=900)
    outs = []
    for key in ("A", "B"):
        s = _solver(key)
        _upload(s, data, slice(0, 40), capacity=64)
        res = []
        for g, dg in enumerate(data):
            assert _drop(s, g, 7, "det") == [1]
            assert s.append_gp(g, dg["X"][40:56], dg["y"][40:56]).cpu().tolist() == [1]
            assert _drop(s, g, 20, "det") == [1, 1]
            assert s.append_gp(g, dg["X"][56:61], dg["y"][56:61]).cpu().tolist() == [1]
            assert s.gp_size(g) == (34, 64)
            res.append(_outputs(s, g, dg["Z"], f"det {key} gp{g}"))
        outs.append(res)
    for g in range(2):
        for q in QUANT:
            assert np.array_equal(outs[0][g][q], outs[1][g][q]), (g, q)


def _refused(s, g, dg, m, code, cause, var=True):
    """drop_gp of m rows is refused with `code` and a message naming `cause`; size and predictions unchanged."""
    with U.refused(s, g, dg, code, cause, var):
        s.drop_gp(g, m)


def test_refusals_leave_the_gp_unchanged():
    from gpmpc import _lib

    data = D.data(24, seed=500)
    s = _solver("A")
    gps = _gp_objects(data, slice(0, 24))
    s.set_gps(gps)
    for g, dg in enumerate(data):
        _refused(s, g, dg, 1, -3, "gpmpc_gp_reserve")   # no second factor buffer yet
        s.reserve_gp(g, 24)
        _refused(s, g, dg, 0, -1, "no rows")
        _refused(s, g, dg, -3, -1, "no rows")
        _refused(s, g, dg, 24, -1, "at least one row stays")
        _refused(s, g, dg, 25, -1, "at least one row stays")
        assert s.drop_gp(g, 23).cpu().tolist() == [1, 1]   # down to one row is allowed
        assert s.gp_size(g) == (1, 24)
        _refused(s, g, dg, 1, -1, "at least one row stays")
    # no Linv
    s.set_gps(gps, with_variance=False)
    for g, dg in enumerate(data):
        s.reserve_gp(g, 40)
        _refused(s, g, dg, 1, -3, "Linv", var=False)
    # FITC upload
    s.set_gps(gps, fitc=[(dg["X"][:8], np.linspace(0.5, 1.5, 8)) for dg in data])
    for g, dg in enumerate(data):
        _refused(s, g, dg, 1, -3, "FITC")
    # LOVE root installed; removing it lets the drop through
    s.set_gps(gps, variance="love", love_rank=8, love_force=True)
    for g, dg in enumerate(data):
        s.reserve_gp(g, 40)
        _refused(s, g, dg, 1, -3, "LOVE root")
        _lib.check(s.lib.gpmpc_set_gp_variance_root(s._h, g, 0, 0, None))
        assert s.drop_gp(g, 1).cpu().tolist() == [1]
        assert s.gp_size(g) == (23, 40)
    # a GP that was never set
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    fresh = BatchSolver(get_spec("quad2d"), 5, 2)
    with pytest.raises(_lib.GPMPCError, match=r"error -3: GP not set"):
        fresh.drop_gp(0, 1)


def test_tightening_and_solve_after_drop():
    """quad2d H = 5, B = 8, NLP tolerance 1e-9, QP tolerance 1e-11.  Handle A: 64 rows uploaded, 16
    dropped; handle B: set_gps on rows 16..63.  Three closed-loop steps each (solve, plant_step):
    identical statuses; x, u and variance() agree within 1e-6 (1 + |.|), the append's closed-loop
    bound.  A step of handle A that follows a drop computes its first linearisation afresh (stats
    slot 9 advances by sqp_iter + 1, against sqp_iter for a cache hit)."""
    loop = U.ClosedLoop(64)
    sa, sb = (loop.handle([(X[lo:], y[lo:]) for X, y in loop.data], loop.hyp) for lo in (0, 16))
    loop.start(sa, sb)
    for g in range(2):
        sa.reserve_gp(g, 64)
        assert sa.drop_gp(g, 16).cpu().tolist() == [1]
    assert [sa.gp_size(g) for g in range(2)] == [(48, 64)] * 2
    loop.three_steps()
    for g in range(2):
        assert sa.drop_gp(g, 8).cpu().tolist() == [1]
    loop.step_after_update()


def test_zz_report_ratios():
    """Largest measured e_drop / e_full per quantity over the tests above (the figures DESIGN records)."""
    if not RATIOS:   # (run on its own: nothing to report)
        return
    for q in QUANT:
        k = max((k for k in RATIOS if k[2] == q), key=lambda k: RATIOS[k])
        print(f"[gp-drop] worst {q}: {RATIOS[k]:.3f} ({k[0]}, gp{k[1]})")
    bulk = [v for k, v in RATIOS.items() if k[0] != "one row left"]
    if bulk:
        print(f"[gp-drop] worst ratio with two rows or more kept: {max(bulk):.3f} (MARGIN_BULK {D.MARGIN_BULK})")
    print(f"[gp-drop] worst ratio overall: {max(RATIOS.values()):.3f} (MARGIN_DROP {D.MARGIN_DROP})")
    assert max(RATIOS.values()) <= D.MARGIN_DROP and (not bulk or max(bulk) <= D.MARGIN_BULK)
