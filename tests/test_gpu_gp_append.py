"""Appending GP training rows on the device (gpmpc_gp_reserve / gpmpc_gp_append / gpmpc_gp_size;
csrc/gp_append.hip), MI355X only.

Setting.  A quad2d BatchSolver: GP 0 has d = 1, GP 1 has d = 3.  Inputs and evaluation points come
from tests/gp_ref.py (synthetic_gp, points: uniform in [-1, 1]^d, every kernel value in
[0.05, 1] sf2), sf2 = 1, sn2 = 1e-3, targets sin(3 sum x) + 0.5 (non-zero everywhere).

Reference.  A np.longdouble recompute on the concatenated data: K = k(X, X) + sn2 I
(gp_ref.kernel_ld; tests/gp_append_ref.py), its Cholesky factor, alpha = K^-1 y and v = L^-1 k(X, z) by forward / backward
substitution, all in longdouble (gp_ref.inv_lower_ld rounds the factor it is given to float64
first, which would put an error of the measured size into the reference, so the substitutions are
done here without that rounding): mean = k alpha, var = sf2 - |v|^2 + sn2, grad = d mean / d z.

Yardstick.  The existing upload path: a float64 full recompute (GaussianProcess.device_layout) fed
to set_gps on a second handle.  Its worst error over the case's 64 points against the same
reference is e_full, per quantity (gp_predict mean, gp_predict variance, gp_mean_grad mean,
gp_mean_grad gradient).  The appended handle's worst error must be at most 8 e_full: the numpy
model of the update measured 1.6, the margin allows for the MFMA's summation order and for the
rounding carried from block to block.  The measured ratio is printed per case (run with -s).

The variance is the predictive one (with_noise: the tightening's): before any GPU call the
reference variance is asserted to be at least sn2 / 2 at every point.

Every output of these tests is pre-filled with NaN and followed by 64 sentinels, as in
tests/test_gpu_gp_kernels.py.
"""

import numpy as np
import pytest

import gp_ref as R
import gp_update_util as U
from gp_append_ref import MARGIN, reference, worst_ratio
from gp_update_util import REFKEY, SF2, SN2

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

NPTS = 64
RATIOS: dict = {}
_torch = U.gpu_torch
_gp_objects = U.gp_objects
_outputs = U.outputs
_upload = U.upload


def _solver(key):
    return U.solver(__name__, key)


def _reference(X, y, ell, Z):
    return reference(X, y, ell, SF2, SN2, Z)   # (asserts var >= sn2 / 2: before any GPU call)


def _targets(X):
    return np.sin(3.0 * X.sum(1)) + 0.5


def _data(n, seed):
    """Per GP of quad2d (d = 1, 3): X (n, d), y (n,), ell, Z (NPTS, d)."""
    out = []
    for g, d in enumerate((1, 3)):
        gp = R.synthetic_gp(n, d, seed=seed + 17 * g, sf2=SF2, sn2=SN2)
        out.append(dict(X=gp["X"], y=_targets(gp["X"]), ell=gp["ell"], Z=R.points(NPTS, d, seed=seed + 17 * g + 5), d=d))
    return out


def _append(s, g, X, y, what):
    """gpmpc_gp_append of (X, y) to GP g with a guarded status array; returns the flags (host)."""
    torch = _torch()
    from gpmpc import _lib

    Xt = torch.tensor(np.ascontiguousarray(X, dtype=np.float64).reshape(len(y), -1), device="cuda")
    yt = torch.tensor(np.ascontiguousarray(y, dtype=np.float64), device="cuda")
    nb = (len(y) + 15) // 16
    fl = U.guarded(nb, torch.int32)
    _lib.check(s.lib.gpmpc_gp_append(s._h, g, len(y), Xt.data_ptr(), yt.data_ptr(), fl.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return U.read(fl, nb, what + " flags")


def _compare(case, g, app, full, ref):
    """Appended handle's worst error <= MARGIN * the full re-upload's, per quantity."""
    for q in ("mean", "var", "tmean", "grad"):
        e_app, e_full, ratio = worst_ratio(app[q], full[q], ref[REFKEY[q]])
        RATIOS[(case, g, q)] = ratio
        print(f"[gp-append] {case} gp{g} {q}: e_app {e_app:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
    for q in ("mean", "var", "tmean", "grad"):
        assert RATIOS[(case, g, q)] <= MARGIN, (case, g, q, RATIOS[(case, g, q)])


CASES = [("inside a tile", 5, (3,)), ("filling a tile exactly", 13, (3,)), ("crossing a tile boundary", 14, (5,)),
         ("aligned full block", 16, (16,)), ("several chunks in one call", 17, (40,)),
         ("many small appends", 20, (7,) * 12), ("crossing npad = 256", 250, (16,))]


@pytest.mark.parametrize("case,n0,blocks", CASES, ids=[c[0].replace(" ", "-") for c in CASES])
def test_append_matches_full_recompute(case, n0, blocks):
    n = n0 + sum(blocks)
    data = _data(n, seed=100 + n0)
    refs = [_reference(dg["X"], dg["y"], dg["ell"], dg["Z"]) for dg in data]
    sa, sb = _solver("A"), _solver("B")
    _upload(sa, data, slice(0, n0), capacity=n)
    assert [sa.gp_size(g) for g in range(2)] == [(n0, n), (n0, n)]
    for g, dg in enumerate(data):
        at = n0
        for m in blocks:
            fl = sa.append_gp(g, dg["X"][at:at + m], dg["y"][at:at + m])
            assert fl.shape == ((m + 15) // 16,) and fl.dtype == _torch().int32 and fl.is_cuda
            assert fl.cpu().tolist() == [1] * ((m + 15) // 16), (case, g, at)
            at += m
        assert sa.gp_size(g) == (n, n)
    _upload(sb, data, slice(0, n))
    for g, dg in enumerate(data):
        app = _outputs(sa, g, dg["Z"], f"{case} appended gp{g}")
        full = _outputs(sb, g, dg["Z"], f"{case} full gp{g}")
        _compare(case, g, app, full, refs[g])


def test_guard_rejected_blocks_are_inert():
    """A block with a NaN target (and one with a NaN input) reports 0, advances the size and leaves
    every prediction where it was; a following valid block reports 1 and matches the reference on
    the data without the rejected blocks; a block that duplicates training inputs is accepted."""
    n0, nbad, nok, ndup = 20, 6, 9, 5
    data = _data(n0 + nok, seed=300)
    sa, sb = _solver("A"), _solver("B")
    refs0 = [_reference(dg["X"][:n0], dg["y"][:n0], dg["ell"], dg["Z"]) for dg in data]
    refs1 = [_reference(dg["X"], dg["y"], dg["ell"], dg["Z"]) for dg in data]
    dup = [dict(dg, X=np.vstack([dg["X"], dg["X"][:ndup]]), y=np.concatenate([dg["y"], dg["y"][:ndup] + 0.25]))
           for dg in data]
    refs2 = [_reference(dg["X"], dg["y"], dg["ell"], dg["Z"]) for dg in dup]
    _upload(sa, data, slice(0, n0), capacity=64)
    _upload(sb, data, slice(0, n0))
    full0 = [_outputs(sb, g, dg["Z"], f"guard full0 gp{g}") for g, dg in enumerate(data)]
    for g, dg in enumerate(data):
        rng = np.random.default_rng(7 + g)
        Xb, yb = rng.uniform(-1, 1, (nbad, dg["d"])), rng.uniform(0.5, 1.5, nbad)
        yb[2] = np.nan
        assert _append(sa, g, Xb, yb, "NaN target").tolist() == [0]
        assert sa.gp_size(g) == (n0 + nbad, 64)
        _compare("guard: after a NaN target", g, _outputs(sa, g, dg["Z"], f"guard nan-y gp{g}"), full0[g], refs0[g])
        Xb2, yb2 = Xb.copy(), np.ones(nbad)
        Xb2[4, -1] = np.nan
        assert _append(sa, g, Xb2, yb2, "NaN input").tolist() == [0]
        assert sa.gp_size(g) == (n0 + 2 * nbad, 64)
        _compare("guard: after a NaN input", g, _outputs(sa, g, dg["Z"], f"guard nan-x gp{g}"), full0[g], refs0[g])
        assert _append(sa, g, dg["X"][n0:], dg["y"][n0:], "valid").tolist() == [1]
        assert sa.gp_size(g) == (n0 + 2 * nbad + nok, 64)
    _upload(sb, data, slice(0, n0 + nok))
    for g, dg in enumerate(data):
        _compare("guard: valid block after rejected ones", g, _outputs(sa, g, dg["Z"], f"guard valid gp{g}"),
                 _outputs(sb, g, dg["Z"], f"guard full1 gp{g}"), refs1[g])
        assert _append(sa, g, dup[g]["X"][n0 + nok:], dup[g]["y"][n0 + nok:], "duplicates").tolist() == [1]
    _upload(sb, dup, slice(0, n0 + nok + ndup))
    for g, dg in enumerate(dup):
        _compare("guard: duplicated inputs", g, _outputs(sa, g, dg["Z"], f"guard dup gp{g}"),
                 _outputs(sb, g, dg["Z"], f"guard full2 gp{g}"), refs2[g])


def test_reserved_capacity_is_not_overrun():
    """Capacity 64 filled to the last row (40 + 16 + 8): every output is guarded, the next row is refused."""
    from gpmpc import _lib

    n0, n = 40, 64
    data = _data(n, seed=400)
    refs = [_reference(dg["X"], dg["y"], dg["ell"], dg["Z"]) for dg in data]
    sa, sb = _solver("A"), _solver("B")
    _upload(sa, data, slice(0, n0), capacity=64)
    _upload(sb, data, slice(0, n))
    for g, dg in enumerate(data):
        assert _append(sa, g, dg["X"][n0:], dg["y"][n0:], "fill").tolist() == [1, 1]
        assert sa.gp_size(g) == (64, 64)
        app = _outputs(sa, g, dg["Z"], f"fill gp{g}")
        _compare("capacity 64 filled", g, app, _outputs(sb, g, dg["Z"], f"fill full gp{g}"), refs[g])
        with pytest.raises(_lib.GPMPCError, match=r"error -1: capacity exceeded"):
            sa.append_gp(g, dg["X"][:1], dg["y"][:1])
        again = _outputs(sa, g, dg["Z"], f"fill again gp{g}")
        assert all(np.array_equal(app[q], again[q]) for q in app)


def _refused(s, g, dg, code, cause, var=True):
    """append_gp of one row is refused with `code` and a message naming `cause`; predictions bit-identical."""
    with U.refused(s, g, dg, code, cause, var):
        s.append_gp(g, dg["X"][:1], dg["y"][:1])


def test_refusals_leave_the_gp_unchanged():
    from gpmpc import _lib

    data = _data(24, seed=500)
    s = _solver("A")
    gps = _gp_objects(data, slice(0, 24))
    # capacity exceeded: set_gps leaves the capacity at the uploaded size; a reserve of 30 holds 6 more rows
    s.set_gps(gps)
    for g, dg in enumerate(data):
        assert s.gp_size(g) == (24, 24)
        _refused(s, g, dg, -1, "capacity exceeded")
        s.reserve_gp(g, 30)
        with pytest.raises(_lib.GPMPCError, match=r"error -1: capacity exceeded"):
            s.append_gp(g, np.zeros((7, dg["d"])), np.ones(7))
        assert s.gp_size(g) == (24, 30)
        with pytest.raises(_lib.GPMPCError, match=r"error -1: capacity below"):
            s.reserve_gp(g, 23)
    # set_gps again: the capacity is back at the uploaded size
    s.set_gps(gps)
    assert s.gp_size(0) == (24, 24)
    # no Linv
    s.set_gps(gps, with_variance=False)
    for g, dg in enumerate(data):
        s.reserve_gp(g, 40)
        _refused(s, g, dg, -3, "Linv", var=False)
    # FITC upload
    fitc = [(dg["X"][:8], np.linspace(0.5, 1.5, 8)) for dg in data]
    s.set_gps(gps, fitc=fitc)
    for g, dg in enumerate(data):
        with pytest.raises(_lib.GPMPCError, match=r"error -3: FITC"):
            s.reserve_gp(g, 40)
        _refused(s, g, dg, -3, "FITC")
    # LOVE root installed; dropping it lets the append through
    s.set_gps(gps, variance="love", love_rank=8, love_force=True)
    for g, dg in enumerate(data):
        s.reserve_gp(g, 40)
        _refused(s, g, dg, -3, "LOVE root")
        _lib.check(s.lib.gpmpc_set_gp_variance_root(s._h, g, 0, 0, None))
        assert s.append_gp(g, dg["X"][:1] * 0.5, dg["y"][:1]).cpu().tolist() == [1]
        assert s.gp_size(g) == (25, 40)
    # a GP that was never set
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    fresh = BatchSolver(get_spec("quad2d"), 5, 2)
    with pytest.raises(_lib.GPMPCError, match=r"error -3: GP not set"):
        fresh.append_gp(0, np.zeros((1, 1)), np.ones(1))
    with pytest.raises(_lib.GPMPCError, match=r"error -3: GP not set"):
        fresh.reserve_gp(0, 8)


def test_tightening_and_solve_after_append():
    """quad2d H = 5, B = 8, NLP tolerance 1e-9, QP tolerance 1e-11 (the tight settings of
    test_gpu_launch.py).  Handle A: 30 rows uploaded, then 2 x 9 appended; handle B: set_gps on all 48.
    Three closed-loop steps each (solve, plant_step): identical statuses; x, u and variance() agree
    within 1e-6 (1 + |.|).  A step of handle A that follows an append computes its first
    linearisation (stats slot 9 advances by sqp_iter + 1, against sqp_iter for a cache hit)."""
    loop = U.ClosedLoop(57)
    data, hyp = loop.data, loop.hyp

    def append(s, lo, hi):
        for g, (X, y) in enumerate(data):
            assert s.append_gp(g, X[lo:hi], y[lo:hi]).cpu().tolist() == [1]

    sa, sb = (loop.handle([(X[:rows], y[:rows]) for X, y in data], hyp) for rows in (30, 48))
    loop.start(sa, sb)
    for g in range(2):
        sa.reserve_gp(g, 57)
    append(sa, 30, 39)
    append(sa, 39, 48)
    assert [sa.gp_size(g) for g in range(2)] == [(48, 57)] * 2
    loop.three_steps()
    append(sa, 48, 57)
    loop.step_after_update()


def test_zz_report_ratios():
    """Largest measured e_app / e_full per quantity over the cases above (the figure DESIGN records)."""
    if not RATIOS:   # (run on its own: nothing to report)
        return
    for q in ("mean", "var", "tmean", "grad"):
        k = max((k for k in RATIOS if k[2] == q), key=lambda k: RATIOS[k])
        print(f"[gp-append] worst {q}: {RATIOS[k]:.3f} ({k[0]}, gp{k[1]})")
    print(f"[gp-append] worst ratio overall: {max(RATIOS.values()):.3f}")
    assert max(RATIOS.values()) <= MARGIN
