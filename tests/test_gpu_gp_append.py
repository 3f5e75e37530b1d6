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
from gp_append_ref import MARGIN, reference, worst_ratio
from helpers import initial_states, lqr, problem, product_gps

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

SF2, SN2 = 1.0, 1e-3
NPTS = 64
GUARD = 64
SENTINEL = -7.25e77
RATIOS: dict = {}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


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


# ---------------------------------------------------------------------------- device side
_SOLVERS: dict = {}


def _solver(key, H=5, B=2, **kw):
    _torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    if key not in _SOLVERS:
        _SOLVERS[key] = BatchSolver(get_spec("quad2d"), H, B, **kw)
    return _SOLVERS[key]


def _gp_objects(data, rows):
    """GaussianProcess per GP on the given rows (an index array or slice) of the case's data."""
    torch = _torch()
    from gpmpc.gp import GaussianProcess

    gps = []
    for dg in data:
        gp = GaussianProcess(torch.tensor(dg["X"][rows]), torch.tensor(dg["y"][rows]))
        gp.set_hyperparameters(dg["ell"], SF2, SN2)
        gps.append(gp)
    return gps


def _guarded(P, dtype=None):
    torch = _torch()
    if dtype is torch.int32:
        t = torch.full((P + GUARD,), -77, dtype=torch.int32, device="cuda")
        t[P:] = -99
        return t
    t = torch.full((P + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    t[P:] = SENTINEL
    return t


def _read(t, P, what):
    a = t.cpu().numpy()
    if a.dtype == np.int32:
        assert (a[P:] == -99).all(), f"{what}: wrote past the end of the output"
        assert (a[:P] != -77).all(), f"{what}: output not written"
        return a[:P].copy()
    assert (a[P:] == SENTINEL).all(), f"{what}: wrote past the end of the output"
    assert not np.isnan(a[:P]).any(), f"{what}: {int(np.isnan(a[:P]).sum())} of {P} outputs not written"
    return a[:P].copy()


def _append(s, g, X, y, what):
    """gpmpc_gp_append of (X, y) to GP g with a guarded status array; returns the flags (host)."""
    torch = _torch()
    from gpmpc import _lib

    Xt = torch.tensor(np.ascontiguousarray(X, dtype=np.float64).reshape(len(y), -1), device="cuda")
    yt = torch.tensor(np.ascontiguousarray(y, dtype=np.float64), device="cuda")
    nb = (len(y) + 15) // 16
    fl = _guarded(nb, torch.int32)
    _lib.check(s.lib.gpmpc_gp_append(s._h, g, len(y), Xt.data_ptr(), yt.data_ptr(), fl.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return _read(fl, nb, what + " flags")


def _outputs(s, g, Z, what):
    """gp_predict mean / predictive variance and gp_mean_grad mean / gradient at Z, guarded."""
    torch = _torch()
    from gpmpc import _lib

    P, d = Z.shape
    Zt = torch.tensor(np.ascontiguousarray(Z), device="cuda")
    mb, vb, gm, gg = _guarded(P), _guarded(P), _guarded(P), _guarded(P * d)
    s.gp_predict(g, Zt, with_noise=True, mean=mb, var=vb)
    _lib.check(s.lib.gpmpc_gp_mean_grad(s._h, g, Zt.data_ptr(), P, gm.data_ptr(), gg.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return dict(mean=_read(mb, P, what + " mean"), var=_read(vb, P, what + " var"),
                tmean=_read(gm, P, what + " tile mean"), grad=_read(gg, P * d, what + " grad").reshape(P, d))


REFKEY = dict(mean="mean", var="var", tmean="mean", grad="grad")


def _compare(case, g, app, full, ref):
    """Appended handle's worst error <= MARGIN * the full re-upload's, per quantity."""
    for q in ("mean", "var", "tmean", "grad"):
        e_app, e_full, ratio = worst_ratio(app[q], full[q], ref[REFKEY[q]])
        RATIOS[(case, g, q)] = ratio
        print(f"[gp-append] {case} gp{g} {q}: e_app {e_app:.3e} e_full {e_full:.3e} ratio {ratio:.3f}")
    for q in ("mean", "var", "tmean", "grad"):
        assert RATIOS[(case, g, q)] <= MARGIN, (case, g, q, RATIOS[(case, g, q)])


def _upload(s, data, rows, capacity=None):
    s.set_gps(_gp_objects(data, rows))
    if capacity is not None:
        for g in range(2):
            s.reserve_gp(g, capacity)


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
    torch = _torch()
    from gpmpc import _lib

    Zt = torch.tensor(dg["Z"], device="cuda")

    def snap():
        m, v = s.gp_predict(g, Zt, with_noise=True, var=var)
        tm, tg = s.gp_mean_grad(g, Zt)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (m, v, tm, tg) if t is not None]

    before, size = snap(), s.gp_size(g)
    with pytest.raises(_lib.GPMPCError, match=rf"error {code}: .*{cause}"):
        s.append_gp(g, dg["X"][:1], dg["y"][:1])
    assert s.gp_size(g) == size
    after = snap()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))


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
    torch = _torch()
    from gpmpc.solver import BatchSolver

    H, B, tol = 5, 8, 1e-9
    spec, data, hyp = problem("quad2d", 57)
    mats = lqr(spec)
    traj = spec.reference_trajectory()
    x0, phase = initial_states(spec, traj, B)

    def handle(rows):
        s = BatchSolver(spec, H, B, tol=tol, qp_tol=1e-11, qp_max_iter=100)
        s.set_gps(product_gps([(X[:rows], y[:rows]) for X, y in data], hyp))
        s.set_tightening(True, 0.95, *mats)
        s.reset(reset_iterate=True)
        return s

    def append(s, lo, hi):
        for g, (X, y) in enumerate(data):
            assert s.append_gp(g, X[lo:hi], y[lo:hi]).cpu().tolist() == [1]

    sa, sb = handle(30), handle(48)
    stats = torch.zeros(B, sa.STATS_SLOTS, dtype=torch.int64, device="cuda")
    sa.set_stats(stats)
    for g in range(2):
        sa.reserve_gp(g, 57)
    append(sa, 30, 39)
    append(sa, 39, 48)
    assert [sa.gp_size(g) for g in range(2)] == [(48, 57)] * 2
    obs = [torch.tensor(x0, device="cuda"), torch.tensor(x0, device="cuda")]
    ts = [torch.tensor(phase, dtype=torch.int32, device="cuda") for _ in range(2)]
    lin_prev = stats[:, 9].clone()

    def step(i, s):
        u = s.solve(obs[i], ts[i].clone())
        out = dict(st=s.status.cpu().numpy(), it=s.sqp_iter.cpu().numpy())
        out["x"], out["u"], _ = (t.cpu().numpy() for t in s.solution())
        obs[i] = s.plant_step(obs[i], u.clone(), ts[i])
        return out

    def close(a, b):
        return float((np.abs(a - b) / (1 + np.abs(b))).max())

    for k in range(3):
        ra, rb = step(0, sa), step(1, sb)
        np.testing.assert_array_equal(ra["st"], rb["st"])
        assert np.isin(ra["st"], (0, 2)).all(), ra["st"]
        assert close(ra["x"], rb["x"]) <= 1e-6 and close(ra["u"], rb["u"]) <= 1e-6, (k, close(ra["x"], rb["x"]))
        if k > 0:   # (the first step after a reset runs no variance launch)
            va, vb = sa.variance().cpu().numpy(), sb.variance().cpu().numpy()
            assert close(va, vb) <= 1e-6, (k, close(va, vb))
        lin = stats[:, 9].clone()
        d = (lin - lin_prev).cpu().numpy()
        # step 0 follows the appends (and the reset): no cached rows; steps 1, 2 read the cache
        np.testing.assert_array_equal(d, ra["it"] + (1 if k == 0 else 0))
        lin_prev = lin
    append(sa, 48, 57)
    ra = step(0, sa)
    d = (stats[:, 9] - lin_prev).cpu().numpy()
    assert (d > 0).all()
    np.testing.assert_array_equal(d, ra["it"] + 1)   # the cache served nothing computed with the old model


def test_zz_report_ratios():
    """Largest measured e_app / e_full per quantity over the cases above (the figure DESIGN records)."""
    if not RATIOS:   # (run on its own: nothing to report)
        return
    for q in ("mean", "var", "tmean", "grad"):
        k = max((k for k in RATIOS if k[2] == q), key=lambda k: RATIOS[k])
        print(f"[gp-append] worst {q}: {RATIOS[k]:.3f} ({k[0]}, gp{k[1]})")
    print(f"[gp-append] worst ratio overall: {max(RATIOS.values()):.3f}")
    assert max(RATIOS.values()) <= MARGIN
