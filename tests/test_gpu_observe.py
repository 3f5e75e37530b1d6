"""gpmpc_gp_observe on the MI355X: transitions preprocessed and appended to every GP of the handle in one call.

The contract is bit-identity: handle A runs observe; handle B, uploaded with the same rows, runs preprocess, slices
the columns per GP and calls drop_gp / append_gp.  The predictions of every GP (gp_update_util.outputs at 64
points), gp_size and the accepted / dropped_ok flags must then be equal, bit for bit.  quad2d with H = 5 and
B = 40; one case on quad3d for the three-GP layout."""

import numpy as np
import pytest

import gp_drop_ref as D
import gp_update_util as U
import observe_ref as OR

pytestmark = pytest.mark.gpu

OWNER = "observe"
P = 40
CAP = 64
_T: dict = {}


def _transitions(s):
    """P transitions of the solver's model on the device: (x, u, x_next), one plant step with the true parameters."""
    torch = U.gpu_torch()
    if s.spec.name not in _T:
        x, u = OR.transitions(s.spec, P, seed=9)
        xt, ut = torch.tensor(x, device="cuda"), torch.tensor(u, device="cuda")
        _T[s.spec.name] = (xt, ut, s.plant_step(xt, ut))
    return _T[s.spec.name]


def _two_handles(n, capacity=CAP):
    sa, sb = U.solver(OWNER, "A", H=5, B=P), U.solver(OWNER, "B", H=5, B=P)
    data = D.data(n, seed=60 + n)
    for s in (sa, sb):
        U.upload(s, data, slice(0, n), capacity)
    return sa, sb, data


def _by_hand(s, x, u, xn, pick, m, evict):
    """What observe must equal: preprocess, a column slice per GP, drop_gp where needed, append_gp."""
    inputs, targets = s.preprocess(x, u, xn, pick=pick, m=m)
    rows = inputs.shape[0]
    accepted, dropped, col = [], [], 0
    for g, d in enumerate(s.spec.gp_dims):
        n, cap = s.gp_size(g)
        excess = n + rows - cap
        if evict and excess > 0:
            dropped.append(s.drop_gp(g, excess).cpu().numpy())
        else:
            dropped.append(np.ones(1, dtype=np.int32))
        accepted.append(s.append_gp(g, inputs[:, col:col + d].contiguous(), targets[:, g].contiguous()).cpu().numpy())
        col += d
    return inputs, targets, np.array(accepted), np.array(dropped)


def _same(sa, sb, data, out_a, out_b, what):
    for k in range(2):
        np.testing.assert_array_equal(out_a[k].cpu().numpy(), out_b[k].cpu().numpy(), err_msg=f"{what}: rows")
    np.testing.assert_array_equal(out_a[2].cpu().numpy(), out_b[2], err_msg=f"{what}: accepted")
    np.testing.assert_array_equal(out_a[3].cpu().numpy(), out_b[3], err_msg=f"{what}: dropped_ok")
    for g, dg in enumerate(data):
        assert sa.gp_size(g) == sb.gp_size(g)
        qa, qb = U.outputs(sa, g, dg["Z"], f"{what} A gp{g}"), U.outputs(sb, g, dg["Z"], f"{what} B gp{g}")
        for q in U.QUANT:
            np.testing.assert_array_equal(qa[q], qb[q], err_msg=f"{what}: gp{g} {q}")


@pytest.mark.parametrize("m", [1, 16, 17, 40])
def test_observe_is_preprocess_plus_append_bit_for_bit(m):
    sa, sb, data = _two_handles(24)
    x, u, xn = _transitions(sa)
    out_a = sa.observe(x, u, xn, m=m)
    out_b = _by_hand(sb, x, u, xn, None, m, False)
    _same(sa, sb, data, out_a, out_b, f"m = {m}")
    assert [sa.gp_size(g) for g in range(2)] == [(24 + m, CAP)] * 2
    assert out_a[2].shape == (2, (m + 15) // 16) and (out_a[2].cpu().numpy() == 1).all()
    assert out_a[3].cpu().numpy().tolist() == [[1], [1]]


def test_observe_with_picks_and_eviction():
    torch = U.gpu_torch()
    sa, sb, data = _two_handles(56)
    x, u, xn = _transitions(sa)
    pick = torch.tensor(np.random.default_rng(4).permutation(P)[:24].astype(np.int32), device="cuda")
    out_a = sa.observe(x, u, xn, pick=pick, evict_oldest=True)   # 56 + 24 - 64: drops 16
    out_b = _by_hand(sb, x, u, xn, pick, None, True)
    _same(sa, sb, data, out_a, out_b, "eviction")
    assert [sa.gp_size(g) for g in range(2)] == [(CAP, CAP)] * 2
    assert out_a[3].cpu().numpy().tolist() == [[1], [1]] and out_a[2].cpu().numpy().tolist() == [[1, 1]] * 2


def test_a_nan_transition_makes_its_block_inert():
    sa, sb, data = _two_handles(24)
    x, u, xn = _transitions(sa)
    xn = xn.clone()
    xn[20] = float("nan")   # row 20: block 1 of 33 rows
    out_a = sa.observe(x, u, xn, m=33)
    out_b = _by_hand(sb, x, u, xn, None, 33, False)
    assert out_a[2].cpu().numpy().tolist() == [[1, 0, 1]] * 2
    assert [sa.gp_size(g) for g in range(2)] == [(57, CAP)] * 2
    # (the returned rows hold the NaN targets: compared with it in place)
    assert np.isnan(out_a[1].cpu().numpy()[20]).all()
    _same(sa, sb, data, out_a, out_b, "a NaN transition")


def test_an_out_of_range_pick_makes_its_block_inert():
    torch = U.gpu_torch()
    sa, sb, data = _two_handles(24)
    x, u, xn = _transitions(sa)
    pick = torch.tensor(np.r_[np.arange(17), P, np.arange(17, 20)].astype(np.int32), device="cuda")
    out_a = sa.observe(x, u, xn, pick=pick)
    out_b = _by_hand(sb, x, u, xn, pick, None, False)
    assert out_a[2].cpu().numpy().tolist() == [[1, 0]] * 2
    _same(sa, sb, data, out_a, out_b, "a pick out of range")


def test_quad3d_three_gps():
    torch = U.gpu_torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver
    from helpers import problem, product_gps

    spec, data, hyp = problem("quad3d", 24)
    handles = []
    for _ in range(2):
        s = BatchSolver(get_spec("quad3d"), 5, P)
        s.set_gps(product_gps(data, hyp))
        for g in range(3):
            s.reserve_gp(g, 48)
        handles.append(s)
    sa, sb = handles
    x, u, xn = _transitions(sa)
    out_a = sa.observe(x, u, xn, m=17)
    out_b = _by_hand(sb, x, u, xn, None, 17, False)
    assert out_a[0].shape == (17, 7) and out_a[1].shape == (17, 3) and out_a[2].shape == (3, 2)
    for k in range(2):
        np.testing.assert_array_equal(out_a[k].cpu().numpy(), out_b[k].cpu().numpy())
    np.testing.assert_array_equal(out_a[2].cpu().numpy(), out_b[2])
    rng = np.random.default_rng(2)
    for g, (X, _) in enumerate(data):
        assert sa.gp_size(g) == sb.gp_size(g) == (41, 48)
        Z = X[rng.integers(0, len(X), 64)] + 0.05 * rng.standard_normal((64, X.shape[1]))
        qa, qb = U.outputs(sa, g, Z, f"quad3d A gp{g}"), U.outputs(sb, g, Z, f"quad3d B gp{g}")
        for q in U.QUANT:
            np.testing.assert_array_equal(qa[q], qb[q], err_msg=f"quad3d gp{g} {q}")


def test_refusals_leave_every_gp_unchanged():
    torch = U.gpu_torch()
    from gpmpc import _lib
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    sa, _, data = _two_handles(56)
    x, u, xn = _transitions(sa)
    for g, dg in enumerate(data):
        with U.refused(sa, g, dg, -1, "capacity exceeded"):
            sa.observe(x, u, xn, m=24)
        with U.refused(sa, g, dg, -1, "max_batch"):
            sa.observe(x, u, xn, pick=torch.zeros(P + 1, dtype=torch.int32, device="cuda"), evict_oldest=True)
        with U.refused(sa, g, dg, -1, "dt_diff"):
            _lib.check(sa.lib.gpmpc_gp_observe(sa._h, P, x.data_ptr(), u.data_ptr(), xn.data_ptr(), 4, None, 0.0, 9.81, 1,
                                               None, None, None, None, sa._stream()))
    sa, _, data = _two_handles(24, capacity=24)
    for g, dg in enumerate(data):
        with U.refused(sa, g, dg, -1, "at least one row stays"):
            sa.observe(x, u, xn, m=40, evict_oldest=True)
    sa, _, data = _two_handles(24)
    for g, dg in enumerate(data):
        assert sa.love_root_gp(g, rank=8)[1] == 1
        for k, dk in enumerate(data):
            with U.refused(sa, k, dk, -3, "LOVE root"):
                sa.observe(x, u, xn, m=8)
        sa.drop_love_root(g)
        assert sa.fitc_gp(g, np.arange(0, 24, 3), dg["y"][:24], 1e-8) == 1
        for k, dk in enumerate(data):
            with U.refused(sa, k, dk, -3, "FITC mean is installed"):
                sa.observe(x, u, xn, m=8)
        sa.drop_fitc(g)
    sa, _, data = _two_handles(24, capacity=None)   # no reserve: nothing can be dropped
    for g, dg in enumerate(data):
        with U.refused(sa, g, dg, -3, "gpmpc_gp_reserve"):
            sa.observe(x, u, xn, m=8, evict_oldest=True)
    # GPs that differ in their rows
    sa, _, data = _two_handles(24)
    assert sa.append_gp(0, data[0]["X"][:1] + 0.5, data[0]["y"][:1]).cpu().tolist() == [1]
    for g, dg in enumerate(data):
        with U.refused(sa, g, dg, -3, "differ"):
            sa.observe(x, u, xn, m=8)
    fresh = BatchSolver(get_spec("quad2d"), 5, P)
    with pytest.raises(_lib.GPMPCError, match=r"error -3: .*GP not set"):
        fresh.observe(x, u, xn, m=8)
    # after all that an observe still goes through
    sa, sb, data = _two_handles(24)
    _same(sa, sb, data, sa.observe(x, u, xn, m=8), _by_hand(sb, x, u, xn, None, 8, False), "after the refusals")


def test_closed_loop_after_observe_agrees_with_a_fresh_upload():
    torch = U.gpu_torch()
    loop = U.ClosedLoop(30)
    data, hyp = loop.data, loop.hyp
    sa = loop.handle(data, hyp)
    for g in range(2):
        sa.reserve_gp(g, 48)
    x = torch.tensor(loop.x0, device="cuda")
    u = torch.tensor(np.random.default_rng(6).uniform(loop.spec.u_lo, loop.spec.u_hi, (loop.B, loop.spec.nu)), device="cuda")
    xn = sa.plant_step(x, u)
    inputs, targets, accepted, _ = sa.observe(x, u, xn)
    assert accepted.cpu().numpy().tolist() == [[1], [1]]
    assert [sa.gp_size(g) for g in range(2)] == [(30 + loop.B, 48)] * 2
    inputs, targets = inputs.cpu().numpy(), targets.cpu().numpy()
    grown, col = [], 0
    for g, (X, y) in enumerate(data):
        d = X.shape[1]
        grown.append((np.vstack([X, inputs[:, col:col + d]]), np.r_[y, targets[:, g]]))
        col += d
    sb = loop.handle(grown, hyp)
    loop.start(sa, sb)
    loop.three_steps()
