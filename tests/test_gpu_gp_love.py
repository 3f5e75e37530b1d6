"""Building the LOVE variance root on the device (gpmpc_gp_love_root, gpmpc_get_gp_variance_root;
csrc/gp_love.hip), MI355X only.

The reference is the host root, ``GaussianProcess.love_root(rank, seed)`` (or
``oracle.lanczos_love_root`` on the live rows where some are inert), from the same start vector.  The
two roots differ by an orthogonal factor (the device takes the bidiagonal Cholesky factor of the
Lanczos matrix, the host its eigendecomposition), so they are compared where a root is used:
``oracle.love_var`` at 64 points near the training rows (row + N(0, 0.1^2)) and 64 points drawn
N(0, 0.5^2), to 1e-9 sf2, the bar of test_gpu_love.py and test_love_cpu.py.  Every figure is printed
before it is asserted (run with -s).
"""

from contextlib import contextmanager
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import gp_update_util as U
from helpers import O, initial_states, lqr, oracle_gps, problem, product_gps

pytestmark = pytest.mark.gpu

H, B = 8, 4
TOL = 1e-9          # x sf2: the project's LOVE bar
_torch = U.gpu_torch
_SOLVERS: dict = {}


@lru_cache(maxsize=None)
def _case(name, N):
    spec, data, hyp = problem(name, N)
    data = [(np.asarray(X, dtype=np.float64).reshape(N, -1), np.asarray(y, dtype=np.float64)) for X, y in data]
    return spec, data, hyp


def _solver(name):
    _torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    if name not in _SOLVERS:
        _SOLVERS[name] = BatchSolver(get_spec(name), H, B)
    return _SOLVERS[name]


def _start(n, seed=0):
    """The draw of GaussianProcess.love_root(seed=seed)."""
    torch = _torch()
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randn(n, dtype=torch.float64, generator=gen).numpy()


def _points(X, seed=5):
    rng = np.random.default_rng(seed)
    N, d = X.shape
    near = X[rng.integers(0, N, 64)] + rng.normal(scale=0.1, size=(64, d))
    return dict(near=near, far=rng.normal(scale=0.5, size=(64, d)))


def _var_errors(og, R_dev, R_host, what):
    """max |love_var(device root) - love_var(host root)| / sf2 per point set, printed."""
    out = {}
    for k, Z in _points(og.X).items():
        out[k] = float(np.abs(O.love_var(og, R_dev, Z) - O.love_var(og, R_host, Z)).max()) / og.sf2
        print(f"[gp-love] {what} {k}: variance error {out[k]:.3e} sf2 (bound {TOL:g})")
    return out


def _upload(s, name, N, rows=None, capacity=None, **kw):
    spec, data, hyp = _case(name, N)
    rows = slice(0, N) if rows is None else rows
    gpp = product_gps([(X[rows], y[rows]) for X, y in data], hyp)
    s.set_gps(gpp, **kw)
    if capacity is not None:
        for g in range(spec.n_gp):
            s.reserve_gp(g, capacity)
    return gpp


PARITY = [("quad2d", 40, 8), ("quad2d", 48, 20), ("quad2d", 200, 50), ("cartpole", 50, 100)]


@pytest.mark.parametrize("name,N,rank", PARITY)
def test_device_root_matches_the_host_root(name, N, rank):
    spec, data, hyp = _case(name, N)
    s = _solver(name)
    gpp = _upload(s, name, N, capacity=N, variance="exact")
    ogs = oracle_gps(data, hyp)
    cap = min(rank, N)
    for g, og in enumerate(ogs):
        assert s.love_ranks[g] is None
        R_host = gpp[g].love_root(rank, seed=0).numpy()
        m, ok = s.love_root_gp(g, rank, seed=0)
        R = s.love_roots[g]
        print(f"[gp-love] {name} N={N} rank={rank} gp{g}: device rank {m}, host rank {R_host.shape[1]}, ok {ok}")
        assert ok == 1 and s.love_ranks[g] == m and R.shape == (N, m)
        assert abs(m - R_host.shape[1]) <= 1 and m <= cap
        if R_host.shape[1] == cap:   # no breakdown: the cap itself
            assert m == cap
        err = _var_errors(og, R, R_host, f"{name} N={N} rank={rank} gp{g}")
        ortho = float(np.abs(R.T @ og.K @ R - np.eye(m)).max())
        print(f"[gp-love] {name} N={N} rank={rank} gp{g}: |R^T K R - I| {ortho:.3e} (bound 1e-8)")
        assert max(err.values()) <= TOL, (g, err)
        assert ortho <= 1e-8, (g, ortho)
    if (name, N) == ("quad2d", 48):   # the 1-D thrust GP breaks down near 12, the pitch GP runs to the cap
        assert s.love_ranks[0] < 20 and s.love_ranks[1] == 20, s.love_ranks


def test_device_root_at_the_love_switch_size():
    """quad2d N = 1000, rank 100 (bench config 4, just past the 800-row switch): the near-row points are
    held to the bar; the far set, where the broken-down thrust GP's variance moves by about 2e-9 sf2 under
    rounding-sized perturbations of the host algorithm itself, is reported only."""
    name, N, rank = "quad2d", 1000, 100
    spec, data, hyp = _case(name, N)
    s = _solver(name)
    gpp = _upload(s, name, N, capacity=N, variance="exact")
    ogs = oracle_gps(data, hyp)
    for g, og in enumerate(ogs):
        R_host = gpp[g].love_root(rank, seed=0).numpy()
        m, ok = s.love_root_gp(g, rank, seed=0)
        print(f"[gp-love] {name} N={N} rank={rank} gp{g}: device rank {m}, host rank {R_host.shape[1]}, ok {ok}")
        assert ok == 1 and abs(m - R_host.shape[1]) <= 1
        if R_host.shape[1] == rank:
            assert m == rank
        err = _var_errors(og, s.love_roots[g], R_host, f"{name} N={N} rank={rank} gp{g}")
        assert err["near"] <= TOL, (g, err)


def test_installed_root_drives_the_tightening_variance():
    """The root is installed in the layout gp_love_kernel reads, pad16(m) stride included (ranks ~12 and 20:
    strides 16 and 32): variance() of a solve against oracle.love_var with the read-back root at the
    previous solution."""
    torch = _torch()
    name, N, rank = "quad2d", 48, 20
    spec, data, hyp = _case(name, N)
    s = _solver(name)
    _upload(s, name, N, capacity=N, variance="exact")
    for g in range(spec.n_gp):
        assert s.love_root_gp(g, rank, seed=0)[1] == 1
    s.set_tightening(True, 0.95, *lqr(spec))
    s.reset(reset_iterate=True)
    x0, ph = initial_states(spec, spec.reference_trajectory(), B, seed=1)
    obs = torch.tensor(x0, device="cuda")
    ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
    u = s.solve(obs, ts)                          # first step: no previous solution, no variance
    xs, us, _ = (t.cpu().numpy() for t in s.solution())
    s.plant_step(obs, u, ts, out=obs)
    s.solve(obs, ts)                              # variance launch at (xs, us)
    var = s.variance().cpu().numpy()
    z = np.concatenate([xs[:, :-1, :], us], axis=2).reshape(B * H, -1)
    for g, og in enumerate(oracle_gps(data, hyp)):
        ref = O.love_var(og, s.variance_root(g), z[:, spec.var_inputs[g]])
        err = float(np.abs(var[:, :, g].reshape(-1) - ref).max()) / og.sf2
        print(f"[gp-love] in the solve gp{g} (rank {s.love_ranks[g]}): variance error {err:.3e} sf2 (bound {TOL:g})")
        assert err <= TOL, (g, err)
    s.set_tightening(False)


def _live_parity(s, g, X_all, inert, hyp_g, rank, q0, what):
    """The read-back root of GP g (rows X_all, some inert) against the host root of the live rows,
    scattered back; exact zeros at the inert rows."""
    n = X_all.shape[0]
    live = np.flatnonzero(~inert)
    og_live = O.ExactGP(X_all[live], np.zeros(live.size), *hyp_g)
    R_l = O.lanczos_love_root(og_live.K, rank, q0[live])
    R = s.variance_root(g)
    assert R.shape[0] == n and abs(R.shape[1] - R_l.shape[1]) <= 1
    assert (R[inert] == 0.0).all(), what
    R_h = np.zeros((n, R_l.shape[1]))
    R_h[live] = R_l
    og = SimpleNamespace(X=X_all, ell=hyp_g[0], sf2=hyp_g[1], sn2=hyp_g[2])
    err = {}
    for k, Z in _points(X_all[live]).items():
        err[k] = float(np.abs(O.love_var(og, R, Z) - O.love_var(og, R_h, Z)).max()) / og.sf2
        print(f"[gp-love] {what} {k}: variance error {err[k]:.3e} sf2 (bound {TOL:g})")
    assert max(err.values()) <= TOL, (what, err)


def test_inert_rows_and_learning():
    """N = 40 at capacity 96: a rejected (inert) block and a good one appended; the root from a start
    vector that is NaN at the inert rows; the updates refuse while it is installed and go through after
    drop_love_root, and the rebuilt root matches again."""
    torch = _torch()
    from gpmpc import _lib

    name, rank = "quad2d", 20
    spec, data, hyp = _case(name, 56)
    s = _solver(name)
    _upload(s, name, 56, rows=slice(0, 40), capacity=96, variance="exact")
    for g, (X, y) in enumerate(data):
        d = X.shape[1]
        U.nan_block(s, g, d, 16, seed=70 + g)                                      # rows 40 .. 55: inert
        assert s.append_gp(g, X[40:56], y[40:56]).cpu().tolist() == [1]             # rows 56 .. 71
        assert s.gp_size(g) == (72, 96)
        X_all = np.vstack([X[:40], np.zeros((16, d)), X[40:56]])
        inert = np.zeros(72, dtype=bool)
        inert[40:56] = True
        q0 = _start(72)
        qn = q0.copy()
        qn[inert] = np.nan
        m, ok = s.love_root_gp(g, rank, start=qn)
        assert ok == 1 and s.love_ranks[g] == m
        _live_parity(s, g, X_all, inert, hyp[g], rank, q0, f"inert rows gp{g}")
        # installed: the updates refuse as before, with the root and the GP unchanged
        R0 = s.variance_root(g)
        yt = torch.tensor(np.r_[y[:40], np.zeros(16), y[40:56]], device="cuda")
        for call in (lambda: s.append_gp(g, X[:4], y[:4]), lambda: s.drop_gp(g, 16),
                     lambda: s.refactor_gp(g, yt, *hyp[g])):
            with pytest.raises(_lib.GPMPCError, match=r"error -3: .*LOVE root"):
                call()
        assert s.gp_size(g) == (72, 96) and np.array_equal(s.variance_root(g), R0)
        # dropped: the update goes through, and the root is rebuilt for what the GP holds now
        s.drop_love_root(g)
        assert s.love_ranks[g] is None and s.love_roots[g] is None
        with pytest.raises(_lib.GPMPCError, match=r"error -3: no LOVE root"):
            s.variance_root(g)
        assert s.drop_gp(g, 16).cpu().tolist() == [1]
        assert s.gp_size(g) == (56, 96)
        q1 = _start(56, seed=3)
        qn = q1.copy()
        qn[inert[16:]] = np.nan
        m, ok = s.love_root_gp(g, rank, start=qn)
        assert ok == 1
        _live_parity(s, g, X_all[16:], inert[16:], hyp[g], rank, q1, f"after a drop gp{g}")


def test_two_calls_give_the_same_bits():
    name, N, rank = "quad2d", 200, 50
    s = _solver(name)
    _upload(s, name, N, capacity=N + 24, variance="exact")
    for g in range(2):
        first = s.love_root_gp(g, rank, seed=4)
        R1 = s.love_roots[g].copy()
        assert s.love_root_gp(g, 8, seed=9)[1] == 1      # other contents in the scratch in between
        assert s.love_root_gp(g, rank, seed=4) == first
        assert np.array_equal(s.love_roots[g], R1)


@contextmanager
def _refused(s, g, Z, code, cause, var=True):
    """The body's call on GP g is refused with `code` and a message naming `cause`; the size, the
    predictions and the installed root (or its absence) are the same afterwards, bit for bit."""
    torch = _torch()
    from gpmpc import _lib

    Zt = torch.tensor(Z, device="cuda")

    def snap():
        try:
            root = s.variance_root(g)
        except _lib.GPMPCError as e:
            assert "error -3: no LOVE root" in str(e)
            root = None
        mean, v = s.gp_predict(g, Zt, with_noise=True, var=var)
        torch.cuda.synchronize()
        return root, mean.cpu().numpy(), None if v is None else v.cpu().numpy(), s.gp_size(g)

    before = snap()
    with pytest.raises(_lib.GPMPCError, match=rf"error {code}: .*{cause}"):
        yield
    after = snap()
    for a, b in zip(before, after):
        assert (a is None and b is None) or np.array_equal(a, b) or a == b


def test_refusals_leave_the_handle_unchanged():
    torch = _torch()
    from gpmpc import _lib

    name, N = "quad2d", 40
    spec, data, hyp = _case(name, N)
    s = _solver(name)
    r, ok = _lib.ctypes.c_int32(-5), _lib.ctypes.c_int32(-5)

    def call(g, rank, q0):
        _lib.check(s.lib.gpmpc_gp_love_root(s._h, g, rank, None if q0 is None else q0.data_ptr(),
                                            _lib.ctypes.byref(r), _lib.ctypes.byref(ok), s._stream()))

    q0 = torch.tensor(_start(N), device="cuda")
    Zs = [_points(X)["near"] for X, _ in data]
    gpp = _upload(s, name, N, variance="exact")
    for g in range(2):
        with _refused(s, g, Zs[g], -3, "gpmpc_gp_reserve"):   # no scratch, no second factor buffer yet
            call(g, 8, q0)
        s.reserve_gp(g, N)
        assert s.love_root_gp(g, 8, seed=0)[1] == 1           # a root to keep
        with _refused(s, g, Zs[g], -1, "start vector"):
            call(g, 8, None)
        for bad in (0, 257, -1):
            with _refused(s, g, Zs[g], -1, "rank"):
                call(g, bad, q0)
    # no Linv
    s.set_gps(gpp, with_variance=False)
    for g in range(2):
        s.reserve_gp(g, N)
        with _refused(s, g, Zs[g], -3, "Linv", var=False):
            call(g, 8, q0)
    # a FITC upload, with the host's root installed
    s.set_gps(gpp, fitc=[(X[:8], np.linspace(0.5, 1.5, 8)) for X, _ in data], variance="love", love_rank=8,
              love_force=True)
    for g in range(2):
        with _refused(s, g, Zs[g], -3, "FITC"):
            call(g, 8, q0)
    assert (r.value, ok.value) == (-5, -5)                    # no refusal wrote the outputs
    # a GP that was never set; the getter's own refusals
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    fresh = BatchSolver(get_spec(name), 5, 2)
    with pytest.raises(_lib.GPMPCError, match=r"error -3: GP not set"):
        _lib.check(fresh.lib.gpmpc_gp_love_root(fresh._h, 0, 8, q0.data_ptr(), None, None, fresh._stream()))
    with pytest.raises(_lib.GPMPCError, match=r"error -3: no LOVE root"):
        _lib.check(fresh.lib.gpmpc_get_gp_variance_root(fresh._h, 0, None, None, None, None))


def test_gpmpc_keeps_learning_past_the_love_switch():
    """quad2d on 808 training rows, room for 840, variance="love": append_data (with and without
    eviction) goes through with the roots rebuilt on the device, the next steps solve, and the tightening
    variances are those of the read-back roots."""
    torch = _torch()
    from gpmpc.gpmpc import GPMPC

    N0 = 808
    spec, data, hyp = _case("quad2d", N0 + 48)
    ctrl = GPMPC("quad2d", horizon=H, batch=B, gp_capacity=840, variance="love")
    ctrl.set_gaussian_processes(product_gps([(X[:N0], y[:N0]) for X, y in data], hyp))
    ctrl.reset()
    s = ctrl.solver
    assert all(r is not None for r in s.love_ranks), s.love_ranks

    def block(a, b):
        return np.hstack([X[a:b] for X, _ in data]), np.column_stack([y[a:b] for _, y in data])

    flags = ctrl.append_data(*block(N0, N0 + 16))
    assert all(f.cpu().tolist() == [1] for f in flags)
    assert [s.gp_size(g) for g in range(2)] == [(N0 + 16, 840)] * 2
    assert all(r is not None for r in s.love_ranks), s.love_ranks
    flags = ctrl.append_data(*block(N0 + 16, N0 + 48), evict_oldest=True)      # 824 + 32 > 840: drops 16
    assert all(f.cpu().tolist() == [1, 1] for f in flags)
    assert [s.gp_size(g) for g in range(2)] == [(840, 840)] * 2
    assert all(r is not None for r in s.love_ranks), s.love_ranks
    x0, _ = initial_states(spec, spec.reference_trajectory(), B, seed=1)
    obs = torch.tensor(x0, device="cuda")
    u = ctrl.select_action_batch(obs)
    assert (s.status.cpu().numpy() == 0).all(), s.status
    xs, us, _ = (t.cpu().numpy() for t in s.solution())
    s.plant_step(obs, u, out=obs)
    ctrl.select_action_batch(obs)
    assert (s.status.cpu().numpy() == 0).all(), s.status
    var = s.variance().cpu().numpy()
    z = np.concatenate([xs[:, :-1, :], us], axis=2).reshape(B * H, -1)
    for g, gp in enumerate(ctrl.gaussian_process):
        Xg = gp.train_inputs[0].cpu().numpy()
        assert np.array_equal(Xg, data[g][0][16:N0 + 48])
        og = SimpleNamespace(X=Xg, ell=hyp[g][0], sf2=hyp[g][1], sn2=hyp[g][2])
        ref = O.love_var(og, s.variance_root(g), z[:, spec.var_inputs[g]])
        err = float(np.abs(var[:, :, g].reshape(-1) - ref).max()) / og.sf2
        print(f"[gp-love] GPMPC gp{g} (rank {s.love_ranks[g]}): tightening variance error {err:.3e} sf2 (bound {TOL:g})")
        assert err <= TOL, (g, err)
