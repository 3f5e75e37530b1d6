"""What the GPU tests of the device-side GP updates share (test_gpu_gp_append.py, test_gpu_gp_drop.py,
test_gpu_gp_refactor.py): a BatchSolver (quad2d unless the test names a model) per test file and name,
uploads of the case's data (dicts with X, y, ell, Z, d per GP; sf2 = 1, sn2 = 1e-3), outputs pre-filled with
NaN and followed by 64 sentinels, the unchanged-after-a-refusal check and the closed-loop comparison of two
handles."""

from contextlib import contextmanager

import numpy as np
import pytest

from gp_drop_ref import SF2, SN2
from helpers import initial_states, lqr, problem, product_gps

GUARD = 64
SENTINEL = -7.25e77
REFKEY = dict(mean="mean", var="var", tmean="mean", grad="grad")
QUANT = ("mean", "var", "tmean", "grad")
_SOLVERS: dict = {}


def gpu_torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def solver(owner, key, H=5, B=2, model="quad2d", **kw):
    """The BatchSolver `key` ("A", "B") of the test file `owner` for `model`: no two files share a handle."""
    gpu_torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    if (owner, key, model) not in _SOLVERS:
        _SOLVERS[(owner, key, model)] = BatchSolver(get_spec(model), H, B, **kw)
    return _SOLVERS[(owner, key, model)]


def hyp(dg):
    return dg["ell"], SF2, SN2


def gp_objects(data, rows, hyps=None):
    """GaussianProcess per GP on the given rows (an index array or slice) of the case's data."""
    torch = gpu_torch()
    from gpmpc.gp import GaussianProcess

    gps = []
    for g, dg in enumerate(data):
        gp = GaussianProcess(torch.tensor(dg["X"][rows]), torch.tensor(dg["y"][rows]))
        gp.set_hyperparameters(*(hyp(dg) if hyps is None else hyps[g]))
        gps.append(gp)
    return gps


def upload(s, data, rows, capacity=None, hyps=None):
    """set_gps of the case's data (one dict per GP of the handle's model) on `rows`; `capacity`: one for every GP, or
    one per GP (None: that GP keeps the uploaded size)."""
    assert len(data) == s.spec.n_gp
    s.set_gps(gp_objects(data, rows, hyps))
    if capacity is not None:
        caps = capacity if isinstance(capacity, (tuple, list)) else [capacity] * s.spec.n_gp
        for g in range(s.spec.n_gp):
            if caps[g] is not None:
                s.reserve_gp(g, caps[g])


def guarded(P, dtype=None):
    torch = gpu_torch()
    if dtype is torch.int32:
        t = torch.full((P + GUARD,), -77, dtype=torch.int32, device="cuda")
        t[P:] = -99
        return t
    t = torch.full((P + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    t[P:] = SENTINEL
    return t


def read(t, P, what):
    a = t.cpu().numpy()
    if a.dtype == np.int32:
        assert (a[P:] == -99).all(), f"{what}: wrote past the end of the output"
        assert (a[:P] != -77).all(), f"{what}: output not written"
        return a[:P].copy()
    assert (a[P:] == SENTINEL).all(), f"{what}: wrote past the end of the output"
    assert not np.isnan(a[:P]).any(), f"{what}: {int(np.isnan(a[:P]).sum())} of {P} outputs not written"
    return a[:P].copy()


def outputs(s, g, Z, what):
    """gp_predict mean / predictive variance and gp_mean_grad mean / gradient at Z, guarded."""
    torch = gpu_torch()
    from gpmpc import _lib

    P, d = Z.shape
    Zt = torch.tensor(np.ascontiguousarray(Z), device="cuda")
    mb, vb, gm, gg = guarded(P), guarded(P), guarded(P), guarded(P * d)
    s.gp_predict(g, Zt, with_noise=True, mean=mb, var=vb)
    _lib.check(s.lib.gpmpc_gp_mean_grad(s._h, g, Zt.data_ptr(), P, gm.data_ptr(), gg.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return dict(mean=read(mb, P, what + " mean"), var=read(vb, P, what + " var"),
                tmean=read(gm, P, what + " tile mean"), grad=read(gg, P * d, what + " grad").reshape(P, d))


def nan_block(s, g, d, m, seed):
    """An append of m rows with one NaN target: rejected, so m inert rows."""
    rng = np.random.default_rng(seed)
    Xb, yb = rng.uniform(-1, 1, (m, d)), rng.uniform(0.5, 1.5, m)
    yb[m // 2] = np.nan
    assert s.append_gp(g, Xb, yb).cpu().tolist() == [0]


@contextmanager
def refused(s, g, dg, code, cause, var=True):
    """The body's call on GP g is refused with `code` and a message naming `cause`; the size (which
    the body is given) and the predictions are bit-identical afterwards."""
    torch = gpu_torch()
    from gpmpc import _lib

    Zt = torch.tensor(dg["Z"], device="cuda")

    def snap():
        m, v = s.gp_predict(g, Zt, with_noise=True, var=var)
        tm, tg = s.gp_mean_grad(g, Zt)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (m, v, tm, tg) if t is not None]

    before, size = snap(), s.gp_size(g)
    with pytest.raises(_lib.GPMPCError, match=rf"error {code}: .*{cause}"):
        yield size
    assert s.gp_size(g) == size
    after = snap()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))


class ClosedLoop:
    """quad2d H = 5, B = 8, NLP tolerance 1e-9, QP tolerance 1e-11 (the tight settings of
    test_gpu_launch.py) on n training rows: handle A, which the test updates on the device, against
    handle B, a set_gps of what A should then hold."""

    H, B, tol = 5, 8, 1e-9

    def __init__(self, n):
        self.spec, self.data, self.hyp = problem("quad2d", n)
        self.mats = lqr(self.spec)
        self.x0, self.phase = initial_states(self.spec, self.spec.reference_trajectory(), self.B)

    def handle(self, data, hyp):
        from gpmpc.solver import BatchSolver

        s = BatchSolver(self.spec, self.H, self.B, tol=self.tol, qp_tol=1e-11, qp_max_iter=100)
        s.set_gps(product_gps(data, hyp))
        s.set_tightening(True, 0.95, *self.mats)
        s.reset(reset_iterate=True)
        return s

    def start(self, sa, sb):
        torch = gpu_torch()
        self.s = (sa, sb)
        self.stats = torch.zeros(self.B, sa.STATS_SLOTS, dtype=torch.int64, device="cuda")
        sa.set_stats(self.stats)
        self.obs = [torch.tensor(self.x0, device="cuda"), torch.tensor(self.x0, device="cuda")]
        self.ts = [torch.tensor(self.phase, dtype=torch.int32, device="cuda") for _ in range(2)]

    def step(self, i):
        s = self.s[i]
        u = s.solve(self.obs[i], self.ts[i].clone())
        out = dict(st=s.status.cpu().numpy(), it=s.sqp_iter.cpu().numpy())
        out["x"], out["u"], _ = (t.cpu().numpy() for t in s.solution())
        self.obs[i] = s.plant_step(self.obs[i], u.clone(), self.ts[i])
        return out

    def three_steps(self):
        """Three closed-loop steps each (solve, plant_step): identical statuses; x, u and variance()
        agree within 1e-6 (1 + |.|).  Step 0 follows A's update (and the reset), so it computes its
        first linearisation (stats slot 9 advances by sqp_iter + 1); steps 1, 2 read the cache."""
        def close(a, b):
            return float((np.abs(a - b) / (1 + np.abs(b))).max())

        sa, sb = self.s
        self.lin_prev = self.stats[:, 9].clone()
        for k in range(3):
            ra, rb = self.step(0), self.step(1)
            np.testing.assert_array_equal(ra["st"], rb["st"])
            assert np.isin(ra["st"], (0, 2)).all(), ra["st"]
            assert close(ra["x"], rb["x"]) <= 1e-6 and close(ra["u"], rb["u"]) <= 1e-6, (k, close(ra["x"], rb["x"]))
            if k > 0:   # (the first step after a reset runs no variance launch)
                va, vb = sa.variance().cpu().numpy(), sb.variance().cpu().numpy()
                assert close(va, vb) <= 1e-6, (k, close(va, vb))
            lin = self.stats[:, 9].clone()
            d = (lin - self.lin_prev).cpu().numpy()
            np.testing.assert_array_equal(d, ra["it"] + (1 if k == 0 else 0))
            self.lin_prev = lin

    def step_after_update(self):
        """A step of handle A that follows another update: the cache served nothing computed with the old model."""
        ra = self.step(0)
        d = (self.stats[:, 9] - self.lin_prev).cpu().numpy()
        assert (d > 0).all()
        np.testing.assert_array_equal(d, ra["it"] + 1)
