"""gpmpc_rollout_sample on the MI355X: closed-loop samples of the learned model's future.

Cases (the smallest sizes at which the kernel can go wrong; inputs as in test_gpu_rollout.py):
  a  quad2d,   17 training rows (two column tiles, the second ragged),      P = 3,  T = 4
  b  quad2d,   200 rows (13 column tiles),                                  P = 33, T = 6 (crosses a 16-trajectory tile)
  c  cartpole, 50 rows (both GPs state-dependent),                          P = 16, T = 5
  d  quad3d,   60 rows, FITC mean over 24 inducing rows, exact variance,    P = 17, T = 4
  e  quad2d,   272 rows (17 column tiles: the first size past one group),   P = 2,  T = 2
Every case draws xi from default_rng, takes the spec's LQR gain as K, its own plain rollout as xref and clips, with the
upper bound of input 0 lowered to u_eq[0] + 0.05 in its handle so that the clip acts; the likelihood noise is in the
draw.  Each case's handle, inputs and results are computed once and shared."""

import ctypes
import functools

import numpy as np
import pytest

import gp_update_util as U
import rollout_ref as RR
import rollout_sample_ref as SR
from helpers import fitc_oracle_gps, fitc_weights, initial_states, lqr, oracle_gps, problem, product_gps

pytestmark = pytest.mark.gpu

CASES = {"a": ("quad2d", 17, 3, 4, None), "b": ("quad2d", 200, 33, 6, None), "c": ("cartpole", 50, 16, 5, None),
         "d": ("quad3d", 60, 17, 4, 24), "e": ("quad2d", 272, 2, 2, None)}


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def sample(s, x0, u, xref=None, K=None, clip=False, xi=None, with_gp=True, with_noise=True, var=True):
    """BatchSolver.rollout_sample on numpy arrays: dict of numpy arrays."""
    torch = U.gpu_torch()

    def t(a):
        return None if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda")

    out = s.rollout_sample(t(x0), t(u), xref=t(xref), K=K, clip=clip, xi=t(xi), with_gp=with_gp, with_noise=with_noise,
                           var=var)
    return {k: v.cpu().numpy() for k, v in out.items()}


def plain(s, x0, u, with_gp=True):
    torch = U.gpu_torch()
    return s.rollout(torch.tensor(np.ascontiguousarray(x0), device="cuda"), torch.tensor(np.ascontiguousarray(u), device="cuda"),
                     with_gp=with_gp).cpu().numpy()


class Case:
    def __init__(self, key):
        U.gpu_torch()
        name, N, self.P, self.T, M = CASES[key]
        spec, self.data, self.hyp = problem(name, N)
        self.spec = spec.copy()
        self.spec.u_hi = np.array(spec.u_hi, dtype=np.float64)
        self.spec.u_hi[0] = spec.u_eq[0] + 0.05
        self.gpp = product_gps(self.data, self.hyp)
        self.exact = oracle_gps(self.data, self.hyp)               # the variance's GPs
        self.fitc = fitc_weights(self.gpp, M) if M else None
        self.gpo = oracle_gps(self.data, self.hyp)                 # the mean's GPs
        if self.fitc is not None:
            self.gpo = fitc_oracle_gps(self.gpo, self.fitc)
        self.K = np.ascontiguousarray(lqr(spec)[2])
        self.x0, _ = initial_states(spec, spec.reference_trajectory(), self.P)
        rng = np.random.default_rng(100 + N)
        self.u = spec.u_eq + 0.1 * rng.standard_normal((self.P, self.T, spec.nu))
        self.xi = np.random.default_rng(300 + N).standard_normal((self.P, self.T, spec.n_gp))
        self.s = self.handle()

    def handle(self, **kw):
        from gpmpc.solver import BatchSolver

        s = BatchSolver(self.spec, 5, 2)
        s.set_gps(self.gpp, fitc=self.fitc, **kw)
        return s

    @functools.lru_cache(maxsize=None)
    def plain(self, with_gp=True):
        x = plain(self.s, self.x0, self.u, with_gp)
        x.setflags(write=False)
        return x

    def call(self, s=None, **kw):
        """The case's call (the feedback around the plain rollout, the clip, the draws), with changes."""
        args = dict(x0=self.x0, u=self.u, xref=self.plain(), K=self.K, clip=True, xi=self.xi)
        args.update(kw)
        return sample(self.s if s is None else s, **args)

    @functools.lru_cache(maxsize=None)
    def run(self):
        out = self.call()
        for a in out.values():
            a.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def case(key):
    return Case(key)


def step_bound(c, ref, e):
    """test_gpu_rollout.py's one-step bound with the disturbance added to the scale."""
    scale = sum(gp.sf2 * np.abs(gp.alpha).sum() for gp in c.gpo)
    return 1e-10 * (1.0 + np.abs(ref) + c.spec.dt * (scale + np.abs(e).sum(axis=-1, keepdims=True)))


def check_against_reference(c, out, what):
    """The applied inputs against the numpy feedback and clip of the GPU's own states, every state against the
    reference step from (x_gpu[k], u_gpu[k]) with the draw formed from the GPU's own variance, and the variance against
    the oracle's at the applied points.  Returns the reference steps and their bounds."""
    spec = c.spec
    x, ua, v = out["x"], out["u"], out["var"]
    xref = c.plain()
    assert x.shape == (c.P, c.T + 1, spec.nx) and ua.shape == c.u.shape and v.shape == (c.P, c.T, spec.n_gp)
    assert same(x[:, 0], c.x0) and np.isfinite(x).all() and np.isfinite(ua).all() and np.isfinite(v).all()
    refs, bounds = [], []
    for k in range(c.T):
        uk = SR.applied_input(spec, x[:, k], c.u[:, k], xref[:, k], c.K, clip=True)
        eu = np.abs(ua[:, k] - uk) / (1.0 + np.abs(uk))
        assert (eu <= 1e-13).all(), (what, k, float(eu.max()))
        e = SR.draws(c.exact, v[:, k], c.xi[:, k], with_noise=True)
        ref = SR.one_step(spec, c.gpo, x[:, k], ua[:, k], e)
        bound = step_bound(c, ref, e)
        err = np.abs(x[:, k + 1] - ref)
        assert (err <= bound).all(), (what, k, float((err / bound).max()))
        refs.append(ref)
        bounds.append(bound)
    refs, bounds = np.stack(refs, axis=1), np.stack(bounds, axis=1)
    err = np.abs(x[:, 1:] - refs)
    want = RR.variances(spec, c.exact, x, ua)
    ev = np.abs(v - want) / np.array([gp.sf2 for gp in c.exact])
    print(f"[rollout_sample] {what}: max state err / bound {(err / bounds).max():.3e}, smallest bound {bounds.min():.3e}, "
          f"max |var - oracle| / sf2 {ev.max():.3e}")
    assert (ev <= 1e-9).all(), (what, float(ev.max()))
    return refs, bounds


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("key", list(CASES))
def test_one_step_parity_with_the_reference_from_the_gpus_own_states(key):
    c = case(key)
    out = c.run()
    refs, bounds = check_against_reference(c, out, f"case {key}")
    # the disturbance matters: without the draws the same call misses the bound
    calm = c.call(xi=None)
    assert same(calm["x"][:, 0], c.x0)
    assert not (np.abs(calm["x"][:, 1:] - refs) <= bounds).all()
    # and so does the feedback: step 0 applies the clipped nominal input (x_0 - xref_0 is an exact zero), later steps do not
    assert same(out["u"][:, 0], np.clip(c.u[:, 0], c.spec.u_lo, c.spec.u_hi))
    assert not same(out["u"][:, 1:], np.clip(c.u[:, 1:], c.spec.u_lo, c.spec.u_hi))
    if key == "b":
        hi = c.spec.u_hi[0]
        clipped = out["u"][..., 0] == hi
        print(f"[rollout_sample] case b: {int(clipped.sum())} of {clipped.size} applied inputs sit on the lowered bound {hi}")
        assert clipped.any() and (out["u"][..., 0] <= hi).all()
        free = c.call(clip=False)
        assert (free["u"][..., 0] > hi).any()   # (without the clip the same call exceeds it)


# ------------------------------------------------------------------------------------------------ 2
def _predicted_variances(s, spec, x, u):
    torch = U.gpu_torch()
    out = []
    for g, Z in enumerate(RR.gp_points(spec, x, u)):
        Zt = torch.tensor(np.ascontiguousarray(Z.reshape(-1, Z.shape[-1])), device="cuda")
        out.append(s.gp_predict(g, Zt, with_noise=False, mean=False)[1].cpu().numpy().reshape(Z.shape[:2]))
    return np.stack(out, axis=-1)


@pytest.mark.parametrize("key", list(CASES))
def test_variance_is_the_exact_one_at_the_applied_points(key):
    c = case(key)
    out = c.run()
    sf2 = np.array([gp.sf2 for gp in c.exact])
    want = RR.variances(c.spec, c.exact, out["x"], out["u"])
    pred = _predicted_variances(c.s, c.spec, out["x"], out["u"])
    e1, e2 = np.abs(out["var"] - want) / sf2, np.abs(out["var"] - pred) / sf2
    print(f"[rollout_sample] case {key}: |var - oracle| / sf2 {e1.max():.3e}, |var - gp_predict| / sf2 {e2.max():.3e}, "
          f"var in [{out['var'].min():.3e}, {out['var'].max():.3e}]")
    assert (e1 <= 1e-9).all() and (e2 <= 1e-9).all()
    # the points are the applied ones: at the nominal inputs the variance of the GP that reads input 0 is another
    nominal = RR.variances(c.spec, c.exact, out["x"], c.u)
    assert not (np.abs(out["var"] - nominal) / sf2 <= 1e-9).all()
    # the variance alone (no draws), and along a prior rollout
    for with_gp in (True, False):
        alone = c.call(xi=None, K=None, xref=None, clip=False, with_gp=with_gp)
        assert same(alone["x"], c.plain(with_gp)) and same(alone["u"], c.u)
        w = RR.variances(c.spec, c.exact, alone["x"], c.u)
        assert (np.abs(alone["var"] - w) / sf2 <= 1e-9).all()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("key", ("a", "c", "d", "e"))
@pytest.mark.parametrize("with_gp", (True, False))
def test_without_draws_feedback_and_clip_it_is_the_plain_rollout_bit_for_bit(key, with_gp):
    c = case(key)
    want = c.plain(with_gp)
    bare = c.call(xi=None, K=None, xref=None, clip=False, with_gp=with_gp, var=False)
    assert same(bare["x"], want) and same(bare["u"], c.u) and "var" not in bare
    # a gain around that very rollout adds exact zeros
    fb = c.call(xi=None, xref=want, clip=False, with_gp=with_gp, var=False)
    assert same(fb["x"], want) and same(fb["u"], c.u)
    # (and around another reference it does not)
    moved = c.call(xi=None, xref=want + 0.01, clip=False, with_gp=with_gp, var=False)
    assert not same(moved["x"], want) and not same(moved["u"], c.u)


def test_prior_with_draws_is_the_reference_with_the_draw_as_the_mean():
    """with_gp = 0: the value passed to f is e_g alone."""
    c = case("a")
    out = c.call(with_gp=False, xref=c.plain(False))
    x, ua, v = out["x"], out["u"], out["var"]
    for k in range(c.T):
        e = SR.draws(c.exact, v[:, k], c.xi[:, k], with_noise=True)
        ref = SR.one_step(c.spec, None, x[:, k], ua[:, k], e)
        assert (np.abs(x[:, k + 1] - ref) <= 1e-10 * (1.0 + np.abs(ref) + c.spec.dt * np.abs(e).sum(axis=-1, keepdims=True))).all()
    assert not same(x, c.run()["x"]) and not same(x, c.plain(False))


# ------------------------------------------------------------------------------------------------ 4
def test_independence_of_the_batch_and_prefixes_bit_for_bit():
    c = case("b")
    full = c.run()
    xref = c.plain()
    for i in (5, 20, 32):   # (slot 5 of tile 0, slot 4 of tile 1, the lone trajectory of tile 2)
        alone = c.call(x0=c.x0[i:i + 1], u=c.u[i:i + 1], xref=xref[i:i + 1], xi=c.xi[i:i + 1])
        j = np.r_[0:32, i]
        last = c.call(x0=c.x0[j], u=c.u[j], xref=xref[j], xi=c.xi[j])
        for k in ("x", "u", "var"):
            assert same(alone[k][0], full[k][i]), (i, k)
            assert same(last[k][32], full[k][i]) and same(last[k][:32], full[k][:32]), (i, k)
    head = c.call(u=c.u[:, :2], xref=xref[:, :3], xi=c.xi[:, :2])
    assert same(head["x"], full["x"][:, :3]) and same(head["u"], full["u"][:, :2]) and same(head["var"], full["var"][:, :2])
    again = c.call()
    assert all(same(again[k], full[k]) for k in ("x", "u", "var"))


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("where", ("xi", "xref"))
def test_a_nan_stays_in_its_trajectory(where):
    c = case("b")
    clean = c.run()
    i = 5
    if where == "xi":
        xi = c.xi.copy()
        xi[i, 3] = np.nan
        out, first = c.call(xi=xi), 4          # the draw of step 3 reaches row 4
    else:
        xref = c.plain().copy()
        xref[i, 2] = np.nan
        out, first = c.call(xref=xref), 3      # the input of step 2 reaches row 3
    assert (~np.isfinite(out["x"][i, first:])).any(axis=-1).all()
    assert same(out["x"][i, :first], clean["x"][i, :first])
    nu = first - 1 if where == "xref" else first          # applied inputs before the poisoned step
    assert same(out["u"][i, :nu], clean["u"][i, :nu]) and same(out["var"][i, :nu], clean["var"][i, :nu])
    if where == "xref":
        assert np.isnan(out["u"][i, 2]).all()             # the clip leaves the NaN a NaN
    others = np.arange(c.P) != i
    assert all(same(out[k][others], clean[k][others]) for k in ("x", "u", "var"))


# ------------------------------------------------------------------------------------------------ 6
def test_inert_rows_stay_inert():
    """After a rejected append block (a NaN target: 16 inert rows, a third column tile) the results are those of the
    handle uploaded without the block, to the bounds of the reference comparison."""
    c = case("a")
    s = c.handle()
    for g in range(c.spec.n_gp):
        s.reserve_gp(g, 48)
        U.nan_block(s, g, c.spec.gp_dims[g], 16, seed=40 + g)
        assert s.gp_size(g)[0] == 33
    out = c.call(s)
    check_against_reference(c, out, "case a behind an inert block")
    clean = c.run()
    assert (np.abs(out["u"] - clean["u"]) <= 1e-13 * (1.0 + np.abs(clean["u"]))).all()
    assert (np.abs(out["var"] - clean["var"]) <= 1e-9 * np.array([gp.sf2 for gp in c.exact])).all()


def test_a_love_root_is_ignored():
    c = case("d")
    s = c.handle(variance="love", love_force=True, love_rank=8)
    assert all(r is not None for r in s.love_ranks)
    out, clean = c.call(s), c.run()
    assert all(same(out[k], clean[k]) for k in ("x", "u", "var"))


# ------------------------------------------------------------------------------------------------ 7
def test_the_call_waits_for_the_handles_last_call_on_another_stream():
    """A delay and a gpmpc_gp_refactor of GP 1 at a scaled lengthscale on stream A, then the call: when it returns the
    delay has ended, and its outputs are those of the serial run behind the refactorisation."""
    from gpmpc import _lib
    from gpmpc.solver import BatchSolver
    from stream_order_util import DELAY_FLOOR_MS, Delay

    torch = U.gpu_torch()
    g, P, T = 1, 20, 3
    spec, data, hyp = problem("quad2d", 28)
    ell, sf2, sn2 = hyp[g]
    y = torch.tensor(data[g][1], device="cuda")
    ok = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    x0, _ = initial_states(spec, spec.reference_trajectory(), P)
    rng = np.random.default_rng(9)
    u = spec.u_eq + 0.1 * rng.standard_normal((P, T, spec.nu))
    xi = rng.standard_normal((P, T, spec.n_gp))
    K = np.ascontiguousarray(lqr(spec)[2])

    def handle():
        s = BatchSolver(spec, 5, 2)
        s.set_gps(product_gps(data, hyp))
        for k in range(spec.n_gp):
            s.reserve_gp(k, 32)
        return s

    def refactor(s, stream):
        _lib.check(s.lib.gpmpc_gp_refactor(s._h, g, y.data_ptr(), 1.3 * ell, sf2, sn2, ok.data_ptr(), stream))

    s = handle()
    xref = plain(s, x0, u) + 0.01
    args = dict(x0=x0, u=u, xref=xref, K=K, clip=True, xi=xi)
    before = sample(s, **args)
    refactor(s, s._stream())
    torch.cuda.synchronize()
    serial = sample(s, **args)
    assert ok.cpu().tolist() == [1]
    assert not same(serial["x"], before["x"]) and not same(serial["var"], before["var"])
    # the same on two streams: everything staged, then the delay, the writer and the call with no synchronise between
    s = handle()
    A, delay = torch.cuda.Stream(), Delay(torch)
    x0t, ut, xrt, xit = (torch.tensor(a, device="cuda") for a in (x0, u, xref, xi))
    xo = torch.full((P, T + 1, spec.nx), float("nan"), dtype=torch.float64, device="cuda")
    uo = torch.full((P, T, spec.nu), float("nan"), dtype=torch.float64, device="cuda")
    vo = torch.full((P, T, spec.n_gp), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    delay.queue(A, DELAY_FLOOR_MS)
    end = torch.cuda.Event()
    end.record(A)
    refactor(s, A.cuda_stream)
    pending = not end.query()
    status = s.lib.gpmpc_rollout_sample(s._h, P, T, x0t.data_ptr(), ut.data_ptr(), xrt.data_ptr(), K.ctypes.data, 1,
                                        xit.data_ptr(), 1, 1, xo.data_ptr(), uo.data_ptr(), vo.data_ptr())
    done = end.query()
    got = dict(x=xo.cpu().numpy(), u=uo.cpu().numpy(), var=vo.cpu().numpy())   # (the call returned with its work completed)
    torch.cuda.synchronize()
    _lib.check(status)
    assert pending, "the delay had ended before the call was made: it showed nothing"
    assert done, "the call returned while the delay ahead of the refactorisation still ran: it did not wait"
    assert all(same(got[k], serial[k]) for k in ("x", "u", "var"))


# ------------------------------------------------------------------------------------------------ 8
def test_refusals_leave_the_outputs_untouched():
    from gpmpc.solver import BatchSolver

    torch = U.gpu_torch()
    c = case("a")
    spec, P, T = c.spec, c.P, c.T
    x0t, ut, xrt, xit = (torch.tensor(np.ascontiguousarray(a), device="cuda") for a in (c.x0, c.u, c.plain(), c.xi))
    xo = torch.full((P, T + 1, spec.nx), float("nan"), dtype=torch.float64, device="cuda")
    uo = torch.full((P, T, spec.nu), float("nan"), dtype=torch.float64, device="cuda")
    vo = torch.full((P, T, spec.n_gp), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = c.s.lib
    Knan = c.K.copy()
    Knan[-1, -1] = np.nan
    Kinf = c.K.copy()
    Kinf[0, 0] = np.inf

    def call(h, P=P, T=T, x0=True, u=True, xref=True, K=c.K, clip=1, xi=True, with_gp=1, with_noise=1, x=True, uapp=True,
             var=True):
        return lib.gpmpc_rollout_sample(h, P, T, x0t.data_ptr() if x0 else None, ut.data_ptr() if u else None,
                                        xrt.data_ptr() if xref else None, None if K is None else K.ctypes.data, clip,
                                        xit.data_ptr() if xi else None, with_gp, with_noise, xo.data_ptr() if x else None,
                                        uo.data_ptr() if uapp else None, vo.data_ptr() if var else None)

    for kw, cause in ((dict(P=0), b"P, T >= 1"), (dict(P=-2), b"P, T >= 1"), (dict(T=0), b"P, T >= 1"), (dict(T=-1), b"P, T >= 1"),
                      (dict(x0=False), b"null array"), (dict(u=False), b"null array"), (dict(x=False), b"null array"),
                      (dict(with_gp=2), b"with_gp"), (dict(with_gp=-1), b"with_gp"),
                      (dict(with_noise=2), b"with_noise"), (dict(with_noise=-1), b"with_noise"),
                      (dict(clip=2), b"clip"), (dict(clip=-1), b"clip"),
                      (dict(K=None), b"K and xref_dev go together"), (dict(xref=False), b"K and xref_dev go together"),
                      (dict(K=Knan), b"non-finite"), (dict(K=Kinf), b"non-finite"),
                      (dict(P=60_000_000, T=5), b"int32"), (dict(P=1, T=2**31 - 1), b"int32")):
        assert call(c.s._h, **kw) == -1 and cause in lib.gpmpc_last_error(), kw
    assert call(None) == -1 and b"null handle" in lib.gpmpc_last_error()
    # before gpmpc_set_model
    h = ctypes.c_void_p()
    assert lib.gpmpc_create(spec.model_id, 5, 2, torch.cuda.current_device(), ctypes.byref(h)) == 0
    try:
        for with_gp in (0, 1):
            assert call(h, with_gp=with_gp, xi=False, var=False) == -3 and b"gpmpc_set_model" in lib.gpmpc_last_error()
    finally:
        lib.gpmpc_destroy(h)
    # the GPs off: none set, or switched off; the draws or the variance without a GP, or without its Linv
    fresh = BatchSolver(spec, 5, 2)
    assert call(fresh._h, xi=False, var=False) == -3 and b"GPs are off" in lib.gpmpc_last_error()
    assert call(fresh._h, with_gp=0, var=False) == -3 and b"not set" in lib.gpmpc_last_error()
    assert call(fresh._h, with_gp=0, xi=False) == -3 and b"not set" in lib.gpmpc_last_error()
    fresh.set_gps(c.gpp, with_variance=False)
    assert call(fresh._h, var=False) == -3 and b"Linv" in lib.gpmpc_last_error()
    assert call(fresh._h, xi=False) == -3 and b"Linv" in lib.gpmpc_last_error()
    assert call(fresh._h, with_gp=0) == -3 and b"Linv" in lib.gpmpc_last_error()
    fresh.set_gps(c.gpp)
    fresh.set_gps(None)
    assert call(fresh._h, xi=False, var=False) == -3 and b"GPs are off" in lib.gpmpc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(xo).all() and torch.isnan(uo).all() and torch.isnan(vo).all()
    # and the calls go through where nothing is in their way
    fresh.set_gps(c.gpp)
    assert call(fresh._h) == 0
    clean = c.run()
    assert same(xo.cpu().numpy(), clean["x"]) and same(uo.cpu().numpy(), clean["u"]) and same(vo.cpu().numpy(), clean["var"])
    xo.fill_(float("nan"))
    torch.cuda.synchronize()
    assert call(fresh._h, uapp=False, var=False) == 0 and same(xo.cpu().numpy(), clean["x"])
    fresh.set_gps(c.gpp, with_variance=False)
    xo.fill_(float("nan"))
    torch.cuda.synchronize()
    assert call(fresh._h, K=None, xref=False, clip=0, xi=False, var=False) == 0   # no variance needed: no Linv needed
    assert same(xo.cpu().numpy(), c.plain())


# ------------------------------------------------------------------------------------------------ 9
@functools.lru_cache(maxsize=None)
def _controller():
    from gpmpc.gpmpc import GPMPC

    U.gpu_torch()
    spec, data, _ = problem("quad2d", 40)
    ctrl = GPMPC("quad2d", horizon=5, batch=8, variance="exact")
    ctrl.train_gp(np.hstack([X for X, _ in data]), np.column_stack([y for _, y in data]), lr=0.05, iterations=20)
    ctrl.reset()
    return spec, ctrl


def test_controller_samples_trajectories_and_reports_coverage():
    from gpmpc.learning import tightening_coverage

    torch = U.gpu_torch()
    spec, ctrl = _controller()
    B, T, S = 3, 6, 5
    x0, _ = initial_states(spec, ctrl.traj, B)
    u = spec.u_eq + 0.1 * np.random.default_rng(4).standard_normal((B, T, spec.nu))
    x, ua = ctrl.sample_trajectories(x0, u, S, seed=3)
    assert x.shape == (B, S, T + 1, spec.nx) and ua.shape == (B, S, T, spec.nu) and np.isfinite(x).all()
    assert same(x[:, :, 0], np.repeat(x0[:, None], S, axis=1)) and not same(x[:, 0], x[:, 1])
    x1, u1 = ctrl.sample_trajectories(x0[1], u[1], S, seed=3, feedback="lqr")
    assert x1.shape == (S, T + 1, spec.nx) and u1.shape == (S, T, spec.nu)
    assert not same(u1, np.repeat(u[1][None], S, axis=0))          # the feedback acts
    again, _ = ctrl.sample_trajectories(x0, u, S, seed=3)
    other, _ = ctrl.sample_trajectories(x0, u, S, seed=4)
    assert same(again, x) and not same(other, x)
    # the draws forced to zero: the sample is the mean prediction (the draw is then an exact zero added to every mean;
    # what is left is the rounding of that sum inside the step, a few ulp of the state per step)
    mean = ctrl.predict_trajectory(x0, u)
    zero = ctrl.solver.rollout_sample(torch.tensor(x0, device="cuda"), torch.tensor(u, device="cuda"),
                                      xi=torch.zeros(B, T, spec.n_gp, dtype=torch.float64, device="cuda"), with_noise=True)
    d = np.abs(zero["x"].cpu().numpy() - mean)
    print(f"[rollout_sample] zero draws against predict_trajectory: max |d| {d.max():.3e}, bit for bit {same(zero['x'].cpu().numpy(), mean)}")
    assert (d <= 1e-10 * (1.0 + np.abs(mean))).all() and same(zero["u"].cpu().numpy(), u)
    cov = tightening_coverage(ctrl, x0, u, 16, seed=1)
    print(f"[rollout_sample] tightening_coverage (prob {ctrl.prob}):\n{cov}")
    assert cov.shape == (T + 1, spec.nx) and np.isnan(cov[0]).all()
    assert (np.isnan(cov) | ((cov >= 0.0) & (cov <= 1.0))).all() and np.isfinite(cov[1:]).any()
