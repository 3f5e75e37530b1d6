"""gpmpc_preprocess on the MI355X: GP training rows from transitions, against GPMPC.preprocess_data in numpy.

P = 40 transitions per model (states around the reference, inputs uniform over the input box, one plant step each
with the true parameters).  The inputs are copies and must be bit-equal.  The targets' bound is derived, not
tuned: |dev - ref| <= 16 eps S, S the target's own expression with every summand replaced by its absolute value
(observe_ref.target_scale): both sides evaluate the same formula in float64, and differ by the handful of roundings
along it, a 2-ulp sincos, the sqrt and FMA contraction, each at most an ulp or two of a partial sum no larger
than S."""

import ctypes

import numpy as np
import pytest

import gp_update_util as U
import observe_ref as OR

pytestmark = pytest.mark.gpu

P = 40
EPS = np.finfo(np.float64).eps
MODELS = ("quad2d", "quad3d", "cartpole")
_CASES: dict = {}


def _case(name):
    """The model's solver (H = 5, B = 40), its transitions on the host and the device, and the numpy reference."""
    torch = U.gpu_torch()
    from gpmpc.gpmpc import GPMPC
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    if name not in _CASES:
        spec = get_spec(name)
        s = BatchSolver(spec, 5, P)
        x, u = OR.transitions(spec, P)
        xn = s.plant_step(torch.tensor(x, device="cuda"), torch.tensor(u, device="cuda")).cpu().numpy()
        _CASES[name] = dict(spec=spec, s=s, x=x, u=u, xn=xn)
    c = _CASES[name]
    if "ref" not in c:
        c["ref"] = _reference(c["spec"], c["x"], c["u"], c["xn"])
    return c


def _reference(spec, x, u, xn):
    from gpmpc.gpmpc import GPMPC

    me = type("Me", (), {})()
    me.model = spec
    me.acc_symbolic_fn = GPMPC.setup_symbolic_acceleration(me, spec.prior) if "a" in spec.prior else None
    me.prior_dynamics = lambda xs, us: spec.prior_f(xs, us)
    with np.errstate(invalid="ignore"):
        return GPMPC.preprocess_data(me, x, u, xn)


def _call(c, m, pick=None, x=None, u=None, xn=None, inputs=True, targets=True, P_=P, dt=None, grav=None):
    """gpmpc_preprocess on guarded outputs; returns (inputs (m, D), targets (m, n_gp)) with the guards checked."""
    torch = U.gpu_torch()
    from gpmpc import _lib

    s, spec = c["s"], c["spec"]
    D, G = sum(spec.gp_dims), spec.n_gp
    dev = [torch.tensor(c[k] if a is None else a, device="cuda") for k, a in (("x", x), ("u", u), ("xn", xn))]
    pk = None if pick is None else torch.tensor(np.asarray(pick, dtype=np.int32), device="cuda")
    ib, tb = U.guarded(m * D), U.guarded(m * G)
    dt0, g0 = s._diff_constants()
    _lib.check(s.lib.gpmpc_preprocess(s._h, P_, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), m,
                                      _lib.ptr(pk), dt0 if dt is None else dt, g0 if grav is None else grav,
                                      ib.data_ptr() if inputs else None, tb.data_ptr() if targets else None,
                                      s._stream()))
    torch.cuda.synchronize()
    out = []
    for buf, n, cols in ((ib, m * D, D), (tb, m * G, G)):
        a = buf.cpu().numpy()
        assert (a[n:] == U.SENTINEL).all(), "wrote past the end of the output"
        out.append(a[:n].reshape(m, cols).copy())
    return out


def _check(c, rows, inputs, targets, what):
    """Rows `rows` of the reference against the device's outputs: inputs bit-equal, targets within 16 eps S."""
    spec = c["spec"]
    ri, rt = c["ref"]
    rows = np.asarray(rows)
    assert not np.isnan(inputs).any() and not np.isnan(targets).any(), f"{what}: outputs not written"
    np.testing.assert_array_equal(inputs, ri[rows], err_msg=what)
    S = OR.target_scale(spec, c["x"], c["u"], c["xn"], *c["s"]._diff_constants())[rows]
    ratio = np.abs(targets - rt[rows]) / (EPS * S)
    print(f"[preprocess] {spec.name} {what}: worst |dev - ref| / (eps S) per target {ratio.max(0)}")
    assert (ratio <= 16.0).all(), (what, ratio.max(0))


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("m", [1, 16, 17, 40])
def test_first_rows_match_preprocess_data(name, m):
    c = _case(name)
    inputs, targets = _call(c, m)
    _check(c, np.arange(m), inputs, targets, f"rows 0..{m - 1}")


@pytest.mark.parametrize("name", MODELS)
def test_picks_with_repeats(name):
    c = _case(name)
    pick = np.random.default_rng(8).permutation(P)[:33]
    pick[5], pick[20], pick[32] = pick[4], pick[0], pick[0]
    inputs, targets = _call(c, 33, pick)
    _check(c, pick, inputs, targets, "33 picks with repeats")


@pytest.mark.parametrize("name", MODELS)
def test_picks_out_of_range_give_nan_rows(name):
    c = _case(name)
    pick = np.array([3, -1, 7, P, 0, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)
    inputs, targets = _call(c, len(pick), pick.astype(np.int32))
    bad = np.array([1, 3, 5, 6])
    assert np.isnan(inputs[bad]).all() and np.isnan(targets[bad]).all()
    good = np.array([0, 2, 4])
    _check(c, pick[good], inputs[good], targets[good], "the rows between out-of-range picks")


@pytest.mark.parametrize("name", MODELS)
def test_a_nan_transition_stays_in_its_row(name):
    c = _case(name)
    xn = c["xn"].copy()
    xn[9] = np.nan
    inputs, targets = _call(c, 17, xn=xn)
    assert np.isnan(targets[9]).all()
    np.testing.assert_array_equal(inputs[9], c["ref"][0][9])   # (the inputs come from x and u)
    keep = np.r_[0:9, 10:17]
    _check(c, keep, inputs[keep], targets[keep], "the rows around a NaN transition")


@pytest.mark.parametrize("name", MODELS)
def test_wrapper_and_single_outputs(name):
    torch = U.gpu_torch()
    c = _case(name)
    s = c["s"]
    dev = [torch.tensor(c[k], device="cuda") for k in ("x", "u", "xn")]
    pick = torch.tensor([4, 4, 39, 0], dtype=torch.int32, device="cuda")
    inputs, targets = s.preprocess(*dev, pick=pick)
    full_i, full_t = _call(c, 4, [4, 4, 39, 0])
    np.testing.assert_array_equal(inputs.cpu().numpy(), full_i)
    np.testing.assert_array_equal(targets.cpu().numpy(), full_t)
    only_i, untouched = _call(c, 4, [4, 4, 39, 0], targets=False)
    np.testing.assert_array_equal(only_i, full_i)
    assert np.isnan(untouched).all()
    untouched, only_t = _call(c, 4, [4, 4, 39, 0], inputs=False)
    np.testing.assert_array_equal(only_t, full_t)
    assert np.isnan(untouched).all()
    i2, t2 = s.preprocess(*dev, m=7)
    assert i2.shape == (7, sum(c["spec"].gp_dims)) and t2.shape == (7, c["spec"].n_gp)
    np.testing.assert_array_equal(i2.cpu().numpy(), c["ref"][0][:7])


def test_refusals_leave_the_outputs_untouched():
    torch = U.gpu_torch()
    from gpmpc import _lib

    c = _case("quad2d")
    s = c["s"]
    x, u, xn = (torch.tensor(c[k], device="cuda") for k in ("x", "u", "xn"))
    pick = torch.zeros(50, dtype=torch.int32, device="cuda")
    ib, tb = U.guarded(50 * 4), U.guarded(50 * 2)
    dt, g = s._diff_constants()
    ok = dict(P=P, x=x.data_ptr(), u=u.data_ptr(), xn=xn.data_ptr(), m=8, pick=None, dt=dt, g=g, i=ib.data_ptr(),
              t=tb.data_ptr())

    def call(h=None, **kw):
        a = {**ok, **kw}
        return s.lib.gpmpc_preprocess(s._h if h is None else h, a["P"], a["x"], a["u"], a["xn"], a["m"], a["pick"],
                                      a["dt"], a["g"], a["i"], a["t"], s._stream())

    for kw in (dict(P=0), dict(m=0), dict(x=None), dict(u=None), dict(xn=None), dict(i=None, t=None), dict(m=41),
               dict(dt=0.0), dict(dt=-0.02), dict(dt=float("inf")), dict(dt=float("nan")), dict(g=float("nan")),
               dict(g=float("inf"))):
        assert call(**kw) == -1, kw
    assert call(m=50, pick=pick.data_ptr()) == 0   # (with picks m may exceed P)
    torch.cuda.synchronize()
    ib.copy_(U.guarded(50 * 4))
    tb.copy_(U.guarded(50 * 2))
    h = ctypes.c_void_p()
    _lib.check(s.lib.gpmpc_create(c["spec"].model_id, 5, P, s.dev_index, ctypes.byref(h)))
    try:
        assert call(h=h) == -3   # before gpmpc_set_model
        assert b"gpmpc_set_model" in s.lib.gpmpc_last_error()
    finally:
        s.lib.gpmpc_destroy(h)
    assert call(P=0) == -1
    torch.cuda.synchronize()
    for buf in (ib, tb):
        a = buf.cpu().numpy()
        n = len(a) - U.GUARD
        assert np.isnan(a[:n]).all() and (a[n:] == U.SENTINEL).all()
