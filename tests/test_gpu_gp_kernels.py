"""GP posterior kernels (csrc/gp_kernels.hip) at every dispatch shape, and the domain of exp_rbf /
exp_rbf_n (csrc/gpmpc_common.h), on synthetic operands against an extended-precision reference
(tests/gp_ref.py, which states the operands, the reference and the error bound; MI355X only).

Every case pre-fills its outputs with NaN, keeps 64 sentinel doubles past their end, and asserts
|err| <= tol elementwise with the reference's worst-case bound; max(err / tol) per kernel family is
printed (run with -s).  Families, by what launch_gp_post_batch picks:

  post<FROM_STATE, FULL>       gp_post_kernel (mean, mean + variance, npad > 256, dense roots, mixed launches)
  var_tri<FROM_STATE>          gp_var_tri_kernel<NT>, NT = 1..16
  var_split<FROM_STATE>        gp_var_split_kernel<NT, ., 4>, NT = 1..16
  love                         gp_love_kernel -> love_points<NF, NQ, true>

Handle-based cases load synthetic GPs with alpha = 0 (the dynamics stay the prior's) into a
BatchSolver and read the tightening's variance launch back (solve, set_iterate, solve, variance),
like test_tightening_variance_matches_oracle; the solves' statuses are not asserted.  The inverse
factors are scaled (by a power of two, gp_ref.reference) so that the reference variance is
>= sf2 / 2 at every point, which is asserted before any GPU call.
"""

import functools

import numpy as np
import pytest

import gp_ref as R
from helpers import initial_states, lqr

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")]

GUARD = 64
SENTINEL = -7.25e77
RATIOS: dict = {}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _record(family, got, want, tol, what=""):
    """Assert |got - want| <= tol elementwise; print and keep max(err / tol) of the family."""
    got, want, tol = np.asarray(got), np.asarray(want), np.asarray(tol)
    assert got.shape == want.shape, (family, what, got.shape, want.shape)
    assert np.isfinite(got).all(), (family, what)
    ratio = float((np.abs(got - want) / tol).max())
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print(f"[gp-kernels] {family:22s} {what:44s} max(err/tol) = {ratio:.3e}   (family max {RATIOS[family]:.3e})")
    assert ratio <= 1.0, (family, what, ratio)


def _guarded(P):
    """NaN-filled output of P doubles followed by GUARD sentinels."""
    torch = _torch()
    t = torch.full((P + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    t[P:] = SENTINEL
    return t


def _read(t, P, what=""):
    """The P outputs: sentinel untouched, no NaN left."""
    a = t.cpu().numpy()
    assert (a[P:] == SENTINEL).all(), f"{what}: wrote past the end of the output"
    assert not np.isnan(a[:P]).any(), f"{what}: {int(np.isnan(a[:P]).sum())} of {P} outputs not written"
    return a[:P].copy()


def _untouched(t, P):
    a = t.cpu().numpy()
    return bool(np.isnan(a[:P]).all() and (a[P:] == SENTINEL).all())


def _c(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


# ============================================================================ (a) handle-free
NS = [1, 15, 16, 17, 100, 240, 255, 256, 257, 300, 500, 512, 520]


@functools.lru_cache(maxsize=None)
def _free_case(n, d, P, with_linv=True):
    """Synthetic GP n x d, its device layout (zero padded to npad) and the reference at P points."""
    torch = _torch()
    gp = R.synthetic_gp(n, d, seed=1000 * d + n)
    Z = R.points(P, d, seed=77 + n + d)
    ref = R.reference(gp["X"], gp["ell"], gp["sf2"], Z, alpha=gp["alpha"], B=gp["Linv"].T if with_linv else None,
                      frac=0.4 if with_linv else None)
    npad = (n + 15) // 16 * 16
    rows = np.zeros((npad, 4))
    rows[:n, :d] = gp["X"]
    rows[:n, 3] = gp["alpha"]
    lay = dict(npad=npad, rows=torch.tensor(rows, device="cuda"), linvT=None)
    if with_linv:
        lt = np.zeros((npad, npad))
        lt[:n, :n] = (ref["scale"] * gp["Linv"]).T
        lay["linvT"] = torch.tensor(lt, device="cuda")
    return gp, Z, ref, lay


def _posterior(gp, lay, Z, want_mean, want_var, with_noise, what):
    """gpmpc_gp_posterior at Z into guarded buffers; returns (mean, var) host arrays or None."""
    torch = _torch()
    from gpmpc import _lib

    lib = _lib.load()
    P = Z.shape[0]
    Zt = torch.tensor(_c(Z), device="cuda")
    m = _guarded(P) if want_mean else None
    v = _guarded(P) if want_var else None
    _lib.check(lib.gpmpc_gp_posterior(gp["n"], gp["d"], lay["npad"], _lib.ptr(lay["rows"]),
                                      _lib.ptr(lay["linvT"]) if want_var else None, gp["ell"], gp["sf2"], gp["sn2"],
                                      _lib.ptr(Zt), P, _lib.ptr(m), _lib.ptr(v), int(with_noise),
                                      _lib.stream_ptr(Zt.device)))
    torch.cuda.synchronize()
    return (_read(m, P, what + " mean") if want_mean else None), (_read(v, P, what + " var") if want_var else None)


def _post_family(npad, from_state=False):
    return f"post<{'state' if from_state else 'dense'},{'FULL' if npad >= 256 else 'part'}>"


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n", NS)
def test_posterior_mean_and_variance(n, d):
    """gp_post_kernel, mean + variance in one launch, with and without noise; P = 37 is three point
    tiles, the last partly valid.  npad <= 240: one column group of npad / 16 tiles (non-FULL);
    255, 256: one full group; 257: 16 + 1 tiles; 500, 512: two full groups; 520: 16 + 16 + 1."""
    gp, Z, ref, lay = _free_case(n, d, 37)
    for noise in (0, 1):
        what = f"n={n} d={d} noise={noise}"
        m, v = _posterior(gp, lay, Z, True, True, noise, what)
        fam = _post_family(lay["npad"])
        _record(fam, m, ref["mean"], ref["tol_mean"], what + " mean")
        _record(fam, v, ref["var"] + (gp["sn2"] if noise else 0.0), ref["tol_var"], what + " var")


@pytest.mark.parametrize("n", NS)
def test_posterior_point_counts(n):
    """The same training sizes at P = 1 .. 300 points (one lane, one tile, a tile + 1, a workgroup
    - 1 / + 0 / + 1, three workgroups), d = 2."""
    gp, Z, ref, lay = _free_case(n, 2, 300)
    for P in (1, 16, 17, 127, 128, 129, 300):
        what = f"n={n} P={P}"
        m, v = _posterior(gp, lay, Z[:P], True, True, 1, what)
        fam = _post_family(lay["npad"])
        _record(fam, m, ref["mean"][:P], ref["tol_mean"][:P], what + " mean")
        _record(fam, v, ref["var"][:P] + gp["sn2"], ref["tol_var"][:P], what + " var")


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 17, 300])
def test_posterior_mean_only(n, d):
    """linvT = NULL: the mean-only path of gp_post_kernel."""
    gp, Z, ref, lay = _free_case(n, d, 37, with_linv=False)
    m, v = _posterior(gp, lay, Z, True, False, 0, f"n={n} d={d}")
    assert v is None
    _record("post<dense,mean-only>", m, ref["mean"], ref["tol_mean"], f"n={n} d={d} mean")


def _n_cu():
    return int(_torch().cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("NT", range(1, 17))
def test_variance_only_split(NT):
    """mean = NULL at npad = 16 NT, n = 16 NT - 3, P = 37: few points, so the launch takes the
    four-wave column split, gp_var_split_kernel<NT, false, 4> (two workgroups of two point tiles,
    the last tile partly valid)."""
    assert 2 * 1 <= _n_cu()
    d = 1 + NT % 3
    gp, Z, ref, lay = _free_case(16 * NT - 3, d, 37)
    for noise in (0, 1):
        what = f"NT={NT} d={d} P=37 noise={noise}"
        _, v = _posterior(gp, lay, Z, False, True, noise, what)
        _record("var_split<dense>", v, ref["var"] + (gp["sn2"] if noise else 0.0), ref["tol_var"], what)


@pytest.mark.parametrize("NT", range(1, 17))
def test_variance_only_unsplit(NT):
    """The same with just enough points to turn the split off (2 ceil(P / 128) > CUs):
    gp_var_tri_kernel<NT, false>.  The P points cycle through 193 distinct ones with stride 7, so
    every wave's 16 points differ and the reference is computed on the 193 only."""
    P = 128 * (_n_cu() // 2) + 1
    assert 2 * ((P + 127) // 128) > _n_cu()
    d = 1 + (NT + 1) % 3
    gp, Zu, ref, lay = _free_case(16 * NT - 3, d, 193)
    idx = (7 * np.arange(P)) % 193
    what = f"NT={NT} d={d} P={P}"
    _, v = _posterior(gp, lay, Zu[idx], False, True, 1, what)
    _record("var_tri<dense>", v, ref["var"][idx] + gp["sn2"], ref["tol_var"][idx], what)


# ============================================================================ (b) handle-based
SF2, SN2 = 1e-3, 1e-6
_SOLVERS: dict = {}
_CASE = [0]


def _solver(name, H, B):
    """One BatchSolver per (model, H, B), tightening on, shared by the cases (each loads its GPs)."""
    _torch()
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    key = (name, H, B)
    if key not in _SOLVERS:
        spec = get_spec(name)
        s = BatchSolver(spec, H, B)
        s.set_tightening(True, 0.95, *lqr(spec))
        _SOLVERS[key] = s
    return _SOLVERS[key]


def _iterate(s):
    """A seeded iterate in [-1, 1] (a new one per call, so a variance the kernel left unwritten
    cannot pass on a stale value) and the GP inputs z_k = [x_k; u_k][var_inputs] per GP."""
    _CASE[0] += 1
    rng = np.random.default_rng(5000 + _CASE[0])
    B, H = s.batch, s.H
    xs = rng.uniform(-1.0, 1.0, (B, H + 1, s.nx))
    us = rng.uniform(-1.0, 1.0, (B, H, s.nu))
    z = np.concatenate([xs[:, :H, :], us], axis=2)
    Zs = [_c(z[:, :, list(idx)].reshape(B * H, len(idx))) for idx in s.spec.var_inputs]
    return xs, us, Zs


def _load(s, g, gp, Z, root=None, alpha=None, linv=True):
    """gpmpc_set_gp of the synthetic GP (alpha = 0 unless given) with Linv scaled for the points Z,
    and optionally a dense root (n, r), also scaled; returns the reference of the variance the
    handle will compute at Z (noise not included)."""
    from gpmpc import _lib

    n, d = gp["n"], gp["d"]
    ref = R.reference(gp["X"], gp["ell"], gp["sf2"], Z, alpha=alpha, B=gp["Linv"].T, frac=0.4)
    X, a, L = _c(gp["X"]), _c(np.zeros(n) if alpha is None else alpha), _c(ref["scale"] * gp["Linv"])
    _lib.check(s.lib.gpmpc_set_gp(s._h, g, n, d, X.ctypes.data, a.ctypes.data, 0, None,
                                  L.ctypes.data if linv else None, gp["ell"], gp["sf2"], gp["sn2"]))
    if root is not None:
        ref = R.reference(gp["X"], gp["ell"], gp["sf2"], Z, B=root, frac=0.4)
        Rs = _c(ref["scale"] * root)
        _lib.check(s.lib.gpmpc_set_gp_variance_root(s._h, g, n, Rs.shape[1], Rs.ctypes.data))
    assert ref["var"].min() >= 0.5 * gp["sf2"], (g, ref["var"].min())   # sqrt(var) of the tightening stays real
    return ref


def _state_variance(s, xs, us, what):
    """solve, set_iterate(xs, us), solve, gpmpc_get_variance into a guarded buffer -> (B H, n_gp)."""
    torch = _torch()
    from gpmpc import _lib

    _lib.check(s.lib.gpmpc_use_gp(s._h, 1))
    B, H, ngp = s.batch, s.H, s.spec.n_gp
    x0, ph = initial_states(s.spec, s.spec.reference_trajectory(), B)
    obs = torch.tensor(x0, device="cuda")
    ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
    s.reset(reset_iterate=True)
    s.solve(obs, ts)                                    # marks a previous solution
    s.set_iterate(torch.tensor(xs, device="cuda"), torch.tensor(us, device="cuda"))
    s.solve(obs, ts)                                    # variance launch at (xs, us)
    v = _guarded(B * H * ngp)
    _lib.check(s.lib.gpmpc_get_variance(s._h, B, v.data_ptr(), s._stream()))
    torch.cuda.synchronize()
    return _read(v, B * H * ngp, what).reshape(B * H, ngp)


def _gps(s, ns, seed):
    return [R.synthetic_gp(n, d, seed=seed + 17 * g, sf2=SF2, sn2=SN2) for g, (n, d) in enumerate(zip(ns, s.spec.gp_dims))]


def _run_state(s, ns, family, what, roots=None, seed=0):
    """Load GPs of ns[g] rows (and roots[g] = rank or None), run the variance launch, check."""
    xs, us, Zs = _iterate(s)
    gps = _gps(s, ns, seed)
    refs = []
    for g, gp in enumerate(gps):
        r = None if roots is None else roots[g]
        root = None if r is None else R.synthetic_root(gp["n"], r, seed=900 + r + g)
        refs.append(_load(s, g, gp, Zs[g], root=root))
    v = _state_variance(s, xs, us, what)
    for g, ref in enumerate(refs):
        _record(family, v[:, g], ref["var"] + SN2, ref["tol_var"], f"{what} gp{g}")
    return v


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("NT", range(1, 17))
def test_state_variance_every_tile_count(NT, split):
    """quad2d (GP0 d = 1, GP1 d = 3), B = 5, H = 7 (35 points: three point tiles, the last partly
    valid), both GPs n = 16 NT - 3: gp_var_tri_kernel<NT, true> (var_split = 1) and
    gp_var_split_kernel<NT, true, 4> (var_split = 4)."""
    s = _solver("quad2d", 7, 5)
    s.set_tuning(var_split=split)
    try:
        _run_state(s, [16 * NT - 3] * 2, "var_tri<state>" if split == 1 else "var_split<state>",
                   f"NT={NT} split={split}", seed=100 * NT + split)
    finally:
        s.set_tuning(var_split=0)


def test_state_variance_automatic_split_threshold():
    """var_split = 0 at a batch on each side of the automatic threshold (2 workgroups of 128
    points x GPs <= CUs): bit-identical to the forced run of the kernel it selects (the two kernels
    sum in different orders, so each automatic run is compared with its own kernel's forced run)."""
    H, ngp = 16, 2
    blocks = _n_cu() // (2 * ngp)           # largest 128-point block count that still splits
    b_lo = 128 * blocks // H
    for B, split in ((b_lo, 4), (b_lo + 1, 1)):
        nblk = (B * H + 127) // 128
        assert (2 * nblk * ngp <= _n_cu()) == (split == 4)
        s = _solver("quad2d", H, B)
        xs, us, Zs = _iterate(s)
        refs = [_load(s, g, gp, Zs[g]) for g, gp in enumerate(_gps(s, [45, 45], seed=31))]
        out = {}
        for mode in (0, 1, 4):
            s.set_tuning(var_split=mode)
            out[mode] = _state_variance(s, xs, us, f"B={B} var_split={mode}")
        s.set_tuning(var_split=0)
        for g, ref in enumerate(refs):
            _record("var_tri<state>", out[1][:, g], ref["var"] + SN2, ref["tol_var"], f"B={B} forced 1 gp{g}")
            _record("var_split<state>", out[4][:, g], ref["var"] + SN2, ref["tol_var"], f"B={B} forced 4 gp{g}")
        print(f"[gp-kernels] B={B}: forced kernels differ in {int((out[1] != out[4]).sum())} of {out[1].size} values")
        assert not np.array_equal(out[1], out[4]), "the forced kernels agree bit for bit: the comparison cannot tell them apart"
        assert np.array_equal(out[0], out[split]), (B, split)


def _love_tiles(rank):
    """love_tiles of gp_kernels.hip."""
    nf, nq = rank >> 4, ((rank & 15) + 3) >> 2
    return (nf + 1, 0) if nq > 2 else (nf, nq)


def _love_ranks():
    """The smallest rank of every (NF, NQ) pair ranks 1..128 reach, and the boundary ranks."""
    first = {}
    for r in range(1, 129):
        first.setdefault(_love_tiles(r), r)
    return sorted(set(first.values()) | {4, 5, 8, 9, 16, 17, 116, 120, 121, 128}), sorted(first)


_RANKS, _PAIRS = _love_ranks()
# two GPs of different rank per launch; npad / 16 = 1..4 rounds of the two-buffer loop in turn
_LOVE_CASES = [(_RANKS[i], _RANKS[-1 - i], (13, 29, 45, 61)[i % 4], (61, 45, 29, 13)[(i // 4) % 4])
               for i in range((len(_RANKS) + 1) // 2)]


def test_love_rank_list_covers_every_pair():
    """(CPU-only arithmetic) the cases below reach every (NF, NQ) pair of love_tiles for ranks
    1..128 -- 24 pairs: NF = 0 has no NQ = 0, and NF = 8 only NQ = 0 -- and every boundary rank."""
    used = {r for c in _LOVE_CASES for r in c[:2]}
    assert used == set(_RANKS) and {_love_tiles(r) for r in used} == set(_PAIRS)
    assert len(_PAIRS) == 24 and {4, 5, 8, 9, 16, 17, 116, 120, 121, 128} <= used
    assert {(n + 15) // 16 for c in _LOVE_CASES for n in c[2:]} == {1, 2, 3, 4}


@pytest.mark.parametrize("r0,r1,n0,n1", _LOVE_CASES)
def test_state_variance_love_roots(r0, r1, n0, n1):
    """gp_love_kernel: synthetic dense roots of different rank on the two GPs of quad2d in one
    launch (each block dispatches its own GP's love_points<NF, NQ, true>)."""
    s = _solver("quad2d", 7, 5)
    _run_state(s, [n0, n1], "love", f"ranks=({r0},{r1}) n=({n0},{n1})", roots=[r0, r1], seed=r0 + 200 * r1)


def test_state_variance_love_roots_cartpole():
    """Both GPs d = 3 (cartpole), ranks 37 (2 tiles + 2 quads) and 100 (6 tiles + 1 quad)."""
    s = _solver("cartpole", 7, 5)
    _run_state(s, [45, 61], "love", "cartpole ranks=(37,100)", roots=[37, 100], seed=7)


@pytest.mark.parametrize("r", [129, 200, 240, 241, 256])
def test_state_variance_dense_root(r):
    """Roots past the LOVE kernel's 128 columns run gp_post_kernel<true, FULL> with a dense B
    (tri == false): non-FULL up to 240 columns, FULL from 241 (256 padded columns)."""
    s = _solver("quad2d", 7, 5)
    _run_state(s, [61, 29], _post_family(256 if r > 240 else 0, True), f"dense root r={r}", roots=[r, r], seed=r)


@pytest.mark.parametrize("ns,roots", [((40, 300), None), ((40, 100), (24, None)), ((40, 60), (24, 200)),
                                      ((300, 300), None)])
def test_state_variance_mixed_launch(ns, roots):
    """Launches that are neither all-LOVE nor all-triangular: different npad (the 300-row GP then
    runs the non-FULL kernel over two column groups, t0 > 0), a root beside an exact GP, a LOVE-size
    root beside a dense one, and both exact at n = 300 (FULL, state-sourced)."""
    s = _solver("quad2d", 7, 5)
    full = roots is None and min(ns) > 240
    _run_state(s, list(ns), _post_family(256 if full else 0, True), f"mixed n={ns} roots={roots}",
               roots=None if roots is None else list(roots), seed=sum(ns))


@pytest.mark.parametrize("gp_id,n", [(0, 300), (1, 100)])
def test_handle_gp_predict(gp_id, n):
    """gpmpc_gp_predict (BatchSolver.gp_predict): mean only, variance only (npad <= 256: the
    FROM_STATE = false triangular / split kernels; above: gp_post_kernel), both; with and without
    noise; P = 1 and 129; P = 0 touches nothing; variance without Linv is GPMPC_ERR_STATE (-3)."""
    torch = _torch()
    from gpmpc import _lib

    s = _solver("quad2d", 7, 5)
    d = s.spec.gp_dims[gp_id]
    gp = R.synthetic_gp(n, d, seed=40 + n, sf2=SF2, sn2=SN2)
    Z = R.points(129, d, seed=41 + n)
    ref = _load(s, gp_id, gp, Z, alpha=gp["alpha"])
    fam_var = "var_split<dense>" if n <= 256 else _post_family(n)
    for P in (1, 129):
        Zt = torch.tensor(_c(Z[:P]), device="cuda")
        for noise in (0, 1):
            for want_mean, want_var in ((True, False), (False, True), (True, True)):
                what = f"gp_predict gp{gp_id} n={n} P={P} noise={noise} mean={want_mean} var={want_var}"
                mb, vb = (_guarded(P) if want_mean else False), (_guarded(P) if want_var else False)
                m, v = s.gp_predict(gp_id, Zt, with_noise=bool(noise), mean=mb, var=vb)
                torch.cuda.synchronize()
                assert (m is None) == (not want_mean) and (v is None) == (not want_var)
                if want_mean:
                    _record("post<dense,mean-only>", _read(m, P, what), ref["mean"][:P], ref["tol_mean"][:P], what)
                if want_var:
                    _record(fam_var, _read(v, P, what), ref["var"][:P] + (SN2 if noise else 0.0),
                            ref["tol_var"][:P], what)
    mb, vb = _guarded(8), _guarded(8)
    m, v = s.gp_predict(gp_id, torch.zeros(0, d, dtype=torch.float64, device="cuda"), mean=mb, var=vb)
    torch.cuda.synchronize()
    assert _untouched(mb, 8) and _untouched(vb, 8)
    _load(s, gp_id, gp, Z, alpha=gp["alpha"], linv=False)
    vb = _guarded(1)
    with pytest.raises(_lib.GPMPCError, match=r"error -3: variance needs Linv"):
        s.gp_predict(gp_id, torch.tensor(_c(Z[:1]), device="cuda"), mean=False, var=vb)
    torch.cuda.synchronize()
    assert _untouched(vb, 1)
    m, _ = s.gp_predict(gp_id, torch.tensor(_c(Z[:1]), device="cuda"), mean=True, var=False)   # the mean still works
    _record("post<dense,mean-only>", m.cpu().numpy(), ref["mean"][:1], ref["tol_mean"][:1], "mean without Linv")
    _load(s, gp_id, gp, Z)   # leave the shared solver with a complete GP


# ============================================================================ (c) exp_rbf domain
def _exp_probe(z, alpha=1.0):
    """mean(z) = alpha exp(-z^2 / 2): one training row at 0, sf2 = ell = 1, d = 1, mean only."""
    torch = _torch()
    rows = np.zeros((16, 4))
    rows[0, 3] = alpha
    gp = dict(n=1, d=1, ell=1.0, sf2=1.0, sn2=0.0)
    lay = dict(npad=16, rows=torch.tensor(rows, device="cuda"), linvT=None)
    m, _ = _posterior(gp, lay, np.asarray(z, dtype=np.float64)[:, None], True, False, 0, "exp probe")
    return m


def test_exp_rbf_in_range():
    """exp_rbf on [-745, 0]: a 4000-point grid, the arguments nearest to every multiple of ln2 / 2 in
    [-40, 0] (the reduction's boundaries, and one float64 step either side of each) and x = 0.
    Down to x = -708.2 the relative error against the longdouble exp(-z^2 / 2) is
    <= (4 + 2 |x|) eps64 (1 ulp for the exp, the rounding of z^2, margin); below that the result is
    in [0, 3e-308].  (The split is at -708.2, not -708: exp(-708) = 3.3e-308, so on (-708.1, -708)
    the correctly rounded result is above 3e-308; exp(-708.2) = 2.7e-308 is still a normal number,
    n = -1022 and p > 1, so the relative bound holds that far and asks more than a split at -708.)"""
    x = np.concatenate([np.linspace(-745.0, 0.0, 4000), -0.5 * np.log(2.0) * np.arange(0, 116), [0.0]])
    z = np.sqrt(-2.0 * x)
    z = np.concatenate([z, np.nextafter(z, np.inf), np.nextafter(z, -np.inf)[z > 0]])
    got = _exp_probe(z)
    zl = z.astype(R.LD)
    xl = -zl * zl / R.LD(2)
    want = np.exp(xl)
    xs = xl.astype(np.float64)
    hi = xs >= -708.2
    assert hi.sum() > 3000 and (~hi).sum() > 100
    rel = (np.abs(got[hi].astype(R.LD) - want[hi]) / want[hi]).astype(np.float64)
    _record("exp_rbf", rel, np.zeros_like(rel), (4.0 + 2.0 * np.abs(xs[hi])) * R.EPS64, "relative error, x >= -708.2")
    assert got[z == 0.0].size and (got[z == 0.0] == 1.0).all()
    assert ((got[~hi] >= 0.0) & (got[~hi] <= 3e-308)).all(), got[~hi][(got[~hi] < 0) | (got[~hi] > 3e-308)]


FAR_X = [-1e4, -1.4e9, -1.5e9, -3e9, -5e9, -1e12, -1e16, -1e20, -1e300]


def test_exp_rbf_far_arguments():
    """exp_rbf is total on x <= 0: arguments past the wrap of the reduction's 32-bit n
    (x < -2^31 ln2 = -1.49e9) still give a value in [0, 3e-308], and a weight of 1e6 on it a finite
    mean below 1e-290."""
    z = np.sqrt(-2.0 * np.array(FAR_X))
    got = _exp_probe(z)
    print("[gp-kernels] exp_rbf far arguments:", dict(zip(FAR_X, got.tolist())))
    assert ((got >= 0.0) & (got <= 3e-308)).all(), dict(zip(FAR_X, got.tolist()))
    big = _exp_probe(z, alpha=1e6)
    assert np.isfinite(big).all() and (np.abs(big) < 1e-290).all(), dict(zip(FAR_X, big.tolist()))


def test_exp_rbf_n_far_points_mean_grad():
    """exp_rbf_n (the linearisation's tile path, BatchSolver.gp_mean_grad): points 1e2 .. 1e7
    lengthscales from the training data give a finite mean and gradient that are 0 or
    subnormal-small (< 1e-290); near points agree with the longdouble reference to
    1e-10 sf2 sum|alpha| (mean) and 1e-9 sf2 sum|alpha| / ell^2 (gradient), the bounds of
    test_linearisation_gp_mean_grad_matches_oracle."""
    torch = _torch()
    s = _solver("quad2d", 7, 5)
    for g, d in enumerate(s.spec.gp_dims):
        gp = R.synthetic_gp(50, d, seed=60 + g, sf2=1.0, sn2=SN2)
        near = R.points(24, d, seed=61 + g)
        _load(s, g, gp, near, alpha=gp["alpha"])
        rng = np.random.default_rng(62 + g)
        far = []
        for dist in (1e2, 1e4, 1e5, 1e7):
            u = rng.standard_normal((6, d))
            far.append(gp["X"][:6] + dist * gp["ell"] * u / np.linalg.norm(u, axis=1, keepdims=True))
        Z = np.vstack([near] + far)
        m, gr = s.gp_mean_grad(g, torch.tensor(Z, device="cuda"))
        m, gr = m.cpu().numpy(), gr.cpu().numpy()
        assert np.isfinite(m).all() and np.isfinite(gr).all(), (g, m[24:], gr[24:])
        assert (np.abs(m[24:]) < 1e-290).all() and (np.abs(gr[24:]) < 1e-290).all(), (g, m[24:], gr[24:])
        k = R.kernel_ld(gp["X"], gp["ell"], gp["sf2"], near)                     # (24, n)
        w = k * gp["alpha"].astype(R.LD)[None, :]
        mo = w.sum(1).astype(np.float64)
        diff = gp["X"].astype(R.LD)[None, :, :] - near.astype(R.LD)[:, None, :]  # x_i - z
        go = ((w[:, :, None] * diff).sum(1) / R.LD(gp["ell"]) ** 2).astype(np.float64)
        scale = gp["sf2"] * np.abs(gp["alpha"]).sum()
        _record("gp_tiles(exp_rbf_n)", m[:24], mo, np.full(24, 1e-10 * scale), f"gp{g} near mean")
        _record("gp_tiles(exp_rbf_n)", gr[:24], go, np.full((24, d), 1e-9 * scale / gp["ell"] ** 2), f"gp{g} near grad")
    for g, d in enumerate(s.spec.gp_dims):   # leave the shared solver with alpha = 0 GPs
        _load(s, g, R.synthetic_gp(50, d, seed=60 + g, sf2=SF2, sn2=SN2), R.points(24, d, seed=61 + g))
