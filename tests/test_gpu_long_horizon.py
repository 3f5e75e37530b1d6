"""The SQP kernel at horizons 32 to 63 against references (MI355X only).

gpmpc_create accepts every horizon in [1, 63] that fits the 160 KB LDS budget, and above H = 31 the
kernel runs code the shorter horizons never reach (the parity section's table of horizon
against code path): the one-lane-per-stage layout instead of the split one (H + 1 > 32), the second
pass of the tightening gain table's staging loop (H NB NUNC > 768: quad2d H >= 33), three GP
evaluation tiles (H 33 .. 48) and four (H >= 49), more than 64 KB of dynamic LDS on one wave
(quad2d H >= 49), all 64 lanes (H = 63, the terminal stage in lane 63) and quad3d's LDS budget
(H = 47 is its longest horizon).

* Closed loop against the C++ restatement (oracle/cpu_ref.cpp) at quad2d / cartpole H = 32, 33, 48,
  49, 63 on every launch shape, and quad3d H = 47: B = 6, three steps at KKT tolerance 1e-9.  The
  comparison is that of _run_against_cpp in tests/test_gpu_launch.py without its allowance for
  borderline instances, plus the SQP iteration counts: status and sqp_iter equal, every instance
  at status 0, |x - x_cpp| and |u - u_cpp| <= 1e-6 (1 + |.|) for every instance.  The C++ side alone
  converges every instance of every step of each (model, H) in 3 to 13 SQP iterations (checked on
  the CPU before the list was fixed), and it runs once per (model, N, H): the plant moves with its
  u0, so its closed loop does not depend on the GPU and every launch shape sees the same
  observations.
* The certificate of tests/kkt_ref.py on the GPU's own solution and the bounds of its own
  tightening, with the oracle's dynamics: independent of both solvers.
* The knobs overlap and order at quad2d H = 63, where the LDS layout leaves one instance per CU:
  bit-identical outputs.
* The horizon limits of gpmpc_create.
"""

import functools

import numpy as np
import pytest

import kkt_ref
from helpers import O, initial_states, lqr, oracle_gps, problem, product_gps

pytestmark = pytest.mark.gpu

B, STEPS, TOL, QP_TOL, QP_MAX_ITER = 6, 3, 1e-9, 1e-11, 100
N_TRAIN = {"quad2d": 60, "cartpole": 40, "quad3d": 60}
HORIZONS = (32, 33, 48, 49, 63)
SHAPES = ((1, 0), (2, 0), (4, 0), (2, 1), (4, 1))
CLOSED_LOOP = [pytest.param(name, H, w, g, id=f"{name}-H{H}-w{w}s{g}")
               for name in ("quad2d", "cartpole") for H in HORIZONS for w, g in SHAPES]
CLOSED_LOOP.append(pytest.param("quad3d", 47, 4, 0, id="quad3d-H47-w4s0"))
MODEL_IDS = {"quad2d": 0, "quad3d": 1, "cartpole": 2}   # gpmpc_mi355x.h
LDS_BUDGET = 160 * 1024


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@functools.lru_cache(maxsize=None)
def _cpp_run(name, H):
    """The C++ restatement's closed loop: per step (obs, status, sqp_iter, x, u).  Read only."""
    from oracle import cpu_ref

    spec, data, hyp = problem(name, N_TRAIN[name])
    ref = cpu_ref.CpuRef(spec, H, B, gps=oracle_gps(data, hyp), lqr_mats=lqr(spec), tol=TOL, qp_tol=QP_TOL,
                         qp_max_iter=QP_MAX_ITER)
    x0, phase = initial_states(spec, spec.reference_trajectory(), B)
    plant = O.Dynamics(spec.to_dict(), None, params=spec.true_params)
    out = []
    for s in range(STEPS):
        u0 = ref.step(x0, phase + s, threads=4).copy()
        out.append(tuple(np.array(a) for a in (x0, ref.status, ref.sqp_iter, ref.x, ref.u)))
        for a in out[-1]:
            a.setflags(write=False)
        x0 = np.array([plant.rk4(x0[b], u0[b])[0] for b in range(B)])
    return phase, out


def _gpu_solver(name, H, waves=None, seg=None):
    from gpmpc.solver import BatchSolver

    spec, data, hyp = problem(name, N_TRAIN[name])
    gs = BatchSolver(spec, H, B, tol=TOL, qp_tol=QP_TOL, qp_max_iter=QP_MAX_ITER)
    if waves is not None:
        gs.set_launch(waves=waves)
        gs.set_tuning(seg=seg)
    gs.set_gps(product_gps(data, hyp))
    gs.set_tightening(True, 0.95, *lqr(spec))
    gs.reset(reset_iterate=True)
    return spec, data, hyp, gs


def _run_against_cpp(name, H, waves=None, seg=None):
    """The GPU on the observations of the C++ closed loop; every instance of every step compared."""
    torch = _torch()
    from oracle import cpu_ref

    if not cpu_ref.LIB_PATH.exists():
        pytest.skip("oracle/lib/libcpuref.so not built")
    phase, run = _cpp_run(name, H)
    spec, data, hyp, gs = _gpu_solver(name, H, waves, seg)
    for s, (obs, cst, cit, cx, cu) in enumerate(run):
        gs.solve(torch.tensor(obs, device="cuda"), torch.tensor(phase + s, dtype=torch.int32, device="cuda"))
        xg, ug, _ = (t.cpu().numpy() for t in gs.solution())
        st, it = gs.status.cpu().numpy(), gs.sqp_iter.cpu().numpy()
        ex = np.abs(xg - cx).max(axis=(1, 2)) / (1 + np.abs(cx).max(axis=(1, 2)))
        eu = np.abs(ug - cu).max(axis=(1, 2)) / (1 + np.abs(cu).max(axis=(1, 2)))
        print(f"{name} H={H} waves={waves} seg={seg} step {s}: status gpu {st.tolist()} cpu {cst.tolist()}, sqp_iter gpu "
              f"{it.tolist()} cpu {cit.tolist()}, max rel |dx| {ex.max():.3e} |du| {eu.max():.3e}")
        assert (cst == 0).all(), (s, cst)                 # the reference itself converges everywhere
        np.testing.assert_array_equal(st, cst)
        assert (st == 0).all(), (s, np.bincount(st, minlength=5))
        np.testing.assert_array_equal(it, cit)
        assert ex.max() <= 1e-6 and eu.max() <= 1e-6, (s, ex, eu)   # every instance
    return spec, data, hyp, gs, (phase, run[-1][0])


@pytest.mark.parametrize("name,H,waves,seg", CLOSED_LOOP)
def test_long_horizon_closed_loop_matches_cpp_restatement(name, H, waves, seg):
    """H = 32: the first non-split horizon (quad2d's gain table fills its first pass exactly); 33 and
    48: three evaluation tiles and the table's second pass; 49: four tiles, and quad2d's one-wave
    layout passes 64 KB of dynamic LDS; 63: lane 63.  quad3d H = 47: its longest horizon."""
    *_, gs, _ = _run_against_cpp(name, H, waves, seg)
    info = gs.launch_info()
    segments = 1 if seg == 0 else (3 if waves == 4 else 2)
    assert info["waves"] == waves and info["segments"] == segments, info


@pytest.mark.parametrize("name,H", [("quad2d", 63), ("cartpole", 63), ("quad3d", 47)])
def test_long_horizon_solution_has_a_kkt_certificate(name, H):
    """Instance 0 of the last step on the default launch shape: the dynamics residual and the bound
    violation of the GPU's (x, u) against the bounds of its own tightening are <= 1e-9, and some
    multipliers (found by the certificate itself) leave a stationarity residual <= 2 sqrt(n) 1e-9,
    n = H (nx + nu): the bound kkt_ref's docstring derives."""
    spec, data, hyp, gs, (phase, obs) = _run_against_cpp(name, H)
    sd = spec.to_dict()
    nx, nu = spec.nx, spec.nu
    xs, us, tight = (t.cpu().numpy() for t in gs.solution())
    assert tight[0, 1:, :nx].max() > 0.0                   # (a tightened step)
    sc = -np.concatenate([tight[0, :, :nx].T, tight[0, :, :nx].T])    # (2 nx, H + 1), as the oracle signs it
    ic = -np.concatenate([tight[0, :H, nx:].T, tight[0, :H, nx:].T])
    bounds = O.stage_bounds(sd, sc, ic, -1e-8)
    win = O.reference_window(spec.reference_trajectory(), int(phase[0]) + STEPS - 1, H)
    cert = kkt_ref.certificate(sd, O.Dynamics(sd, oracle_gps(data, hyp)), xs[0], us[0], *bounds, win, x0=obs[0])
    bound = 2 * np.sqrt(H * (nx + nu)) * TOL
    print(f"{name} H={H} certificate: eq {cert.eq:.3e} viol {cert.viol:.3e} stat {cert.stat:.3e} (bound {bound:.3e}), "
          f"active {int(cert.act_lo.sum())}+{int(cert.act_hi.sum())}, max tightening {tight[0].max():.3e}")
    assert cert.eq <= TOL and cert.viol <= TOL, (cert.eq, cert.viol)
    assert cert.stat <= bound, (cert.stat, bound)


def test_overlap_and_order_are_bit_exact_at_one_instance_per_cu():
    """quad2d at H = 63 holds one instance per CU (its two-wave layouts take 95 936 bytes, and
    123 616 with the segment solve), so a batch just above the CU count runs as overlapped halves in
    cost order, on the non-split kernels.  Against overlap = 0 and, separately, order = 0 on the same
    closed loop every output is bit-identical (as test_overlapped_step_is_bit_exact and
    test_cost_ordered_dispatch_is_bit_exact hold at H <= 30 and quad3d)."""
    torch = _torch()
    from gpmpc.solver import BatchSolver

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    name, H, batch, steps = "quad2d", 63, n_cu + 37, 2
    spec, data, hyp = problem(name, N_TRAIN[name])
    mats = lqr(spec)
    gpp = product_gps(data, hyp)
    x0, ph = initial_states(spec, spec.reference_trajectory(), batch)
    outs = []
    for tuning in ({}, {"overlap": 0}, {"order": 0}):
        gs = BatchSolver(spec, H, batch)
        gs.set_tuning(**tuning)
        gs.set_gps(gpp)
        gs.set_tightening(True, 0.95, *mats)
        gs.reset(reset_iterate=True)
        assert gs.launch_info()["overlapped"] == ("overlap" not in tuning), (tuning, gs.launch_info())
        obs = torch.tensor(x0, device="cuda")
        ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
        rec = []
        for k in range(steps):
            u = gs.solve(obs, ts + k)
            rec += [u.clone(), gs.status.clone(), gs.sqp_iter.clone(), gs.qp_iter.clone(), gs.res.clone()]
            rec += [t.clone() for t in gs.solution()[:2]]
            obs = gs.plant_step(obs, u, ts + k)
        outs.append([t.cpu() for t in rec])
        st = torch.cat(outs[-1][1::7])
        print(f"quad2d H=63 B={batch} {tuning or 'default'}: status census {np.bincount(st.numpy(), minlength=5).tolist()}")
        assert (st == 0).float().mean() > 0.9              # a healthy closed loop
    for other in outs[1:]:
        for i, (a, b) in enumerate(zip(outs[0], other)):
            assert torch.equal(a, b), i


def test_lds_bytes_grow_with_the_horizon():
    _torch()
    from gpmpc import _lib

    lib = _lib.load()
    for name, model in MODEL_IDS.items():
        v = [lib.gpmpc_lds_bytes(model, H) for H in range(1, 64)]
        assert all(0 < a <= b for a, b in zip(v, v[1:])), (name, v)


def _one_step_status(name, H):
    torch = _torch()
    spec, _, _, gs = _gpu_solver(name, H)
    x0, ph = initial_states(spec, spec.reference_trajectory(), B)
    gs.solve(torch.tensor(x0, device="cuda"), torch.tensor(ph, dtype=torch.int32, device="cuda"))
    return gs.status.cpu().numpy()


def test_horizon_limits_of_create():
    """gpmpc_create takes H = 63 for quad2d and cartpole and quad3d's largest horizon within the
    160 KB LDS budget, 47 by gpmpc_lds_bytes (163 672 bytes; 48 needs 167 104).  H = 0, H = 64 and
    quad3d one stage above its limit are refused with a message that names the horizon range or the
    LDS budget, and a create after the refusals solves."""
    _torch()
    from gpmpc import _lib
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver

    lib = _lib.load()
    q3max = max(H for H in range(1, 64) if lib.gpmpc_lds_bytes(MODEL_IDS["quad3d"], H) <= LDS_BUDGET)
    assert q3max == 47, q3max
    for name, H in (("quad2d", 63), ("cartpole", 63), ("quad3d", q3max)):
        spec = get_spec(name)
        assert spec.model_id == MODEL_IDS[name]
        assert BatchSolver(spec, H, 2).H == H
    for name in MODEL_IDS:
        for H in (0, 64):
            with pytest.raises(_lib.GPMPCError, match=r"horizon must be in \[1, 63\]"):
                BatchSolver(get_spec(name), H, 2)
    with pytest.raises(_lib.GPMPCError, match="LDS budget"):
        BatchSolver(get_spec("quad3d"), q3max + 1, 2)
    assert (_one_step_status("quad2d", 63) == 0).all()
