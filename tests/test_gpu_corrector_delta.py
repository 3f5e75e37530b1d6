"""The IPM corrector solved as a delta system (sqp_kernel.hip, SqpKernel kCorrDelta) against the
C++ restatement (oracle/cpu_ref.cpp), which keeps the full re-solve of the corrector (MI355X only).

The one-wave single-tile MFMA kernels add the solution of the Newton system for the change of the
gradient (no dynamics residual, dx_0 = 0) to the affine step instead of solving the whole system
again (tests/test_corrector_delta_cpu.py is the numpy model).  The closed loop runs 4
steps at KKT tolerance 1e-9 with N = 50 training rows and B = 8 instances; comparison, tolerances
and the "every instance converged on both sides" condition are those of _run_against_cpp in
tests/test_gpu_launch.py, restated here: identical status, every instance at status 0, and
|x_gpu - x_cpu|, |u_gpu - u_cpu| <= 1e-6 (1 + |.|).

Cases: the shortest recurrence (H = 3: one interior stage), a short split layout (H = 5), the
headline horizon (30), the last split shape (H + 1 = 32), the one-lane-per-stage layout (H = 33),
NX = 4 / NU = 1 (cartpole, H = 11), and the four-wave MFMA path with seg = 0 (measured slower in
the delta form and left in the full re-solve: the case pins that the switch leaves it correct).
The C++ restatement alone converges every instance of every step of each of them (checked on the
CPU before the cases were fixed), so none stands in for another horizon.  The segment path and
quad3d keep the full re-solve; the existing suite covers them unchanged.
"""

import numpy as np
import pytest

from helpers import O, initial_states, lqr, oracle_gps, problem, product_gps

pytestmark = pytest.mark.gpu

N_TRAIN, BATCH, STEPS = 50, 8, 4
CASES = [("quad2d", 3, 1), ("quad2d", 5, 1), ("quad2d", 30, 1), ("quad2d", 31, 1), ("quad2d", 33, 1),
         ("cartpole", 11, 1), ("quad2d", 30, 4)]


def _run_against_cpp(name, N, H, B, steps, waves, seg=0):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpmpc.solver import BatchSolver
    from oracle import cpu_ref

    if not cpu_ref.LIB_PATH.exists():
        pytest.skip("oracle/lib/libcpuref.so not built")
    spec, data, hyp = problem(name, N)
    gpo, gpp = oracle_gps(data, hyp), product_gps(data, hyp)
    mats = lqr(spec)
    tol = 1e-9
    ref = cpu_ref.CpuRef(spec, H, B, gps=gpo, lqr_mats=mats, tol=tol, qp_tol=1e-11, qp_max_iter=100)
    gs = BatchSolver(spec, H, B, tol=tol, qp_tol=1e-11, qp_max_iter=100)
    gs.set_launch(waves=waves)
    gs.set_tuning(seg=seg)
    gs.set_gps(gpp)
    gs.set_tightening(True, 0.95, *mats)
    gs.reset(reset_iterate=True)
    traj = spec.reference_trajectory()
    x0, phase = initial_states(spec, traj, B)
    plant = O.Dynamics(spec.to_dict(), None, params=spec.true_params)
    for s in range(steps):
        gs.solve(torch.tensor(x0, device="cuda"), torch.tensor(phase + s, dtype=torch.int32, device="cuda"))
        u0 = ref.step(x0, phase + s, threads=4).copy()
        xg, ug, _ = (t.cpu().numpy() for t in gs.solution())
        st = gs.status.cpu().numpy()
        ex = np.abs(xg - ref.x).max(axis=(1, 2)) / (1 + np.abs(ref.x).max(axis=(1, 2)))
        eu = np.abs(ug - ref.u).max(axis=(1, 2)) / (1 + np.abs(ref.u).max(axis=(1, 2)))
        print(f"{name} H={H} waves={waves} step {s}: status gpu {st.tolist()} cpu {ref.status.tolist()}, "
              f"max rel |dx| {ex.max():.3e} |du| {eu.max():.3e}, qp_iter {gs.qp_iter.cpu().tolist()}")
        both = (st == 0) & (ref.status == 0)
        assert both.any() and max(ex[both].max(), eu[both].max()) <= 1e-6, (s, ex[both], eu[both])
        np.testing.assert_array_equal(st, ref.status)
        assert (st == 0).all(), (s, np.bincount(st, minlength=5))   # every instance reaches KKT 1e-9
        assert ex.max() <= 1e-6 and eu.max() <= 1e-6, (s, ex.max(), eu.max())
        for b in range(B):
            x0[b] = plant.rk4(x0[b], u0[b])[0]
    return gs


@pytest.mark.parametrize("name,H,waves", CASES)
def test_delta_corrector_matches_cpp_restatement(name, H, waves):
    gs = _run_against_cpp(name, N_TRAIN, H, BATCH, STEPS, waves, seg=0)
    info = gs.launch_info()
    assert info["waves"] == waves and info["segments"] == 1, info
