"""The SQP kernel's constraint tightening (gain table staged in LDS, variables split over the two
half-waves when H + 1 <= 32) vs the oracle's covariance recursion (MI355X only).

Per case: B = 3 instances, a first solve in which instance 1 observes a state outside its box
(status 4: its previous solution is marked invalid), then a second solve from feasible
observations.  The second solve tightens instances 0 and 2 from their previous trajectories and
leaves instance 1 untightened.  Its tightening (solution()[2]) is compared with
oracle.gpmpc_oracle.propagate_constraint_limits on the same previous trajectories at rtol 1e-9 /
atol 1e-13 (the tolerance of test_tightening_matches_reference_fixture: the kernel sums the
recursion as a convolution, in another order); instance 1's row must be exactly zero.

Shapes: odd and even term counts, H = 1 (one term), H + 1 = 32 (the half-wave boundary: H = 31
is the largest split horizon), every (NUNC, NB): quad2d (3, 8), cartpole (2, 5: an odd NB, unequal
halves), quad3d (its table does not fit in LDS: the global-memory loop).

Above the split layout (H >= 32: one lane per stage, every variable of a stage in its lane): H = 32
(quad2d's table of H NB NUNC = 768 entries fills the first pass of the staging loop exactly),
H = 33 and 48 (the loop's second pass, "the rest of the table"; for cartpole the table stays
within one pass up to H = 63), H = 63 (all 64 lanes) and quad3d at its longest horizon, H = 47.
With the second pass's store removed the quad2d cases at H >= 33 fail and every shorter one passes
(profiles/r17/README.md).
"""

import numpy as np
import pytest

from helpers import O, initial_states, lqr, oracle_gps, problem, product_gps

pytestmark = pytest.mark.gpu

CASES = [("quad2d", 30, 1), ("quad2d", 30, 2), ("quad2d", 30, 5), ("quad2d", 40, 30), ("quad2d", 40, 31),
         ("cartpole", 20, 2), ("cartpole", 30, 11), ("cartpole", 30, 20), ("quad3d", 24, 8),
         ("quad2d", 40, 32), ("quad2d", 40, 33), ("quad2d", 40, 48), ("quad2d", 40, 63),
         ("cartpole", 30, 32), ("cartpole", 30, 63), ("quad3d", 24, 47)]


@pytest.mark.parametrize("name,N,H", CASES)
def test_tightening_matches_oracle_recursion(name, N, H):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpmpc.solver import BatchSolver

    B, prob = 3, 0.95
    spec, data, hyp = problem(name, N)
    mats = lqr(spec)
    gs = BatchSolver(spec, H, B)
    gs.set_gps(product_gps(data, hyp))
    gs.set_tightening(True, prob, *mats)
    gs.reset(reset_iterate=True)
    x0, ph = initial_states(spec, spec.reference_trajectory(), B)
    bad = x0.copy()
    j = int(np.flatnonzero(np.isfinite(spec.x_hi))[0])
    bad[1, j] = spec.x_hi[j] + 0.1                         # instance 1: outside its box
    ts = torch.tensor(ph, dtype=torch.int32, device="cuda")
    gs.solve(torch.tensor(bad, device="cuda"), ts)
    st = gs.status.cpu().numpy()
    assert st[0] in (0, 2) and st[1] == 4 and st[2] in (0, 2), st
    xp, up, _ = (t.cpu().numpy() for t in gs.solution())  # the previous trajectories
    gs.solve(torch.tensor(x0, device="cuda"), ts + 1)
    tight = gs.solution()[2].cpu().numpy()                 # (B, H + 1, nx + nu)
    nx, nu = spec.nx, spec.nu
    sd = spec.to_dict()
    gpo = oracle_gps(data, hyp)
    for b in (0, 2):
        sc, ic = O.propagate_constraint_limits(sd, gpo, xp[b].T, up[b].T, *mats, prob)
        err_x = np.abs(tight[b, :, :nx] + sc[:nx].T).max()
        err_u = np.abs(tight[b, :H, nx:] + ic[:nu].T).max()
        print(f"{name} H={H} b={b}: max |dx| {err_x:.3e} (scale {np.abs(sc).max():.3e}), max |du| {err_u:.3e}")
        np.testing.assert_allclose(tight[b, :, :nx], -sc[:nx].T, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(tight[b, :H, nx:], -ic[:nu].T, rtol=1e-9, atol=1e-13)
        if H > 1:
            assert tight[b, 1:, :nx].max() > 0.0           # (the comparison is not of zeros)
    assert not tight[1].any()                              # no previous solution: exactly zero
