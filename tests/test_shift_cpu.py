"""The numpy restatement of the one-stage shifted warm start (shift_util.shift_cpuref) on the C++
CPU restatement, tightening off, KKT 1e-9 (qp_tol 1e-11, qp_max_iter 100): it guards the helper the
GPU tests of GPMPC_TUNE_SHIFT compare against.

* converged: the shifted and the unshifted closed loop solve the same NLPs, so every solve ends
  with status 0 and x, u agree within 1e-6 (1 + |.|) at every step;
* one SQP iteration (max_iter = 1): the result is one QP step from the start point, so the two
  loops must differ, by at least 1e-3 relative at every step >= 1 (the helper does shift).
"""

import pytest

from shift_util import SMALL, oracle_loop, rel_gap


def _need_cpu_ref():
    from oracle import cpu_ref

    if not cpu_ref.LIB_PATH.exists():
        pytest.skip("oracle/lib/libcpuref.so not built (make -C oracle)")


@pytest.mark.parametrize("shape", SMALL, ids=[s[0] for s in SMALL])
def test_shifted_oracle_converges_to_the_same_solution(shape):
    _need_cpu_ref()
    base = oracle_loop(*shape)
    sh = oracle_loop(*shape, shift=True, obs_from=shape)
    assert (base["status"] == 0).all() and (sh["status"] == 0).all(), (base["status"], sh["status"])
    for s in range(shape[4]):
        gap = max(rel_gap(sh["x"][s], base["x"][s]), rel_gap(sh["u"][s], base["u"][s]))
        print(f"{shape[0]} step {s}: shifted vs unshifted {gap:.3e}, sqp_iter {base['sqp_iter'][s].mean():.2f} -> "
              f"{sh['sqp_iter'][s].mean():.2f}")
        assert gap <= 1e-6, (s, gap)


@pytest.mark.parametrize("shape", SMALL, ids=[s[0] for s in SMALL])
def test_one_iteration_shows_the_shift(shape):
    _need_cpu_ref()
    base = oracle_loop(*shape, max_iter=1, obs_from=shape)
    sh = oracle_loop(*shape, max_iter=1, shift=True, obs_from=shape)
    assert (base["status"] == 2).all() and (sh["status"] == 2).all(), (base["status"], sh["status"])
    for s in range(1, shape[4]):
        gap = max(rel_gap(sh["x"][s], base["x"][s]), rel_gap(sh["u"][s], base["u"][s]))
        print(f"{shape[0]} step {s}: one-iteration shifted vs unshifted {gap:.3e}")
        assert gap >= 1e-3, (s, gap)
