"""Horizons at which the Riccati factorisation's stage loop changes shape (MI355X only).

mfma_backward_h peels its first stage and then runs two stages per pass, and the one-wave kernels
form its per-lane LDS streams from compile-time lane masks (csrc/sqp_kernel.hip, LanePlan; the masks
themselves are checked against the case-by-case expressions by a static_assert per model, at build
time).  The launch-shape tests cover H = 10 .. 30; here the closed loop runs against the C++
restatement, with the comparison and tolerances of test_gpu_launch._run_against_cpp, at

  H = 2, 3    the peeled stage, then an even or an odd remainder of the two-stage loop,
  H = 31      the last horizon of the split IPM layout (lanes 31 and 63 hold a stage),
  H = 32      the first horizon of the one-lane-per-stage layout,

for quad2d (NU = 2) and cartpole (NU = 1) on one wave, and H = 3 and 31 on two and four waves with and
without segments, where the factorisation keeps the case-by-case set-up.
"""

import pytest

from test_gpu_launch import _run_against_cpp

pytestmark = pytest.mark.gpu

B, STEPS, N = 6, 3, 40


@pytest.mark.parametrize("H", [2, 3, 31, 32])
@pytest.mark.parametrize("name", ["quad2d", "cartpole"])
def test_one_wave_horizons_match_cpp_restatement(name, H):
    _run_against_cpp(name, N, H, B, STEPS, waves=1)


@pytest.mark.parametrize("waves,seg", [(2, 0), (4, 0), (2, 1), (4, 1)])
@pytest.mark.parametrize("H", [3, 31])
@pytest.mark.parametrize("name", ["quad2d", "cartpole"])
def test_multi_wave_horizons_match_cpp_restatement(name, H, waves, seg):
    _run_against_cpp(name, N, H, B, STEPS, waves=waves, seg=seg)
