"""The one-wave Riccati factorisation stage (mfma_backward_h) at short horizons (MI355X only).

The factorisation peels its first stage (H - 1) off a loop that takes two stages per pass, with a
single trailing stage when H - 1 is odd.  The launch-shape comparison of test_gpu_launch.py
(closed loop against the C++ restatement at KKT tolerance 1e-9: identical status, x and u within
1e-6 (1 + |.|)) is run here at waves = 1, B = 12, 4 steps, at horizons that take every arm:
H = 3 (peeled stage + one pass), H = 4 (+ the trailing stage), H = 5 (two passes), and H = 2 for
cartpole (peeled stage + the trailing stage only); quad2d has NU = 2 (2 x 2 inverse of Ru by the
adjugate), cartpole NU = 1 (scalar reciprocal).

all_converge is a condition on the inputs: the C++ restatement alone, on the CPU, reaches status 0
at every instance-step of the shapes below.  Dropped: quad2d N = 60 H = 2, where one of the 12
instances stops at the SQP iteration limit (status 2) at step 0.
"""

import pytest

from test_gpu_launch import _run_against_cpp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,N,H", [("quad2d", 60, 3), ("quad2d", 60, 4), ("quad2d", 60, 5),
                                      ("cartpole", 40, 2), ("cartpole", 40, 3), ("cartpole", 40, 11)])
def test_factor_stage_short_horizons_match_cpp_restatement(name, N, H):
    _run_against_cpp(name, N, H, 12, 4, 1, all_converge=True)
