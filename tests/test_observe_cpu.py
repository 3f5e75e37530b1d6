"""Training data on the device, the parts that need no GPU: the numpy reference of gpmpc_gp_informative's score
and counting rank (tests/observe_ref.py) on hand-made vectors, and the build plumbing of gp_observe.hip and the
three entry points (gpmpc_preprocess, gpmpc_gp_informative, gpmpc_gp_observe)."""

import ctypes
import re
from pathlib import Path

import numpy as np

import observe_ref as OR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmpc_mi355x.h"
NAN, INF = float("nan"), float("inf")


def test_rank_rule_on_hand_made_scores():
    #            0    1    2    3     4    5    6     7
    s = np.array([0.5, 2.0, NAN, 2.0, -INF, 0.5, INF, 0.25])
    # finite ones by decreasing score, ties to the lower index; then the non-finite ones by index
    want = [1, 3, 0, 5, 7, 2, 4, 6]
    for m in (1, 2, 5, 8):
        assert OR.rank(s, m).tolist() == want[:m]
    assert OR.rank(np.array([NAN]), 1).tolist() == [0]
    assert OR.rank(np.array([1.0, 1.0, 1.0]), 3).tolist() == [0, 1, 2]
    assert OR.rank(np.array([0.0, -0.0, 1e-300]), 3).tolist() == [2, 0, 1]   # (0.0 == -0.0: a tie)


def test_rank_rule_agrees_with_a_stable_sort():
    rng = np.random.default_rng(5)
    for P in (1, 7, 64, 130):
        s = rng.integers(0, 6, P).astype(np.float64)   # many ties
        s[rng.integers(0, P, max(P // 8, 1))] = NAN
        s[rng.integers(0, P, max(P // 16, 1))] = INF
        fin = np.isfinite(s)
        order = sorted(range(P), key=lambda i: (not fin[i], -s[i] if fin[i] else 0.0, i))
        assert OR.rank(s, P).tolist() == order


def test_score_is_the_largest_scaled_variance_and_keeps_nan():
    var = np.array([[1.0, 4.0, NAN, 0.5], [3.0, 2.0, 1.0, NAN]])
    got = OR.score(var, [2.0, 4.0])
    np.testing.assert_array_equal(got[:2], [0.75, 2.0])
    assert np.isnan(got[2]) and np.isnan(got[3])


def _decl(name):
    m = re.search(rf"gpmpc_status\s+{name}\(([^)]*)\)\s*;", HEADER.read_text())
    assert m, f"{name} is not declared in the header"
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_header_and_signature_table_hold_the_three_entry_points():
    from gpmpc import _lib

    P, I, Dd = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    cd, ci = "const double*", "const int32_t*"
    assert _decl("gpmpc_preprocess") == ["gpmpc_handle*", "int32_t", cd, cd, cd, "int32_t", ci, "double", "double",
                                         "double*", "double*", "void*"]
    assert _lib.SIGNATURES["gpmpc_preprocess"] == (I, [P, I, P, P, P, I, P, Dd, Dd, P, P, P])
    assert _decl("gpmpc_gp_informative") == ["gpmpc_handle*", "int32_t", cd, cd, "int32_t", "int32_t*", "double*", "void*"]
    assert _lib.SIGNATURES["gpmpc_gp_informative"] == (I, [P, I, P, P, I, P, P, P])
    assert _decl("gpmpc_gp_observe") == ["gpmpc_handle*", "int32_t", cd, cd, cd, "int32_t", ci, "double", "double",
                                         "int32_t", "double*", "double*", "int32_t*", "int32_t*", "void*"]
    assert _lib.SIGNATURES["gpmpc_gp_observe"] == (I, [P, I, P, P, P, I, P, Dd, Dd, I, P, P, P, P, P])


def test_gp_observe_hip_is_built_last_and_hashed_in_the_same_position():
    from gpmpc import _lib

    mk = (ROOT / "gp-mpc_amd" / "csrc" / "Makefile").read_text()
    srcs = [f for line in re.findall(r"^SRCS \+?= (.*)$", mk, re.M) for f in line.split()]
    hashed = re.search(r"^HASHED = (.*)$", mk, re.M).group(1).split()
    assert srcs[-1] == "gp_observe.hip" and srcs.count("gp_observe.hip") == 1
    assert hashed == _lib.HASHED
    assert hashed.index("gp_observe.hip") == _lib.HASHED.index("gp_observe.hip") == hashed.index("gp_fitc.hip") + 1
    assert (ROOT / "gp-mpc_amd" / "csrc" / "gp_observe.hip").is_file()


def test_python_surface_exists():
    import inspect

    from gpmpc.gpmpc import GPMPC
    from gpmpc.learning import run_online_episode
    from gpmpc.solver import BatchSolver

    assert list(inspect.signature(BatchSolver.informative).parameters)[1:] == ["x", "u", "m", "scores"]
    assert {"x", "u", "x_next", "pick"} <= set(inspect.signature(BatchSolver.preprocess).parameters)
    assert {"pick", "m", "evict_oldest"} <= set(inspect.signature(BatchSolver.observe).parameters)
    assert {"pick", "m", "select", "evict_oldest"} <= set(inspect.signature(GPMPC.observe).parameters)
    sig = inspect.signature(run_online_episode).parameters
    assert sig["device_data"].default is False and sig["select"].default == "random"
