"""The device's LOVE root algorithm (gpmpc_gp_love_root, csrc/gp_love.hip) as its numpy model
(love_device_ref.py) states it, against the host algorithm (oracle.lanczos_love_root) on the same Khat
and start vector: the bidiagonal root gives the eigendecomposition root's variances, is an inverse
root of Khat on the Krylov space, has the oracle's rank, reports a pivot that is not positive, and
leaves inert rows out."""

from functools import lru_cache

import numpy as np
import pytest
import torch

import love_device_ref as LR
from helpers import O, oracle_gps, problem

CASES = [("quad2d", 40, 8), ("quad2d", 48, 20), ("quad2d", 200, 50), ("cartpole", 50, 100)]


def start_vector(n, seed=0):
    """The draw of GaussianProcess.love_root(seed=seed)."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randn(n, dtype=torch.float64, generator=gen).numpy()


def points(og, seed=5):
    """64 points near the training rows and 64 drawn N(0, 0.5^2)."""
    rng = np.random.default_rng(seed)
    N, d = og.X.shape
    near = og.X[rng.integers(0, N, 64)] + rng.normal(scale=0.1, size=(64, d))
    return near, rng.normal(scale=0.5, size=(64, d))


@lru_cache(maxsize=None)
def case(name, N):
    _, data, hyp = problem(name, N)
    return oracle_gps(data, hyp)


@pytest.mark.parametrize("name,N,rank", CASES)
def test_model_root_matches_the_host_root(name, N, rank):
    for g, og in enumerate(case(name, N)):
        q0 = start_vector(N)
        R_o = O.lanczos_love_root(og.K, rank, q0)
        R, m, ok = LR.love_root(og.K, rank, q0)
        assert ok == 1 and R.shape == (N, m)
        assert m == R_o.shape[1], (g, m, R_o.shape)
        np.testing.assert_allclose(R.T @ og.K @ R, np.eye(m), rtol=0, atol=1e-8)
        for Z in points(og):
            err = np.abs(O.love_var(og, R, Z) - O.love_var(og, R_o, Z)).max()
            assert err <= 1e-10 * og.sf2, (g, err, og.sf2)


def test_pivot_that_is_not_positive_reports_failure():
    # T = [[1, 2], [2, 1]] is indefinite: the second pivot is 1 - 4 < 0
    assert LR.bidiagonal_factor(np.array([1.0, 1.0]), np.array([2.0]))[2] == 0
    assert LR.bidiagonal_factor(np.array([1.0, np.nan]), np.array([0.5]))[2] == 0
    assert LR.bidiagonal_factor(np.array([0.0]), np.array([]))[2] == 0
    c, l, ok = LR.bidiagonal_factor(np.array([4.0, 5.0]), np.array([2.0]))
    assert ok == 1
    np.testing.assert_allclose((c, l), ([2.0, 2.0], [0.0, 1.0]), rtol=0, atol=0)
    # a Khat that is not positive definite on the Krylov space: no root
    K = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    R, m, ok = LR.love_root(K, 3, np.array([1.0, 0.0, 0.0]))
    assert ok == 0 and R is None


@pytest.mark.parametrize("name,N,rank", [("quad2d", 48, 20), ("cartpole", 50, 100)])
def test_inert_rows_take_no_part(name, N, rank):
    rng = np.random.default_rng(11)
    inert = np.zeros(N, dtype=bool)
    inert[rng.choice(N, 9, replace=False)] = True
    live = np.flatnonzero(~inert)
    for g, og in enumerate(case(name, N)):
        q0 = start_vector(N)
        qn = q0.copy()
        qn[inert] = np.nan
        R, m, ok = LR.love_root(og.K, rank, qn, inert)
        assert ok == 1 and m <= min(rank, live.size)
        assert (R[inert] == 0.0).all()
        R_l = O.lanczos_love_root(og.K[np.ix_(live, live)], rank, q0[live])
        assert m == R_l.shape[1]
        R_o = np.zeros((N, m))
        R_o[live] = R_l
        for Z in points(og):
            err = np.abs(O.love_var(og, R, Z) - O.love_var(og, R_o, Z)).max()
            assert err <= 1e-10 * og.sf2, (g, err)
