"""The checker of tests/test_gpu_gp_kernels.py, checked where no GPU is needed: the
extended-precision reference (tests/gp_ref.py) against the CPU oracle on real GP fits, and its
error bound against a plain float64 evaluation of the same synthetic operands."""

import numpy as np
import pytest

import gp_ref as R
from helpers import O, oracle_gps, problem

pytestmark = pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64")


@pytest.mark.parametrize("name,N", [("quad2d", 40), ("cartpole", 30)])
def test_reference_matches_oracle_on_a_real_fit(name, N):
    """Mean, exact variance and LOVE variance of the longdouble reference vs oracle.ExactGP.mean /
    .var and O.love_var, to 1e-12 relative to the operands' scale (sf2 for the variances,
    sf2 sum|alpha| for the mean, the scales of tests/test_gpu_parity.py).  The factor's inverse is
    taken in longdouble from the oracle's float64 Cholesky factor; relative to the values
    themselves the oracle's own float64 cancellation (cond K ~ 1e7 here) is the larger error."""
    spec, data, hyp = problem(name, N)
    rng = np.random.default_rng(3)
    for g, gp in enumerate(oracle_gps(data, hyp)):
        X = gp.X
        Z = X[rng.integers(0, N, 50)] + 0.3 * gp.ell * rng.standard_normal((50, X.shape[1]))
        ref = R.reference(X, gp.ell, gp.sf2, Z, alpha=gp.alpha, B=R.inv_lower_ld(gp.L).T)
        assert np.abs(gp.var(Z, with_noise=False) - ref["var"]).max() <= 1e-12 * gp.sf2, g
        assert np.abs(gp.var(Z, with_noise=True) - (ref["var"] + gp.sn2)).max() <= 1e-12 * gp.sf2, g
        assert np.abs(gp.mean(Z) - ref["mean"]).max() <= 1e-12 * gp.sf2 * np.abs(gp.alpha).sum(), g
        root = O.lanczos_love_root(gp.K, 12, np.random.default_rng(0).standard_normal(N))
        love = R.reference(X, gp.ell, gp.sf2, Z, B=root)
        assert np.abs(O.love_var(gp, root, Z, with_noise=False) - love["var"]).max() <= 1e-12 * gp.sf2, g


@pytest.mark.parametrize("n,d", [(1, 1), (17, 2), (100, 3), (257, 1), (300, 3)])
def test_bound_covers_a_float64_evaluation(n, d):
    """On the synthetic operands the bound is at least the error of a plain float64 numpy
    evaluation (one more admissible summation order), for the exact factor and for a dense root;
    the operands have the advertised shape: kernel values in [KMIN, 1] sf2, variance >= sf2 / 2."""
    gp = R.synthetic_gp(n, d, seed=n + d, sf2=1e-3, sn2=1e-6)
    Z = R.points(40, d, seed=5)
    k = R.kernel_ld(gp["X"], gp["ell"], gp["sf2"], Z)
    assert k.min() >= R.KMIN * gp["sf2"] and k.max() <= gp["sf2"]
    ref = R.reference(gp["X"], gp["ell"], gp["sf2"], Z, alpha=gp["alpha"], B=gp["Linv"].T, frac=0.4)
    f = ref["scale"]
    assert np.log2(f) == np.round(np.log2(f))          # a power of two: f * Linv is exact
    assert ref["var"].min() >= 0.5 * gp["sf2"]
    assert (ref["var"] < gp["sf2"]).all() and (ref["tol_var"] > 0).all() and (ref["tol_mean"] > 0).all()
    got = R.numpy64(gp["X"], gp["ell"], gp["sf2"], Z, alpha=gp["alpha"], B=f * gp["Linv"].T)
    assert (np.abs(got["var"] - ref["var"]) <= ref["tol_var"]).all()
    assert (np.abs(got["mean"] - ref["mean"]) <= ref["tol_mean"]).all()
    # the same reference computed from the scaled operand itself
    direct = R.reference(gp["X"], gp["ell"], gp["sf2"], Z, B=f * gp["Linv"].T)
    assert np.array_equal(direct["var"], ref["var"])
    root = R.synthetic_root(n, min(n, 12), seed=9)
    love = R.reference(gp["X"], gp["ell"], gp["sf2"], Z, B=root, frac=0.4)
    got = R.numpy64(gp["X"], gp["ell"], gp["sf2"], Z, B=love["scale"] * root)
    assert love["var"].min() >= 0.5 * gp["sf2"]
    assert (np.abs(got["var"] - love["var"]) <= love["tol_var"]).all()
    # a dropped 16-row panel or 16-column tile is far outside the bound
    if n > 16:
        B = f * gp["Linv"].T
        for broken in (np.vstack([B[:-16], np.zeros((16, n))]), np.hstack([B[:, :-16], np.zeros((n, 16))])):
            bad = R.numpy64(gp["X"], gp["ell"], gp["sf2"], Z, B=broken)
            assert (np.abs(bad["var"] - ref["var"]) > 1e3 * ref["tol_var"]).all()
