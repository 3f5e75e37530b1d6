"""numpy reference of gpmpc_gp_inducing (csrc/gp_observe.hip), the cases its tests share
(tests/test_gp_inducing_cpu.py, tests/test_gpu_inducing.py) and their margin.

The rule.  A GP's n training rows X, its prior covariance k(X, X) (no likelihood noise: K_ss has none), d_i = sf2
for every live row (an inert row is closed from the start, never picked, in no sum, its residual 0).  For
t = 0 .. M-1: the score s_i = d_i / sf2 of the open rows, j_t the largest finite score above tol (ties to the lower
index; none: the selection stops with count = t), then
    l_t[i] = (k(x_i, x_j) - sum_{s<t} l_s[i] l_s[j]) / sqrt(d_j),  d_i -= l_t[i]^2  for every live i,  row j closes.
This is a pivoted partial Cholesky of k(X, X), so the final d_i is sf2 - k(x_i, S) K_ss^-1 k(S, x_i) on the picks S,
and the diagonal of the Cholesky factor of K_ss in pick order is sqrt(gain sf2).

`greedy_ld` runs it in np.longdouble (gp_ref.kernel_ld) and also returns, per step, the gap between the best score
and the runner-up's (a row with the same inputs as the best one is no runner-up: that tie is exact and the index
decides it; step 0, where every score is exactly 1, is excluded for the same reason) and, for the stop decision,
the distance from tol of the last accepted gain and of the first refused best score.  `greedy_f64` is the float64
model in the kernel's summation order: the inner product sum_s l_s[i] l_s[j] in PARTS = 16 parts (part q: the
columns q, q + 16, ..), each a sequential sum, added as a balanced tree ((0 + 1) + (2 + 3)) + .. .

Criterion, the convention of gp_select_ref.py: with e_full the worst error over the rows of the float64 yardstick
sf2 - |L_S^-1 k(S, x_i)|^2 (a float64 Cholesky of k(S, S) on the reference's picks, gp_drop_ref._chol) against the
longdouble residuals, the selection's residuals must have a worst error of at most MARGIN_INDUCING e_full.

R_MODEL.  The worst e_model / e_full of `greedy_f64` over CASES (both GPs), measured with
tests/test_gp_inducing_cpu.py -s: 2.111, rounded up to R_MODEL = 2.12 (n = 40, gp0, M = 1, tol = 0: e_model 1.0e-15
against e_full 4.9e-16, one column whose yardstick happens to round well; 1.80 and 1.68 at n = 24, gp0, 0.16 .. 1.22
in the other cases, errors of 2e-16 .. 2.4e-15 throughout).  MARGIN_INDUCING = ceil(4 R_MODEL) = 9: the factor 4
covers the device's fused multiply-adds and its own exponential (the gp_drop_ref.py convention).

Gap condition.  The device's picks must equal `greedy_ld`'s wherever rounding cannot reorder two rows or move the
stop: at every step of every case the gap, and at the stop both distances from tol, must be at least
GAP_FACTOR = 1000 times the score error the criterion allows, MARGIN_INDUCING e_full / sf2.  Measured over CASES:
with tol = 1e-4 and M = n the counts are (6, 23), (6, 33), (6, 51) for (gp0, gp1) at n = 24, 40, 272; the smallest
gap after step 0 is 3.4e-7 (n = 272, gp0, step 5) against an allowed error of 8.7e-15 there, a factor 4e7; the
smallest stop margin is 3.7e-6 (n = 272, gp1, the last accepted gain).  The inert-row cases and the clustered rows
have gaps of at least 9.2e-7 and stop margins of at least 1.3e-5; DEEP, the case past 256 picks, has a smallest gap
of 2.8e-9 (step 259) against an allowed error of 5.3e-14, and a model ratio of 0.2.
"""

from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

import gp_drop_ref as D
import gp_ref as R
import gp_select_ref as S
from gp_pick_ref import PARTS, tree

LD = R.LD
R_MODEL = 2.12
MARGIN_INDUCING = float(math.ceil(4 * R_MODEL))
GAP_FACTOR = S.GAP_FACTOR
SF2 = S.SF2
NS = S.NS                  # 24 (a ragged tile), 40, 272 (more than 16 row blocks, t past 32)
TOL = 1e-4
# tol = 0: the m up to which the picks are comparable, per GP (GP 0's gains are rounding noise by step 16)
M_TOL0 = ((1, 6), (1, 17, 33))
# the ordering test: GP 0's lengthscale times this before the selection (the picks must differ)
ELL_SCALE = 1.3


def ms_tol0(g, n):
    return sorted({min(m, n) for m in M_TOL0[g]})


# (n, GP, M, tol): tol = TOL runs to the stop (M = n), tol = 0 takes exactly M rows
CASES = [(n, g, n, TOL) for n in NS for g in range(2)] + [(n, g, m, 0.0) for n in NS for g in range(2) for m in ms_tol0(g, n)]


def gp_of(n, g, scale=1.0):
    dg = S.case_data(n)[g]
    return dict(X=dg["X"][:n], y=dg["y"][:n], ell=dg["ell"] * scale, sf2=SF2[g], sn2=D.SN2, d=dg["d"])


def _same_inputs(X, j):
    return (X == X[j]).all(1)


def greedy_ld(X, ell, sf2, M, tol, live=None):
    """picks (count,) int32, gains (count,) float64, resid (n,) longdouble, gaps (count,) in score units (inf
    where there is no runner-up and at step 0), count, and the stop margins: `accepted` (last gain - tol) and
    `refused` (tol - the best score at the stop; inf when the selection ran to M or no row was left)."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    n = X.shape[0]
    live = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    K = R.kernel_ld(X, ell, sf2, X)
    sf2l, toll = LD(float(sf2)), LD(float(tol))
    d = np.where(live, sf2l, LD(0))
    open_ = live.copy()
    ls, picks, gains, gaps = [], [], [], []
    refused = np.inf
    for t in range(M):
        cand = np.flatnonzero(open_)
        if len(cand) == 0:
            break
        s = d / sf2l
        best = s[cand].max()
        if not (np.isfinite(best) and best > toll):
            refused = float(toll - best)
            break
        j = int(cand[np.flatnonzero(s[cand] == best)[0]])
        others = cand[~_same_inputs(X, j)[cand]]
        gaps.append(float(best - s[others].max()) if len(others) and t > 0 else np.inf)
        picks.append(j)
        gains.append(float(best))
        c = K[:, j].copy()
        for l in ls:
            c -= l * l[j]
        l = np.where(live, c / np.sqrt(d[j]), LD(0))
        ls.append(l)
        d = d - l * l
        open_[j] = False
    accepted = float(LD(gains[-1]) - toll) if gains else np.inf
    return dict(picks=np.array(picks, dtype=np.int32), gains=np.array(gains, dtype=np.float64), resid=d,
                gaps=np.array(gaps), count=len(picks), accepted=accepted, refused=refused, L=ls)


def greedy_f64(X, ell, sf2, M, tol, live=None):
    """The float64 model in the kernel's summation order: picks, gains, resid (n,), count."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    n = X.shape[0]
    live = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    d = np.where(live, float(sf2), 0.0)
    open_ = live.copy()
    ls, picks, gains = [], [], []
    for t in range(M):
        cand = np.flatnonzero(open_)
        if len(cand) == 0:
            break
        s = d / sf2
        best = s[cand].max()
        if not (np.isfinite(best) and best > tol):
            break
        j = int(cand[np.flatnonzero(s[cand] == best)[0]])
        picks.append(j)
        gains.append(float(best))
        parts = []
        for q in range(PARTS):
            acc = np.zeros(n)
            for c in range(q, t, PARTS):
                acc = acc + ls[c] * ls[c][j]
            parts.append(acc)
        k = D.kernel64(X[j:j + 1], ell, sf2, X)[:, 0]
        l = np.where(live, (k - tree(parts)) / math.sqrt(d[j]), 0.0)
        ls.append(l)
        d = d - l * l
        open_[j] = False
    return dict(picks=np.array(picks, dtype=np.int32), gains=np.array(gains), resid=d, count=len(picks))


def direct_ld(X, ell, sf2, picks, live=None):
    """sf2 - k(x_i, S) K_ss^-1 k(S, x_i) in longdouble by an unpivoted Cholesky of K_ss (0 for an inert row)."""
    from gp_append_ref import chol_ld, solve_lower_ld

    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    Sx = X[np.asarray(picks)]
    L = chol_ld(R.kernel_ld(Sx, ell, sf2, Sx))
    v = solve_lower_ld(L, R.kernel_ld(X, ell, sf2, Sx).copy())    # (M, n)
    out = LD(float(sf2)) - (v * v).sum(0)
    return (out if live is None else np.where(live, out, LD(0))), np.diag(L)


def yardstick(X, ell, sf2, picks, live=None):
    """The float64 yardstick on the reference's picks: sf2 - |L_S^-1 k(S, x_i)|^2 (0 for an inert row)."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    Sx = X[np.asarray(picks)]
    L, ok = D._chol(D.kernel64(Sx, ell, sf2, Sx))
    assert ok, "the yardstick's float64 Cholesky of k(S, S) lost a pivot"
    v = D._inv_lower(L) @ D.kernel64(X, ell, sf2, Sx)
    out = sf2 - (v * v).sum(0)
    return out if live is None else np.where(live, out, 0.0)


def e_full(X, ell, sf2, ref, live=None):
    return float(np.abs(yardstick(X, ell, sf2, ref["picks"], live) - ref["resid"]).max())


def allowed_score_error(sf2, e):
    """The score error the criterion allows: MARGIN_INDUCING e_full / sf2."""
    return MARGIN_INDUCING * e / sf2


@lru_cache(maxsize=None)
def case_ref(n, g, M, tol, scale=1.0):
    gp = gp_of(n, g, scale)
    return greedy_ld(gp["X"], gp["ell"], gp["sf2"], M, tol)


@lru_cache(maxsize=None)
def case_e_full(n, g, M, tol, scale=1.0):
    gp = gp_of(n, g, scale)
    return e_full(gp["X"], gp["ell"], gp["sf2"], case_ref(n, g, M, tol, scale))


# More picks than one chunk of the pick loop's staged pivot row holds (csrc/gp_observe.hip: 256 columns): GP 1 of the
# 272-row data at 0.4 of its lengthscale, where 264 picks have gains down to 5.4e-7 and gaps of at least 2.8e-9
# (5e4 times the allowed error); as case_ref's arguments
DEEP = (272, 1, 264, 0.0, 0.4)


# ------------------------------------------------------------------------------------------------ inert rows
INERT_N, INERT_BLOCK, INERT_NEW = 24, 16, 8


def inert_case(g, behind):
    """24 rows of the 40-row data, a rejected block of 16 and, with `behind`, an accepted block of the data's next
    8 rows: (X of every row with zeros on the inert ones, live mask, the accepted block's (X, y) or None)."""
    dg = S.case_data(40)[g]
    n = INERT_N + INERT_BLOCK + (INERT_NEW if behind else 0)
    X, live = np.zeros((n, dg["d"])), np.zeros(n, dtype=bool)
    X[:INERT_N], live[:INERT_N] = dg["X"][:INERT_N], True
    new = None
    if behind:
        rows = slice(INERT_N, INERT_N + INERT_NEW)
        X[INERT_N + INERT_BLOCK:], live[INERT_N + INERT_BLOCK:] = dg["X"][rows], True
        new = (dg["X"][rows], dg["y"][rows])
    return X, live, new


# ------------------------------------------------------------------------------------------------ clustered rows
@lru_cache(maxsize=None)
def clustered():
    """The 128 rows of gp_select_ref.clustered_pool as training rows of quad2d's two GPs, with the hyperparameters
    of gp_drop_ref.data(40, seed=80) and SF2: per GP a dict like gp_drop_ref.data's (y = gp_drop_ref.targets, Z the
    64 even rows shifted by 0.01)."""
    from gpmpc.models import get_spec

    spec = get_spec("quad2d")
    Zs = S.gp_inputs(spec, *S.clustered_pool(spec))
    hyp = D.data(40, seed=80)
    return [dict(X=X, y=D.targets(X), ell=h["ell"], sf2=sf2, sn2=D.SN2, Z=X[::2] + 0.01, d=X.shape[1])
            for X, h, sf2 in zip(Zs, hyp, SF2)]


def cluster_of(i):
    return int(i) // S.COPIES
