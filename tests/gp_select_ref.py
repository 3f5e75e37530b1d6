"""numpy reference of gpmpc_gp_select (csrc/gp_observe.hip), the cases its tests share
(tests/test_gp_select_cpu.py, tests/test_gpu_select.py) and their margin.

The rule.  P candidates, per GP g their inputs Z_g (P, d_g); with K_g + sn2_g I = L_g L_g^T over the training rows,
v_g,i = L_g^-1 k_g(X_g, z_i) and d_g,i = sf2_g - |v_g,i|^2.  For t = 0 .. m-1: the score s_i = max_g d_g,i / sf2_g of
the candidates not yet picked (NaN for a candidate with a non-finite input), j_t the largest finite score (ties to the
lower index; when none is left, the non-finite candidates in index order, which condition nothing), and per GP
    p = d_g,j + sn2_g,  l_t[i] = (k_g(z_i, z_j) - v_g,i . v_g,j - sum_{s<t} l_s[i] l_s[j]) / sqrt(p),  d_g,i -= l_t[i]^2.
This is a pivoted partial Cholesky of the candidates' posterior covariance plus sn2 I on the picks, so afterwards
d_g,i is the posterior variance (without noise) of GP g with the picked rows appended.

`greedy_ld` runs it in np.longdouble (gp_append_ref.chol_ld / solve_lower_ld, gp_ref.kernel_ld) and also returns,
per step, the gap between the best score and the runner-up's (a candidate with the same inputs as the best one, the
duplicated transition, is no runner-up: that tie is exact and the index decides it).  `greedy_f64` is the float64
model in the kernels' summation order: V = Linv k from the upload path's float64 factor, the inner product
v_i . v_j + sum_s l_s[i] l_s[j] in PARTS = 16 parts (part q: the column tiles [q nt / 16, (q + 1) nt / 16) of V's
nt, then the l columns q, q + 16, ..), each a sequential sum, added as a balanced tree ((0 + 1) + (2 + 3)) + .. .

Criterion, as for the append and the drop (gp_append_ref.worst_ratio): with e_full the worst error over the finite
candidates of a float64 full recompute of the GP with the picked rows appended (GaussianProcess.device_layout, the
upload path) against the longdouble reference, the selection's residual variances must have a worst error of at most
MARGIN_SELECT e_full, per GP.

R_MODEL.  The worst e_model / e_full of `greedy_f64` over CASES (both GPs), measured with
tests/test_gp_select_cpu.py -s: 2.658, rounded up to R_MODEL = 2.66 (n = 40, P = 1, m = 1, gp1: e_model 7.2e-17
against e_full 2.7e-17, a single candidate whose yardstick happens to round well; 0.66 .. 0.94 in the other cases
with one candidate, 0.52 .. 1.01 in every case with 40 or 130).  MARGIN_SELECT = ceil(4 R_MODEL) = 11: the factor 4
covers the MFMA summation order of V and of the start variances (the gp_drop_ref.py convention).

Gap condition.  The device's picks must equal `greedy_ld`'s wherever rounding cannot reorder two candidates: at every
step of every case the gap must be at least GAP_FACTOR = 1000 times the score error the criterion allows,
MARGIN_SELECT max_g e_full,g / sf2_g (e_full of the host recompute).  Measured over CASES: the smallest gap is
2.45e-9 (n = 272, P = 130, m = 33, step 19) against an allowed error of 4.2e-14 there, a factor 5.9e4, which is also
the smallest factor.

Clustered pool (CLUSTERS = 8 transitions, each repeated COPIES = 16 times with perturbations of 1e-3: what a batch
that tracks one reference produces; GPs of 40 rows).  After m = 16 picks the largest residual score left in the pool
is 1.39e-4 with the greedy rule, whose picks come from six of the eight transitions, against 3.07e-4 with the top-16
rank rule (observe_ref.rank), whose picks are all copies of one: a ratio of 0.45.

Other models (M_CASES; model_data, model_points, model_base, model_ref).  quad3d: three GPs of 24, 272 and 40 rows
(input dimensions 1, 3, 3); cartpole: two GPs of 24 and 40 rows that read the same three columns of z.  Every GP has
its own lengthscale (M_ELL), outputscale (M_SF2), noise (M_SN2) and training rows, drawn uniformly over the box the
GP's inputs span over BOX_POINTS transitions (input_box), so the start scores spread (6e-4 .. 4e-2 over a pool of 40).
Pools of 40 and 130 candidates (quad3d) and 40 (cartpole) with m = 1, 17, 33, and one quad3d pool of a single
candidate.  Besides the duplicate, candidate NANROW holds a NaN in a state column a GP reads (quad3d: x[:, 10], GP 2
alone) and candidate NANROW2 one in a state column no GP reads, which must change nothing.  Measured with
tests/test_gp_select_cpu.py -s:
  * e_model / e_full of `greedy_f64` is at most 1.074 over the pools of 40 and 130 (quad3d, P = 40, m = 1, gp2; 0.25 ..
    1.07 over all of them), within R_MODEL: their GPU tests use MARGIN_SELECT.  The single candidate gives 24.24
    (quad3d, P = 1, m = 1, gp1: e_model 2.2e-16 against e_full 9.1e-18, a yardstick that happens to round well, as
    in the quad2d case that set R_MODEL): that case alone has R_MODEL_ONE = 24.24, MARGIN_SELECT_ONE = ceil(4 x 24.24)
    = 97 (`margin_for`).
  * The smallest gap is 1.01e-6 (cartpole, P = 40, m = 33, step 22) against an allowed score error of 2.4e-14, a factor
    4.2e7, which is also the smallest factor (quad3d: 1.9e8 at P = 40, m = 33, step 25).
  * Every GP decides a pick (`decided_by`: its term is the largest at the picked candidate by more than the allowed
    error both ways): quad3d P = 40 at steps 0 (GP 0), 1 (GP 1), 2 (GP 2), P = 130 at steps 2, 1, 0; cartpole at steps
    0 and 4.  Leaving a GP out, or giving it GP 0's outputscale and noise in the loop, changes the picks at those steps.
"""

from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

import gp_append_ref as A
import gp_drop_ref as D
import gp_ref as R
import observe_ref as OR
from gp_pick_ref import PARTS, tree

LD = R.LD
R_MODEL = 2.66
MARGIN_SELECT = float(math.ceil(4 * R_MODEL))
GAP_FACTOR = 1000.0

DUP, NANROW = (3, 7), 5    # transition 7 repeats transition 3; transition 5 holds a NaN
SF2 = (2.5, 0.7)           # outputscales that are not 1
NS, PS = (24, 40, 272), (1, 40, 130)
CLUSTERS, COPIES = 8, 16


def ms_for(P):
    return sorted({1, min(17, P), min(P, 33)})


CASES = [(n, P, m) for n in NS for P in PS for m in ms_for(P)]


def points(spec, P, seed=5):
    """P transitions' (x, u) with the duplicate and the NaN (where P has room for them)."""
    x, u = OR.transitions(spec, P, seed=seed)
    if P > max(DUP):
        x[DUP[1]], u[DUP[1]] = x[DUP[0]], u[DUP[0]]
        x[NANROW, 4] = np.nan
    return x, u


def gp_inputs(spec, x, u):
    """Per GP the candidates' inputs (P, d_g), gathered as gpmpc_preprocess gathers them."""
    z = np.hstack([x, u])
    return [np.ascontiguousarray(z[:, list(idx)]) for idx in spec.gp_inputs]


def gps_of(data, n, sf2=SF2):
    """The GPs of a case: the first n rows of gp_drop_ref.data with the test's outputscales."""
    return [dict(X=dg["X"][:n], ell=dg["ell"], sf2=s, sn2=D.SN2) for dg, s in zip(data, sf2)]


def finite_mask(Zs):
    return np.logical_and.reduce([np.isfinite(Z).all(1) for Z in Zs])


def _clean(Z, finite):
    Z = np.array(Z, dtype=np.float64)
    Z[~finite] = 0.0   # (a placeholder: such a candidate takes no part)
    return Z


def prepare_ld(gps, Zs):
    """Per GP the start variances d (P,) and the candidates' posterior covariance C (P, P), in longdouble."""
    finite = finite_mask(Zs)
    out = []
    for gp, Z in zip(gps, Zs):
        Z = _clean(Z, finite)
        n = gp["X"].shape[0]
        K = R.kernel_ld(gp["X"], gp["ell"], gp["sf2"], gp["X"]) + LD(float(gp["sn2"])) * np.eye(n, dtype=LD)
        L = A.chol_ld(K)
        v = A.solve_lower_ld(L, R.kernel_ld(gp["X"], gp["ell"], gp["sf2"], Z).T.copy())   # (n, P)
        C = R.kernel_ld(Z, gp["ell"], gp["sf2"], Z) - v.T @ v
        out.append(dict(d=LD(float(gp["sf2"])) - (v * v).sum(0), C=C, sf2=LD(float(gp["sf2"])), sn2=LD(float(gp["sn2"]))))
    return out, finite


def _scores(ds, sf2s, finite, picked):
    s = np.max(np.stack([d / s2 for d, s2 in zip(ds, sf2s)]), axis=0)
    open_ = finite & ~picked
    return s, open_


def _greedy(ds, sf2s, sn2s, finite, m, column, Zs=None, forced=None):
    """The loop on start variances `ds` (list of (P,)); column(g, t, j, ls) returns C_g[:, j] - sum_s l_s l_s[j]
    before the division.  Returns picks, gains, final ds, gaps (absolute, score units; inf where no runner-up)."""
    P = len(ds[0])
    dt = ds[0].dtype
    picked = np.zeros(P, dtype=bool)
    ls = [[] for _ in ds]
    picks, gains, gaps, ok = [], [], [], 1
    for t in range(m):
        s, open_ = _scores(ds, sf2s, finite, picked)
        cand = np.flatnonzero(open_)
        if forced is not None:
            j = int(forced[t])
            gains.append(s[j] if finite[j] else dt.type(np.nan))
            gaps.append(np.inf)
            if not finite[j]:
                picks.append(j)
                picked[j] = True
                continue
        elif len(cand) == 0:
            j = int(np.flatnonzero(~finite & ~picked)[0])
            picks.append(j)
            gains.append(dt.type(np.nan))
            gaps.append(np.inf)
            picked[j] = True
            continue
        else:
            best = s[cand].max()
            j = int(cand[np.flatnonzero(s[cand] == best)[0]])
            gains.append(best)
            others = [i for i in cand if i != j and (Zs is None or any((Z[i] != Z[j]).any() for Z in Zs))]
            gaps.append(float(best - s[others].max()) if others else np.inf)
        picks.append(j)
        picked[j] = True
        for g in range(len(ds)):
            p = ds[g][j] + sn2s[g]
            if not (np.isfinite(p) and p > 0):
                ok = 0
                ls[g].append(np.zeros(P, dtype=dt))
                continue
            l = column(g, t, j, ls[g]) / np.sqrt(p)
            ls[g].append(l)
            ds[g] = ds[g] - l * l
    return np.array(picks, dtype=np.int32), np.array(gains), ds, np.array(gaps), ok


def greedy_ld(gps, Zs, m, forced=None):
    """picks (m,) int32, gains (m,) float64, resid (n_gp, P) longdouble, gaps (m,) in score units, relative gaps."""
    prep, finite = prepare_ld(gps, Zs)
    return greedy_from(prep, finite, Zs, m, forced)


def greedy_from(prep, finite, Zs, m, forced=None):
    def column(g, t, j, ls):
        c = prep[g]["C"][:, j].copy()
        for l in ls:
            c -= l * l[j]
        return c

    picks, gains, ds, gaps, ok = _greedy([p["d"].copy() for p in prep], [p["sf2"] for p in prep],
                                         [p["sn2"] for p in prep], finite, m, column, Zs, forced)
    assert ok == 1
    gains = gains.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = gaps / gains
    return dict(picks=picks, gains=gains, resid=np.stack(ds), gaps=gaps, rel_gaps=rel, finite=finite)


def greedy_f64(gps, Zs, m):
    """The float64 model in the kernels' summation order; picks, gains, resid (n_gp, P), ok."""
    finite = finite_mask(Zs)
    Vs, ds, Zc = [], [], []
    for gp, Z in zip(gps, Zs):
        Z = _clean(Z, finite)
        X, M, _ = D.upload_state(gp["X"], D.targets(gp["X"]), gp["ell"], gp["sf2"], gp["sn2"])
        n = X.shape[0]
        npad = (n + 15) // 16 * 16
        V = np.zeros((npad, len(Z)))
        V[:n] = M @ D.kernel64(X, gp["ell"], gp["sf2"], Z).T
        Vs.append(V)
        ds.append(gp["sf2"] - (V * V).sum(0))
        Zc.append(Z)

    def column(g, t, j, ls):
        V, gp = Vs[g], gps[g]
        ntile = V.shape[0] // 16
        parts = []
        for q in range(PARTS):
            acc = np.zeros(V.shape[1])
            for c in range(16 * (q * ntile // PARTS), 16 * ((q + 1) * ntile // PARTS)):
                acc = acc + V[c] * V[c, j]
            for s in range(q, t, PARTS):
                acc = acc + ls[s] * ls[s][j]
            parts.append(acc)
        k = D.kernel64(Zc[g][j:j + 1], gp["ell"], gp["sf2"], Zc[g])[:, 0]
        return k - tree(parts)

    picks, gains, ds, _, ok = _greedy(ds, [gp["sf2"] for gp in gps], [gp["sn2"] for gp in gps], finite, m, column)
    return dict(picks=picks, gains=gains.astype(np.float64), resid=np.stack(ds), ok=ok, finite=finite)


def appended(gps, Zs, picks, finite):
    """Per GP the training inputs with the finite picks' rows appended (the non-finite ones condition nothing)."""
    keep = [int(j) for j in picks if finite[j]]
    return [np.vstack([gp["X"], Z[keep]]) for gp, Z in zip(gps, Zs)]


def full64(gps, Xs, Zs, finite):
    """The yardstick on the host: a float64 full recompute (the upload path's factor) of the GPs on rows Xs, its
    noise-free variance at the finite candidates, (n_gp, P) with NaN elsewhere."""
    out = np.full((len(gps), len(finite)), np.nan)
    for g, (gp, X, Z) in enumerate(zip(gps, Xs, Zs)):
        st = D.upload_state(X, D.targets(X), gp["ell"], gp["sf2"], gp["sn2"])
        out[g, finite] = D.predict(st, gp["ell"], Z[finite], gp["sf2"], gp["sn2"])["var"] - gp["sn2"]
    return out


def allowed_score_error(gps, e_full):
    """The score error the criterion allows: MARGIN_SELECT max_g e_full,g / sf2_g."""
    return MARGIN_SELECT * max(e / gp["sf2"] for e, gp in zip(e_full, gps))


@lru_cache(maxsize=None)
def case_data(n):
    return D.data(n, seed=40 + n)


@lru_cache(maxsize=None)
def case_base(n, P):
    """(gps, Zs, prep, finite) of the cases with n training rows and P candidates (quad2d)."""
    from gpmpc.models import get_spec

    spec = get_spec("quad2d")
    gps = gps_of(case_data(n), n)
    Zs = gp_inputs(spec, *points(spec, P))
    prep, finite = prepare_ld(gps, Zs)
    return gps, Zs, prep, finite


@lru_cache(maxsize=None)
def case_ref(n, P, m):
    gps, Zs, prep, finite = case_base(n, P)
    return greedy_from(prep, finite, Zs, m)


def clustered_pool(spec, seed=9):
    """CLUSTERS transitions, each repeated COPIES times with perturbations of 1e-3 (a batch on one reference)."""
    x, u = OR.transitions(spec, CLUSTERS, seed=seed)
    rng = np.random.default_rng(seed + 1)
    x = np.repeat(x, COPIES, axis=0) + 1e-3 * rng.standard_normal((CLUSTERS * COPIES, x.shape[1]))
    u = np.repeat(u, COPIES, axis=0) + 1e-3 * rng.standard_normal((CLUSTERS * COPIES, u.shape[1]))
    return x, u


# ------------------------------------------------------------------------- the other models: three GPs, shared inputs
# quad3d: three GPs (input dimensions 1, 3, 3 of a gathered row of 7 columns) of 24, 272 and 40 rows; cartpole: two GPs
# that read the same three columns, of 24 and 40 rows.  Nothing but cartpole's input columns is shared between GPs.
M_SF2 = (2.5, 0.7, 1.3)
M_SN2 = (1e-3, 4e-3, 2e-3)
M_ROWS = {"quad3d": (24, 272, 40), "cartpole": (24, 40)}
M_ELL = {"quad3d": (0.06, 0.15, 0.22), "cartpole": (2.6, 4.1)}
M_SEED = {"quad3d": 300, "cartpole": 400}
M_PS = {"quad3d": (40, 130), "cartpole": (40,)}
# the candidate with a NaN in a state column that a GP reads (quad3d: x[:, 10], read by GP 2 alone) and the one with a
# NaN in a state column no GP reads
NANROW2, READ_COL, UNREAD_COL = 11, {"quad3d": 10, "cartpole": 3}, 0
BOX_POINTS, BOX_SEED = 512, 77

M_CASES = [(name, P, m) for name in M_ROWS for P in M_PS[name] for m in ms_for(P)] + [("quad3d", 1, 1)]
# the model's ratio in the one case with a single candidate (quad3d, P = 1, m = 1, gp1), and its margin
R_MODEL_ONE = 24.24
MARGIN_SELECT_ONE = float(math.ceil(4 * R_MODEL_ONE))


def margin_for(P):
    """The margin of the model cases with P candidates."""
    return MARGIN_SELECT_ONE if P == 1 else MARGIN_SELECT


def model_points(spec, P, seed=5, unread_nan=True):
    """P transitions' (x, u) with the duplicate, the NaN a GP reads and the NaN none reads (where P has room)."""
    x, u = OR.transitions(spec, P, seed=seed)
    if P > NANROW2:
        x[DUP[1]], u[DUP[1]] = x[DUP[0]], u[DUP[0]]
        x[NANROW, READ_COL[spec.name]] = np.nan
        if unread_nan:
            x[NANROW2, UNREAD_COL] = np.nan
    return x, u


@lru_cache(maxsize=None)
def input_box(name):
    """Per GP (lo, hi) of its inputs over BOX_POINTS transitions of the model: where the candidates lie."""
    from gpmpc.models import get_spec

    spec = get_spec(name)
    return [(Z.min(0), Z.max(0)) for Z in gp_inputs(spec, *OR.transitions(spec, BOX_POINTS, seed=BOX_SEED))]


@lru_cache(maxsize=None)
def model_data(name, rows=None):
    """Per GP of the model dict(X, y, ell, sf2, sn2, Z, d): rows[g] training inputs uniform over input_box, each GP from
    its own seed (cartpole's two GPs read the same columns of z and hold different rows)."""
    rows = M_ROWS[name] if rows is None else rows
    out = []
    for g, ((lo, hi), n) in enumerate(zip(input_box(name), rows)):
        rng = np.random.default_rng(M_SEED[name] + 31 * g)
        X = rng.uniform(lo, hi, (max(n, M_ROWS[name][g]), len(lo)))[:n]
        out.append(dict(X=X, y=D.targets(X), ell=M_ELL[name][g], sf2=M_SF2[g], sn2=M_SN2[g], d=len(lo),
                        Z=rng.uniform(lo, hi, (D.NPTS, len(lo)))))
    return out


@lru_cache(maxsize=None)
def model_base(name, P):
    """(gps, Zs, prep, finite) of the model's cases with P candidates."""
    from gpmpc.models import get_spec

    spec = get_spec(name)
    gps = model_data(name)
    Zs = gp_inputs(spec, *model_points(spec, P))
    prep, finite = prepare_ld(gps, Zs)
    return gps, Zs, prep, finite


@lru_cache(maxsize=None)
def model_ref(name, P, m):
    gps, Zs, prep, finite = model_base(name, P)
    return greedy_from(prep, finite, Zs, m)


def decided_by(prep, ref, err):
    """Per GP the steps of the run at which it decides the pick: its term d_g,j / sf2_g of the picked candidate j is
    the largest over the GPs, and stays so when moved by err (the score error the criterion allows) either way.  The
    terms are recomputed step by step from the run's picks."""
    ds = [p["d"].copy() for p in prep]
    ls = [[] for _ in prep]
    out = [[] for _ in prep]
    for t, j in enumerate(int(v) for v in ref["picks"]):
        if not ref["finite"][j]:
            continue
        terms = np.array([float(d[j] / p["sf2"]) for d, p in zip(ds, prep)])
        g = int(terms.argmax())
        if terms[g] - err > np.delete(terms, g).max() + err:
            out[g].append(t)
        for q, p in enumerate(prep):
            c = p["C"][:, j].copy()
            for l in ls[q]:
                c -= l * l[j]
            l = c / np.sqrt(ds[q][j] + p["sn2"])
            ls[q].append(l)
            ds[q] = ds[q] - l * l
    return out
