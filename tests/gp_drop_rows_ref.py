"""Float64 numpy models of gpmpc_gp_drop_rows and gpmpc_gp_redundant (csrc/gp_drop.hip), the
np.longdouble reference of the latter, the cases their tests share (tests/test_gp_drop_rows_cpu.py,
tests/test_gp_redundant_cpu.py, tests/test_gpu_gp_drop_rows.py, tests/test_gpu_redundant.py) and the margin.

Dropping a block.  State as in tests/gp_drop_ref.py: X (n, d), M = L^-1 (n, n), alpha.  D the m <= 16 dropped rows,
ascending, k the kept rows in their old order:

    V = -M[k, D] M[D, D]^-1,  B = M[k, k] + V M[D, k]  (= L[k, k]^-1),  M' = C^-1 B,  C = chol(I + V V^T)
    g = P[D, D]^-1 alpha[D]  (P = M^T M),  u = M[:, D] g,  alpha' = alpha[k] - M[:, k]^T u

C^-1 is applied per 16-row tile as gp_drop_ref.drop_block applies it (G_T, E_T, D_T, S_T).  A call's rows are made
m distinct values in 0 .. n-1 (`normalise`), sorted, and taken in blocks of at most 16 from the highest indices
down.  A zero on the diagonal of M[D, D] / P[D, D] (an inert row) reads as 1.

Criterion: gp_append_ref.worst_ratio against the longdouble recompute of the kept rows, the yardstick being the
upload path on the kept rows, as for gpmpc_gp_drop_oldest.

R_MODEL.  The model's worst e_model / e_full over CASES (each also with idx permuted; the inert-row case gives 2.3),
both GPs, mean, variance and gradient, measured with tests/test_gp_drop_rows_cpu.py -s: R_MODEL = 9.03 over the
states that keep at least two rows (variance, 21 rows less {0, 20}, gp0; 6.1 with 40 of 64 rows dropped, 1.4 at
npad 272), MARGIN = ceil(4 R_MODEL) = 37: the factor 4 covers the MFMA summation order and the rounding carried from
block to block, as in gp_drop_ref.py.  With one row left (17 rows less 16, leaving row 5) the yardstick is a 1 x 1
factorisation, exact to an ulp, and the ratio measures the yardstick (gp_drop_ref.py has the argument): R_ONE = 4499
(mean, gp0: e_model 5.0e-13, as in every other case, over e_full 1.1e-16), MARGIN_ONE = ceil(4 R_ONE) = 17996.

The rows missed least.  P_g = M_g^T M_g; p_g,i = P_g,ii; score s_i = max_g (1 / p_g,i - sn2_g) / sf2_g, a row inert
in g contributing 0; the pick is the smallest score (ties to the lower index, non-finite scores last); conditioning
c_t[i] = (P_ij - sum_{s<t} c_s[i] c_s[j]) / sqrt(p_j), p_i -= c_t[i]^2.  `redundant_f64` sums as the kernel does (16
parts of whole column tiles, a balanced tree), `redundant_ld` is the same recursion in longdouble on the longdouble
precision of the GP's data.  Over RED_CASES and GPU_RED_CASES the smallest gap between the best score and the
runner-up is 4.5e-9 (n = 272) against a float64 score error of 9e-16 there (2.4e-14 at worst, n = 40 with 33 rows
gone): factors of 5e6 and more.  The one step without a gap is the last of m = n - 1 (`structural_tie`).

Three GPs (`model_red_case`): quad3d's GPs of 40 rows each, drawn over the range of the model's transitions, each
with its own lengthscale (M_RED_ELL), outputscale and noise (M_RED_HYP), m = 33; and the same with row 39 inert in GP 1
only (a rejected append there, an accepted one in GPs 0 and 2), which `redundant_ld` takes as a `live` mask.  Measured
with tests/test_gp_redundant_cpu.py -s: the smallest gap is 1.09e-7 against a worst float64 score error of 8.0e-13, the
smallest factor 1.4e5 (step 29); with the inert row 3.5e-8 against 7.9e-13, the smallest factor 4.5e4 (step 32): the
same condition, GAP_FACTOR, as the quad2d cases, and the GPU test holds the device's scores to gap / GAP_FACTOR of
the model as theirs does.  Every GP decides a pick (`red_decided_by`): GP 1 from step 0, GP 2 at step 4 (1 with the inert
row), GP 0 at step 8; leaving one out or scoring it with GP 0's outputscale and noise changes the picks.  The inert row
is not forced out first: it is picked at step 1 with the score 2.2e-3 of the GPs in which it is live.
"""

from __future__ import annotations

import math

import numpy as np

import gp_append_ref as A
import gp_drop_ref as D
import gp_ref as R
from gp_pick_ref import PARTS, tree

LD = R.LD
SF2, SN2 = D.SF2, D.SN2
R_MODEL = 9.03
MARGIN = float(math.ceil(4 * R_MODEL))
R_ONE = 4499.0
MARGIN_ONE = float(math.ceil(4 * R_ONE))
GAP_FACTOR = 1000.0


def margin(n_kept: int) -> float:
    return MARGIN_ONE if n_kept < 2 else MARGIN


# (name, rows, dropped rows)
CASES = [
    ("both ends", 21, (0, 20)),
    ("a tile's first row", 33, (16,)),
    ("around the tile borders", 40, (3, 15, 16, 17, 31, 39)),
    ("a full scattered block", 48, tuple(range(1, 48, 3))),
    ("two blocks over three tiles", 64, (2, 9, 15, 16, 17, 20, 23, 29, 31, 32, 33, 36, 40, 41, 44, 46, 47)),
    ("forty rows", 64, tuple(i for i in range(64) if i % 8 not in (2, 5, 7))),
    ("npad 272 to 256", 272, (0, 5, 17, 40, 63, 64, 100, 128, 150, 191, 200, 222, 240, 255, 256, 271)),
    ("one row left", 17, tuple(i for i in range(17) if i != 5)),
]
CASE_IDS = [f"{n}-{len(rows)}rows" for _, n, rows in CASES]
assert [len(c[2]) for c in CASES] == [2, 1, 6, 16, 17, 40, 16, 16]


def data(n, seed=None):
    return D.data(n, seed=900 + n if seed is None else seed)


def permuted(rows, seed=3):
    return tuple(int(v) for v in np.random.default_rng(seed).permutation(np.asarray(rows)))


def normalise(idx, n, m=None):
    """(rows dropped, ascending; ok) of gpmpc_gp_drop_rows for the caller's indices: the distinct ones in range,
    filled up to m with the lowest rows not among them."""
    idx = [int(v) for v in idx]
    m = len(idx) if m is None else m
    inside = sorted({v for v in idx if 0 <= v < n})
    ok = 1 if len(inside) == m and len(idx) == m and all(0 <= v < n for v in idx) else 0
    fill = [i for i in range(n) if i not in set(inside)][:max(m - len(inside), 0)]
    return sorted(inside + fill), ok


def drop_block(state, d, info=None):
    """One block: the ascending rows d (at most 16) of the state; returns (state', ok)."""
    X, M, alpha = state
    n = M.shape[0]
    d = np.asarray(d, dtype=int)
    m = len(d)
    assert 1 <= m <= 16 and m < n and (np.diff(d) > 0).all() and d[0] >= 0 and d[-1] < n
    k = np.setdiff1d(np.arange(n), d)
    n2 = n - m
    MDD = M[np.ix_(d, d)].copy()
    dz = np.diag(MDD) == 0.0
    MDD[dz, dz] = 1.0                                   # inert dropped rows
    ok = bool(np.all(np.isfinite(np.diag(MDD)) & (np.diag(MDD) > 0.0)))
    LDD = D._inv_lower(MDD)
    MkD, MDk = M[np.ix_(k, d)], M[np.ix_(d, k)]
    V = -(MkD @ LDD)
    PDD = M[:, d].T @ M[:, d]
    pz = np.diag(PDD) == 0.0
    PDD[pz, pz] = 1.0
    Lp, okp = D._chol(PDD)
    g = D._spd_solve(Lp, alpha[d])
    alpha2 = alpha[k] - M[:, k].T @ (M[:, d] @ g)
    ok = ok and okp
    # the rank-m term: above the diagonal every product has a structural zero (V[i][b] needs d_b < k_i, M[d_b][k_c]
    # needs k_c < d_b), so B is lower triangular exactly
    B = M[np.ix_(k, k)] + V @ MDk
    if info is not None:
        info["upper"] = max(info.get("upper", 0.0), float(np.abs(np.triu(B, 1)).max(initial=0.0)))
    Mn = np.zeros((n2, n2))
    G = np.eye(m)
    S = np.zeros((m, n2))
    for lo in range(0, n2, 16):
        hi = min(lo + 16, n2)
        VT, BT = V[lo:hi], B[lo:hi]
        Lg, okg = D._chol(G)
        E = D._spd_solve(Lg, VT.T).T
        Lf, okf = D._chol(np.eye(hi - lo) + E @ VT.T)
        Dt = D._inv_lower(Lf)
        ok = ok and okg and okf
        Mn[lo:hi, :hi] = np.tril(Dt @ (BT[:, :hi] - E @ S[:, :hi]), lo)
        S += VT.T @ BT
        G += VT.T @ VT
    return (X[k].copy(), Mn, alpha2), ok


def drop_rows(state, idx, info=None):
    """gpmpc_gp_drop_rows: returns (state', dropped, ok)."""
    n = state[1].shape[0]
    rows, ok = normalise(idx, n)
    left = len(rows)
    while left > 0:
        mb = min(16, left)
        left -= mb
        state, okb = drop_block(state, rows[left:left + mb], info)
        ok = ok if okb else 0
    return state, rows, ok


# ---------------------------------------------------------------------------------------- the rows missed least
# (rows, picks)
RED_CASES = [(21, 5), (40, 17), (64, 33), (272, 16)]
# the GPU test's: n = 24, 40, 272 with m = 1, 17, min(n - 1, 33); picks are prefixes, so the longest run serves all
GPU_RED_CASES = [(24, 23), (40, 33), (272, 33)]


def structural_tie(n, m, t):
    """Step t of m = n - 1 picks with two rows left: each GP's precision is then 2 x 2 with equal diagonal entries
    (K's diagonal is constant), so the two scores are equal in exact arithmetic and rounding decides between them:
    the one step at which no pick is determined beyond the pair."""
    return m == n - 1 and t == m - 1


def linvT_padded(M):
    n = M.shape[0]
    npad = (n + 15) // 16 * 16
    out = np.zeros((npad, npad))
    out[:n, :n] = M.T
    return out


def _dots(LT, j=None):
    """The parts of linvT[i] . linvT[j] for every row i (j = None: of every row against itself), in the kernel's
    order: part q is one sequential sum over whole column tiles."""
    npad = LT.shape[0]
    nt = npad // 16
    parts = []
    for q in range(PARTS):
        acc = np.zeros(npad)
        for c in range(16 * (q * nt // PARTS), 16 * ((q + 1) * nt // PARTS)):
            acc = acc + LT[:, c] * (LT[:, c] if j is None else LT[j, c])
        parts.append(acc)
    return parts


def _scores(p, live, hyp):
    """max_g (1 / p_g - sn2_g) / sf2_g per row, a row inert in g contributing 0 (a NaN stays)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = [np.where(live[g], (1.0 / p[g] - p[g].dtype.type(hyp[g][1])) / p[g].dtype.type(hyp[g][0]), p[g].dtype.type(0))
                 for g in range(len(p))]
    s = terms[0]
    for t in terms[1:]:
        s = np.where((t > s) | np.isnan(t), t, s)
    return s


def _best(s, open_):
    """The pick: the smallest finite score among the open rows (ties to the lower index), else the lowest open row."""
    fin = open_ & np.isfinite(s.astype(np.float64))
    if fin.any():
        cand = np.flatnonzero(fin)
        return int(cand[np.argmin(s[cand])]), True   # (argmin: the first of equal minima)
    return int(np.flatnonzero(open_)[0]), False


def redundant_f64(Ms, hyp, m):
    """gpmpc_gp_redundant in float64: Ms the GPs' M (n, n), hyp (sf2, sn2) per GP.  Returns picks, scores, ok and
    the final p (n_gp, n)."""
    n = Ms[0].shape[0]
    LTs = [linvT_padded(M) for M in Ms]
    live = [np.diag(M) != 0.0 for M in Ms]
    p = [tree(_dots(LT))[:n].copy() for LT in LTs]   # every row against itself: the same parts and tree
    cols = [np.zeros((m, n)) for _ in Ms]
    open_ = np.ones(n, dtype=bool)
    picks, scores, tables, ok = [], [], [], 1
    for t in range(m):
        s = _scores(p, live, hyp)
        j, fin = _best(s, open_)
        picks.append(j)
        scores.append(float(s[j]) if fin else float("nan"))
        tables.append(np.where(open_, s, np.nan))
        for g, LT in enumerate(LTs):
            pj = p[g][j]
            if not live[g][j]:
                continue
            if not (np.isfinite(pj) and pj > 0.0):
                ok = 0
                continue
            parts = [q[:n].copy() for q in _dots(LT, j)]
            for s_ in range(t):
                parts[s_ % PARTS] = parts[s_ % PARTS] - cols[g][s_] * cols[g][s_, j]
            c = tree(parts) / math.sqrt(pj)
            cols[g][t] = c
            p[g] = p[g] - c * c
        open_[j] = False
    return dict(picks=np.array(picks), scores=np.array(scores), tables=tables, ok=ok, p=np.stack(p))


def precision_ld(X, ell, sf2=SF2, sn2=SN2):
    """(K + sn2 I)^-1 in longdouble from the float64 data."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    n = X.shape[0]
    K = R.kernel_ld(X, ell, sf2, X) + LD(float(sn2)) * np.eye(n, dtype=LD)
    Li = A.solve_lower_ld(A.chol_ld(K), np.eye(n, dtype=LD))
    return Li.T @ Li


def redundant_ld(Ps, hyp, m, forced=None, live=None):
    """The same recursion in longdouble on the precisions Ps (n, n).  `live` (per GP a mask of n rows, default: every
    row) marks the rows that are not inert in that GP; an inert row's row and column of Ps[g] are zero, its term is 0
    and it conditions nothing in g.  Per step: the pick, its score, the gap to the runner-up and the scores of all
    open rows (for the model's error)."""
    n = Ps[0].shape[0]
    p = [np.diag(P).copy() for P in Ps]
    live = [np.ones(n, dtype=bool) for _ in Ps] if live is None else [np.asarray(l, dtype=bool) for l in live]
    cols = [np.zeros((m, n), dtype=LD) for _ in Ps]
    open_ = np.ones(n, dtype=bool)
    picks, scores, gaps, tables = [], [], [], []
    for t in range(m):
        s = _scores(p, live, hyp)
        j, _ = _best(s, open_)
        rest = np.sort(s[open_])
        gaps.append(float(rest[1] - rest[0]) if len(rest) > 1 else float("inf"))
        if forced is not None:
            j = int(forced[t])
        picks.append(j)
        scores.append(s[j])
        tables.append(np.where(open_, s, LD(np.nan)))
        for g, P in enumerate(Ps):
            if not live[g][j]:
                continue
            c = (P[:, j] - cols[g][:t].T @ cols[g][:t, j]) / np.sqrt(p[g][j])
            cols[g][t] = c
            p[g] = p[g] - c * c
        open_[j] = False
    return dict(picks=np.array(picks), scores=np.array(scores), gaps=np.array(gaps), tables=tables, p=np.stack(p), open=open_)


_RED: dict = {}


def red_case(n, m):
    """The quad2d data of n rows, its upload states, the model's and the reference's run: computed once."""
    if (n, m) not in _RED:
        dat = data(n)
        hyp = [(SF2, SN2)] * len(dat)
        states = [D.upload_state(dg["X"], dg["y"], dg["ell"]) for dg in dat]
        model = redundant_f64([s[1] for s in states], hyp, m)
        ref = redundant_ld([precision_ld(dg["X"], dg["ell"]) for dg in dat], hyp, m)
        _RED[(n, m)] = dict(data=dat, hyp=hyp, states=states, model=model, ref=ref)
    return _RED[(n, m)]


def score_error(model_table, ref_table):
    """The worst |model - reference| over the open rows of one step's scores."""
    keep = ~np.isnan(ref_table.astype(np.float64))
    return float(np.abs(model_table[keep] - ref_table[keep].astype(np.float64)).max())


# --------------------------------------------------------------- three GPs with their own outputscale and noise each
# quad3d: n = M_RED_N rows per GP (the call ranks the same rows in all), inputs over the range of the model's
# transitions (gp_select_ref.input_box), (sf2, sn2) and the lengthscale distinct per GP
M_RED_N, M_RED_M = 40, 33
M_RED_HYP = ((2.5, 1e-3), (0.7, 4e-3), (1.3, 2e-3))
M_RED_ELL = (0.015, 0.25, 0.3)
M_RED_SEED = 520
M_INERT = (1, 39)   # (GP, row): the row that is inert in that GP only
_MRED: dict = {}


def model_red_data(name="quad3d", n=M_RED_N):
    import gp_select_ref as S

    out = []
    for g, (lo, hi) in enumerate(S.input_box(name)):
        rng = np.random.default_rng(M_RED_SEED + 31 * g)
        X = rng.uniform(lo, hi, (n, len(lo)))
        out.append(dict(X=X, y=D.targets(X), ell=M_RED_ELL[g], d=len(lo), Z=rng.uniform(lo, hi, (D.NPTS, len(lo)))))
    return out


def model_red_case(m=M_RED_M, inert=False):
    """quad3d's three GPs of M_RED_N rows, their upload states, the model's and the reference's run.  `inert`: row
    M_INERT[1] is inert in GP M_INERT[0] (a rejected append of one row after an upload of the rows before it) and was
    appended to the other GPs (gp_drop_ref.append_block)."""
    if (m, inert) not in _MRED:
        dat, hyp, n = model_red_data(), list(M_RED_HYP), M_RED_N
        gi, row = M_INERT
        assert row == n - 1
        states, Ps, live = [], [], []
        for g, (dg, (sf2, sn2)) in enumerate(zip(dat, hyp)):
            lv = np.ones(n, dtype=bool)
            if not inert:
                states.append(D.upload_state(dg["X"], dg["y"], dg["ell"], sf2, sn2))
                Ps.append(precision_ld(dg["X"], dg["ell"], sf2, sn2))
            else:
                st = D.upload_state(dg["X"][:row], dg["y"][:row], dg["ell"], sf2, sn2)
                if g == gi:
                    states.append(D.with_inert(st, row, 1))
                    P = np.zeros((n, n), dtype=LD)
                    P[:row, :row] = precision_ld(dg["X"][:row], dg["ell"], sf2, sn2)
                    Ps.append(P)
                    lv[row] = False
                else:
                    states.append(D.append_block(st, dg["X"][row:], dg["y"][row:], dg["ell"], sf2, sn2))
                    Ps.append(precision_ld(dg["X"], dg["ell"], sf2, sn2))
            live.append(lv)
        model = redundant_f64([s[1] for s in states], hyp, m)
        ref = redundant_ld(Ps, hyp, m, live=live)
        _MRED[(m, inert)] = dict(data=dat, hyp=hyp, states=states, model=model, ref=ref, Ps=Ps, live=live)
    return _MRED[(m, inert)]


def red_decided_by(Ps, hyp, live, picks, err=0.0):
    """Per GP the steps at which it decides the pick: its term of the picked row is the largest over the GPs (the
    row's score is that GP's) and stays so when moved by err either way.  Recomputed from the picks."""
    n = Ps[0].shape[0]
    p = [np.diag(P).copy() for P in Ps]
    cols = [[] for _ in Ps]
    out = [[] for _ in Ps]
    for t, j in enumerate(int(v) for v in picks):
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = np.array([float((1 / p[g][j] - LD(hyp[g][1])) / LD(hyp[g][0])) if live[g][j] else 0.0 for g in range(len(Ps))])
        g = int(terms.argmax())
        if terms[g] - err > np.delete(terms, g).max() + err:
            out[g].append(t)
        for q, P in enumerate(Ps):
            if not live[q][j]:
                continue
            c = P[:, j].copy()
            for cc in cols[q]:
                c -= cc * cc[j]
            c = c / np.sqrt(p[q][j])
            cols[q].append(c)
            p[q] = p[q] - c * c
    return out
