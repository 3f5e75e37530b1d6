"""numpy reference of gpmpc_gp_informative's score and counting rank, and the transitions and the target scale
the device-side training-data tests share (test_observe_cpu.py, test_gpu_preprocess.py, test_gpu_informative.py,
test_gpu_observe.py)."""

import numpy as np


def score(var, outputscale, inputs=None):
    """s_i = max_g var[g][i] / outputscale[g]; a NaN among a point's variances gives NaN (np.max propagates it),
    and so does a non-finite value among its GP inputs (P, sum d_g), whatever the variances of that point are."""
    var = np.asarray(var, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s = np.max(var / np.asarray(outputscale, dtype=np.float64)[:, None], axis=0)
    if inputs is not None:
        s[~np.isfinite(np.asarray(inputs)).all(1)] = np.nan
    return s


def beats(sj, j, si, i):
    """Whether point j comes before point i: a finite score before a non-finite one, a larger finite score
    before a smaller, and otherwise (equal finite scores, two non-finite ones) the lower index."""
    fj, fi = bool(np.isfinite(sj)), bool(np.isfinite(si))
    if fj != fi:
        return fj
    if fj and sj != si:
        return bool(sj > si)
    return j < i


def rank(scores, m):
    """pick[rank_i] = i for rank_i < m, rank_i = #{j : s_j beats s_i}: int32 (m,)."""
    s = np.asarray(scores, dtype=np.float64)
    P = len(s)
    assert 1 <= m <= P
    pick = np.full(m, -1, dtype=np.int32)
    for i in range(P):
        r = sum(beats(s[j], j, s[i], i) for j in range(P))
        if r < m:
            assert pick[r] == -1, "the rank is not a permutation"
            pick[r] = i
    assert (pick >= 0).all()
    return pick


def transitions(spec, P, seed=3):
    """P transitions (x, u) of the model: states around the reference (gpmpc.synthetic.initial_states), inputs
    uniform over the input box; x_next is the caller's plant step."""
    from gpmpc.synthetic import initial_states

    x, _ = initial_states(spec, spec.reference_trajectory(), P, seed=seed)
    u = np.random.default_rng(seed + 100).uniform(spec.u_lo, spec.u_hi, size=(P, spec.nu))
    return np.ascontiguousarray(x), np.ascontiguousarray(u)


def target_scale(spec, x, u, x_next, dt_diff, gravity):
    """S (P, n_gp): every target's own expression with each summand replaced by its absolute value, at the
    prior parameters -- the scale its rounding errors are proportional to."""
    p = spec.prior
    xd = np.abs((x_next - x) / dt_diff)
    if spec.name in ("quad2d", "quad3d"):
        thrust_map = np.abs(p["a"] * u[:, 0]) + abs(p["b"])
        if spec.name == "quad2d":
            s0 = xd[:, 1] + xd[:, 3] + abs(gravity) + thrust_map
            s1 = xd[:, 5] + np.abs(p["f"] * x[:, 4]) + np.abs(p["h"] * x[:, 5]) + np.abs(p["l"] * u[:, 1])
            return np.column_stack([s0, s1])
        s0 = xd[:, 1] + xd[:, 3] + xd[:, 5] + abs(gravity) + thrust_map
        # (the reference's rate targets subtract f_6 = x_9 and f_7 = x_10)
        return np.column_stack([s0, xd[:, 6] + np.abs(x[:, 9]), xd[:, 7] + np.abs(x[:, 10])])
    # cartpole: x_dot_1 - (tmp - k tha c) and x_dot_3 - tha, tha = (g s - c tmp) / den, tmp = (F + mp l w^2 s) / M
    mc, mp, l = p["m_c"], p["m_p"], p["l"]
    M = mc + mp
    th, w, F = x[:, 2], x[:, 3], u[:, 0]
    s, c = np.abs(np.sin(th)), np.abs(np.cos(th))
    tmp = (np.abs(F) + mp * l * w * w * s) / M
    den = l * (4.0 / 3.0 - mp * c * c / M)   # (a difference of two positive terms, kept as it is: 4/3 > mp / M)
    tha = (abs(spec.gravity) * s + c * tmp) / den   # (the prior's own gravity: the argument serves the thrust norm only)
    return np.column_stack([xd[:, 1] + tmp + mp * l * tha * c / M, xd[:, 3] + tha])
