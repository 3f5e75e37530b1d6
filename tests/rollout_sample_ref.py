"""CPU reference of gpmpc_rollout_sample, on rollout_ref.py and the oracle's dynamics: per step the applied input
(feedback as an fma chain over ascending j, then the clip), the exact posterior variance of every GP at the applied
point, one draw e_g = sqrt(max(var_g + noise_g, 0)) xi_g of its residual, and the oracle's RK4 step over GPs whose
mean is offset by e_g at every substage.

`gps` is a list of oracle GPs for the means (helpers.oracle_gps / fitc_oracle_gps) or None for the prior alone;
`exact_gps` the GPs of the variance (and of the likelihood noise), needed when xi is given or var is asked for."""

import math
from fractions import Fraction

import numpy as np

from helpers import O


def fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic; a non-finite operand falls back to the plain expression)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


class Offset:
    """An oracle GP whose mean is moved by a constant: mean_grad(z) = (m(z) + e, dm/dz).  gp None: the mean is e."""

    def __init__(self, gp, e):
        self.gp, self.e = gp, float(e)

    def mean_grad(self, z):
        if self.gp is None:
            return self.e, np.zeros(len(z))
        m, dm = self.gp.mean_grad(z)
        return m + self.e, dm


def applied_input(spec, x, u_nom, xref=None, K=None, clip=False, u_lo=None, u_hi=None):
    """u [P][nu] applied at x [P][nx]: v_c = u_nom[c], then v_c = fma(K[c][j], x[j] - xref[j], v_c) for j ascending,
    then v_c < lo ? lo : (v_c > hi ? hi : v_c) with the clip (a NaN stays a NaN)."""
    x, u_nom = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.atleast_2d(np.asarray(u_nom, dtype=np.float64))
    lo = np.asarray(spec.u_lo if u_lo is None else u_lo, dtype=np.float64)
    hi = np.asarray(spec.u_hi if u_hi is None else u_hi, dtype=np.float64)
    out = np.empty_like(u_nom)
    for p in range(u_nom.shape[0]):
        for c in range(spec.nu):
            v = float(u_nom[p, c])
            if K is not None:
                for j in range(spec.nx):
                    v = fma(float(K[c][j]), float(x[p, j] - xref[p, j]), v)
            if clip:
                v = lo[c] if v < lo[c] else (hi[c] if v > hi[c] else v)
            out[p, c] = v
    return out


def point_variances(spec, exact_gps, x, u):
    """[P][n_gp]: the exact posterior variance without likelihood noise of every GP at z[gp_src_g], z = [x; u]."""
    z = np.concatenate([np.atleast_2d(x), np.atleast_2d(u)], axis=-1)
    return np.stack([gp.var(z[:, list(idx)], with_noise=False) for gp, idx in zip(exact_gps, spec.to_dict()["gp_inputs"])], axis=-1)


def draws(exact_gps, var, xi, with_noise=False):
    """e [P][n_gp] = sqrt(max(var + with_noise sn2, 0)) xi."""
    noise = np.array([gp.sn2 if with_noise else 0.0 for gp in exact_gps])
    return np.sqrt(np.maximum(np.asarray(var) + noise, 0.0)) * np.asarray(xi)


def one_step(spec, gps, x, u, e=None):
    """x+ [P][nx] of one RK4 step from x under the applied u, every GP mean offset by e [P][n_gp] (None: no offset,
    rollout_ref.one_step)."""
    sd = spec.to_dict()
    out = []
    for p, (xp, up) in enumerate(zip(np.atleast_2d(x), np.atleast_2d(u))):
        if e is None:
            g = gps
        else:
            g = [Offset(None if gps is None else gps[i], e[p][i]) for i in range(spec.n_gp)]
        out.append(O.Dynamics(sd, g).rk4(np.asarray(xp, dtype=np.float64), np.asarray(up, dtype=np.float64))[0])
    return np.array(out)


def rollout(spec, gps, x0, u, xref=None, K=None, clip=False, xi=None, exact_gps=None, with_noise=False, var=False,
            u_lo=None, u_hi=None):
    """dict: x [P][T+1][nx], u [P][T][nu] the applied inputs and, with var, var [P][T][n_gp]."""
    x0 = np.asarray(x0, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    P, T = u.shape[:2]
    x = np.empty((P, T + 1, spec.nx))
    ua = np.empty((P, T, spec.nu))
    v = np.empty((P, T, spec.n_gp))
    x[:, 0] = x0
    for k in range(T):
        ua[:, k] = applied_input(spec, x[:, k], u[:, k], None if xref is None else xref[:, k], K, clip, u_lo, u_hi)
        e = None
        if xi is not None or var:
            v[:, k] = point_variances(spec, exact_gps, x[:, k], ua[:, k])
        if xi is not None:
            e = draws(exact_gps, v[:, k], xi[:, k], with_noise)
        x[:, k + 1] = one_step(spec, gps, x[:, k], ua[:, k], e)
    out = {"x": x, "u": ua}
    if var:
        out["var"] = v
    return out
