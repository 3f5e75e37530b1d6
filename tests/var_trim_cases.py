"""Cases of the trimmed triangular variance kernel (gp_var_tri_kernel<NT, FROM_STATE, NQ>,
csrc/gp_kernels.hip), shared by tests/test_gpu_var_trim.py (MI355X) and tests/test_var_trim_cpu.py,
which builds every case here and makes the reference-only assertions without a GPU.

Operands, reference and bound are those of tests/gp_ref.py.  The handle-based cases run on quad2d
(GP0 d = 1, GP1 d = 3) with B = 5 and H = 7: 35 points, three point tiles, the last partly valid.
Both GPs have n = 16 (NT - 1) + r training rows, so the last column tile holds r real columns:

  NT  1   the only tile is both the diagonal and the ragged one
      2   the smallest case with a full tile in front
      3   the smallest with a diagonal tile that is not the last
      13  the flagship size (r = 8: n = 200, r = 4: n = 196)
      16  the largest
  r   1, 4   both ends of NQ = 1        5, 8   both ends of NQ = 2
      9, 16  both ends of the full tile (NQ = 0)

Every reference is computed once (lru_cache) and handed out read-only.
"""

from __future__ import annotations

import functools

import numpy as np

import gp_ref as R
from gp_append_ref import reference as fit_reference

SF2, SN2 = 1e-3, 1e-6
B, H = 5, 7
NTS = (1, 2, 3, 13, 16)
RS = (1, 4, 5, 8, 9, 16)
HANDLE_CASES = [(nt, r) for nt in NTS for r in RS]
MIXED_CASES = [(196, 200), (200, 205)]     # GP0, GP1 rows: the GPs of one launch disagree on NQ
FREE_NS = (196, 200)                       # handle-free, NT = 13: NQ = 1 and NQ = 2
FREE_POINTS = 193
# append: n = 196 uploaded with capacity 224, then blocks of 4, 4, 1 and 8 rows:
# 196 -> 200 (NQ 1 -> 2) -> 204 -> 205 (the full tile) -> 213 (NT = 14, NQ = 2)
APPEND_N0, APPEND_CAP, APPEND_BLOCKS = 196, 224, (4, 4, 1, 8)
APPEND_SF2, APPEND_SN2 = 1.0, 1e-3         # the setting of tests/test_gpu_gp_append.py


def quads(n: int) -> int:
    """var_tri_quads of gp_kernels.hip for one GP of n rows."""
    r = n - 16 * ((n + 15) // 16 - 1)
    return (r + 3) // 4 if r <= 8 else 0


def _ro(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def spec():
    from gpmpc.models import get_spec

    return get_spec("quad2d")


@functools.lru_cache(maxsize=None)
def iterate(seed: int):
    """A seeded iterate in [-1, 1] and the GP inputs z_k = [x_k; u_k][var_inputs] per GP."""
    sp = spec()
    rng = np.random.default_rng(7000 + seed)
    xs = rng.uniform(-1.0, 1.0, (B, H + 1, sp.nx))
    us = rng.uniform(-1.0, 1.0, (B, H, sp.nu))
    z = np.concatenate([xs[:, :H, :], us], axis=2)
    Zs = tuple(_ro(z[:, :, list(idx)].reshape(B * H, len(idx))) for idx in sp.var_inputs)
    return _ro(xs), _ro(us), Zs


@functools.lru_cache(maxsize=None)
def state_case(ns: tuple, seed: int):
    """Synthetic GPs of ns[g] rows, the iterate, and per GP the reference variance at its inputs
    (noise not included), its bound and the scaled inverse factor the handle is given."""
    xs, us, Zs = iterate(seed)
    out = []
    for g, (n, d) in enumerate(zip(ns, spec().gp_dims)):
        gp = R.synthetic_gp(n, d, seed=seed + 17 * g, sf2=SF2, sn2=SN2)
        ref = R.reference(gp["X"], gp["ell"], gp["sf2"], Zs[g], B=gp["Linv"].T, frac=0.4)
        out.append(dict(gp=gp, X=_ro(gp["X"]), Linv=_ro(ref["scale"] * gp["Linv"]), var=_ro(ref["var"]),
                        tol=_ro(ref["tol_var"])))
    return xs, us, tuple(out)


def handle_case(nt: int, r: int):
    return state_case((16 * (nt - 1) + r,) * 2, 100 * nt + r)


def mixed_case(n0: int, n1: int):
    return state_case((n0, n1), n0 + 3 * n1)


@functools.lru_cache(maxsize=None)
def free_case(n: int):
    """Handle-free (gpmpc_gp_posterior): GP of n rows, d = 2, its device layout zero padded to npad
    (host arrays) and the reference at FREE_POINTS points."""
    d = 2
    gp = R.synthetic_gp(n, d, seed=3000 + n)
    Z = R.points(FREE_POINTS, d, seed=3100 + n)
    ref = R.reference(gp["X"], gp["ell"], gp["sf2"], Z, B=gp["Linv"].T, frac=0.4)
    npad = (n + 15) // 16 * 16
    rows = np.zeros((npad, 4))
    rows[:n, :d] = gp["X"]
    lt = np.zeros((npad, npad))
    lt[:n, :n] = (ref["scale"] * gp["Linv"]).T
    return dict(gp=gp, npad=npad, rows=_ro(rows), linvT=_ro(lt), Z=_ro(Z), var=_ro(ref["var"]), tol=_ro(ref["tol_var"]))


@functools.lru_cache(maxsize=None)
def append_case():
    """Training data of the append case per GP (all APPEND_N0 + sum(APPEND_BLOCKS) rows), the
    iterate, and after each block the extended-precision predictive variance of the exact GP on the
    rows so far at the iterate's inputs (gp_append_ref.reference, which asserts it >= sn2 / 2)."""
    n = APPEND_N0 + sum(APPEND_BLOCKS)
    xs, us, Zs = iterate(4242)
    data, refs = [], []
    for g, d in enumerate(spec().gp_dims):
        gp = R.synthetic_gp(n, d, seed=4300 + 17 * g, sf2=APPEND_SF2, sn2=APPEND_SN2)
        data.append(dict(X=_ro(gp["X"]), y=_ro(np.sin(3.0 * gp["X"].sum(1)) + 0.5), ell=gp["ell"], d=d))
    at = APPEND_N0
    for m in APPEND_BLOCKS:
        at += m
        refs.append(tuple(_ro(fit_reference(dg["X"][:at], dg["y"][:at], dg["ell"], APPEND_SF2, APPEND_SN2, Zs[g])["var"])
                          for g, dg in enumerate(data)))
    return xs, us, tuple(data), tuple(refs)
