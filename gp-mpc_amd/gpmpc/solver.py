"""Batched solver handle: B independent GP-MPC instances on one MI355X.

Thin host layer over the C ABI (``include/gpmpc_mi355x.h``): it owns the solver handle,
uploads the OCP definition and the GP replicas, and runs one batched control step per
:meth:`BatchSolver.solve` (one ``gpmpc_solve`` call = the variance kernel + the SQP kernel,
asynchronous on torch's current stream).  All per-step tensors stay on the device.
"""

from __future__ import annotations

import ctypes

import numpy as np
import scipy.linalg
import scipy.stats
import torch

from . import _lib
from .gp import LOVE_CHOLESKY_ROWS, GaussianProcess
from .models import ModelSpec

STATUS_NAMES = {0: "SUCCESS", 1: "NAN_DETECTED", 2: "MAXITER", 3: "MINSTEP", 4: "QP_FAILURE"}


def discretize_linear_system(A, B, dt: float, exact: bool = False):
    """(Exact) ZOH discretisation (`gpmpc/gpmpc.py:517-527`)."""
    nx, nu = A.shape[1], B.shape[1]
    if exact:
        M = np.zeros((nx + nu, nx + nu))
        M[:nx, :nx] = A
        M[:nx, nx:] = B
        Md = scipy.linalg.expm(M * dt)
        return Md[:nx, :nx], Md[:nx, nx:]
    return np.eye(nx) + A * dt, B * dt


def setup_prior_dynamics(dfdx, dfdu, Q, R, dt):
    """LQR gain of the discretised prior (`gpmpc/gpmpc.py:500-507`)."""
    A, B = discretize_linear_system(dfdx, dfdu, dt, exact=True)
    P = scipy.linalg.solve_discrete_are(A, B, Q, R)
    btp = B.T @ P
    lqr_gain = -np.linalg.inv(R + btp @ B) @ (btp @ A)
    return A, B, lqr_gain


def inverse_cdf(prob: float, nx: int) -> float:
    """`gpmpc/gpmpc.py:63-65`."""
    return float(scipy.stats.norm.ppf(1 - (1 / nx - (prob + 1) / (2 * nx))))


def _c(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def predict_trajectory(solver, x0, u, with_gp: bool = True, return_var: bool = False, return_cov: bool = False,
                       feedback=None, with_noise: bool = False):
    """numpy front of ``solver.rollout`` (``GPMPC.predict_trajectory`` / ``MPC.predict_trajectory``): one trajectory,
    ``x0`` (nx,) and ``u`` (T, nu), gives ``x`` (T+1, nx); a batch, (P, nx) and (P, T, nu), gives (P, T+1, nx).  With
    ``return_var`` also the GP variances (T, n_gp) / (P, T, n_gp).  With ``return_cov`` (``solver.rollout_lin``) the
    state covariance (T+1, nx, nx) / (P, T+1, nx, nx) comes last, propagated from zero with ``feedback`` as the gain
    ``K`` (nu, nx) or None for the open loop, and the likelihood noise added when ``with_noise``."""
    x0 = np.asarray(x0, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    single = x0.ndim == 1
    if single:
        if u.ndim != 2:
            raise ValueError("one trajectory takes x0 (nx,) and u (T, nu)")
        x0, u = x0[None], u[None]
    elif x0.ndim != 2 or u.ndim != 3 or u.shape[0] != x0.shape[0]:
        raise ValueError("a batch takes x0 (P, nx) and u (P, T, nu)")
    dev = solver.device
    x0t, ut = torch.as_tensor(np.ascontiguousarray(x0), device=dev), torch.as_tensor(np.ascontiguousarray(u), device=dev)
    if return_cov:
        res = solver.rollout_lin(x0t, ut, with_gp=with_gp, var=return_var, cov=True, K=feedback, with_noise=with_noise)
        out = (res["x"],) + ((res["var"],) if return_var else ()) + (res["cov"],)
    else:
        out = solver.rollout(x0t, ut, with_gp=with_gp, var=return_var)
        out = out if return_var else (out,)
    out = tuple(t.cpu().numpy() for t in out)
    if single:
        out = tuple(a[0] for a in out)
    return out if return_var or return_cov else out[0]


class BatchSolver:
    """One solver handle for ``batch`` instances of ``spec`` with horizon ``horizon``.

    ``warm_start_shift=True`` turns on the one-stage shifted warm start (``set_tuning(shift=1)``);
    ``GPMPC`` and ``MPC`` pass it through their solver keywords."""

    def __init__(self, spec: ModelSpec, horizon: int, batch: int, device="cuda", prior_params: dict | None = None,
                 traj: np.ndarray | None = None, uh: float = -1e-8, cost_scaling: bool = True, max_iter: int = 25,
                 tol: float = 1e-6, qp_max_iter: int = 50, qp_tol: float | None = None, qp_mu0: float = 1.0,
                 warm_start_shift: bool = False):
        self.lib = _lib.load()
        self.spec = spec
        self.H = int(horizon)
        self.batch = int(batch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GPMPCError("BatchSolver runs on the GPU (device must be cuda)")
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self.dev_index)
        self.nx, self.nu = spec.nx, spec.nu
        h = ctypes.c_void_p()
        _lib.check(self.lib.gpmpc_create(spec.model_id, self.H, self.batch, self.dev_index, ctypes.byref(h)))
        self._h = h
        self._uh, self._cost_scaling = float(uh), int(cost_scaling)
        self.set_prior(prior_params)
        self.set_options(max_iter=max_iter, tol=tol, qp_max_iter=qp_max_iter, qp_tol=qp_tol, qp_mu0=qp_mu0)
        self.set_reference(spec.reference_trajectory() if traj is None else traj)
        self.set_var_inputs(spec.var_inputs)
        self.tuning: dict[str, int] = {}   # options set through set_tuning (the others are on their default)
        if warm_start_shift:
            self.set_tuning(shift=1)
        self.gps: list[GaussianProcess] | None = None
        # per-step device buffers
        kw = dict(device=self.device)
        B = self.batch
        self.u0 = torch.zeros(B, self.nu, dtype=torch.float64, **kw)
        self.status = torch.zeros(B, dtype=torch.int32, **kw)
        self.sqp_iter = torch.zeros(B, dtype=torch.int32, **kw)
        self.qp_iter = torch.zeros(B, dtype=torch.int32, **kw)
        self.res = torch.zeros(B, 4, dtype=torch.float64, **kw)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib._lib is not None:
            _lib._lib.gpmpc_destroy(h)
            self._h = None

    # ------------------------------------------------------------------ configuration
    def set_prior(self, prior_params: dict | None = None):
        """Prior model parameters (``spec.prior`` updated by ``prior_params``), bounds, weights."""
        spec = self.spec
        self.prior = dict(spec.prior if prior_params is None else {**spec.prior, **prior_params})
        params = _c(spec.param_vector(self.prior))
        self._keep = [params]
        _lib.check(self.lib.gpmpc_set_model(
            self._h, params.ctypes.data, params.size, spec.dt, _c(spec.x_lo).ctypes.data, _c(spec.x_hi).ctypes.data,
            _c(spec.u_lo).ctypes.data, _c(spec.u_hi).ctypes.data, _c(spec.q_diag).ctypes.data,
            _c(spec.r_diag).ctypes.data, _c(spec.u_eq).ctypes.data, self._uh, self._cost_scaling))

    def set_options(self, max_iter=25, tol=1e-6, qp_max_iter=50, qp_tol=None, qp_mu0=1.0):
        """SQP / QP options (gpmpc_set_options).  ``qp_tol=None``: the QP solves to the NLP tolerance,
        as acados passes its NLP tolerances on to the QP solver when the OCP leaves the QP
        tolerances unset (`gpmpc/gpmpc.py:257-263`)."""
        qp_tol = tol if qp_tol is None else qp_tol
        _lib.check(self.lib.gpmpc_set_options(self._h, int(max_iter), tol, tol, tol, tol, int(qp_max_iter), qp_tol, qp_mu0))

    def set_reference(self, traj: np.ndarray):
        traj = _c(traj)
        if traj.ndim != 2 or traj.shape[0] != self.nx:
            raise ValueError(f"reference trajectory must be (nx={self.nx}, L)")
        self.traj = traj
        _lib.check(self.lib.gpmpc_set_reference(self._h, traj.ctypes.data, traj.shape[1]))

    def set_gps(self, gps: list[GaussianProcess] | None, with_variance: bool = True, fitc: list | None = None,
                variance: str = "exact", love_rank: int = 100, love_force: bool = False):
        """Upload GP replicas.  ``fitc[g] = (S (M,d), w (M,))`` replaces GP g's mean by the FITC
        approximation (the variance stays exact, as in `gpmpc/gpmpc.py:441-445`).

        ``variance="love"``: the tightening variance of GPs with more than
        ``LOVE_CHOLESKY_ROWS`` (800) training rows uses the rank-``love_rank`` Lanczos root
        (`GaussianProcess.love_root`), as gpytorch's ``fast_pred_var`` does in the reference
        (`gpmpc/gpmpc.py:442-444`); smaller GPs keep the exact root, like gpytorch's Cholesky
        path.  ``love_force`` applies the Lanczos root at every size (tests)."""
        if variance not in ("exact", "love"):
            raise ValueError("variance must be 'exact' or 'love'")
        self.love_ranks = [None] * self.spec.n_gp   # columns of each GP's LOVE root (None: exact)
        self.love_roots = [None] * self.spec.n_gp   # the installed roots (host, float64), for checkers
        self.love_rank = int(love_rank)             # the rank later device-built roots ask for (GPMPC)
        self.fitc_sizes = [0] * self.spec.n_gp      # inducing rows of each GP's device-built FITC mean (0: none)
        if gps is None:
            _lib.check(self.lib.gpmpc_use_gp(self._h, 0))
            self.gps = None
            return
        if len(gps) != self.spec.n_gp:
            raise ValueError(f"{self.spec.name} needs {self.spec.n_gp} GPs")
        for g, gp in enumerate(gps):
            lay = gp.device_layout("cpu")
            X = _c(gp.train_inputs[0].cpu().numpy())
            Linv = _c(lay["Linv"].cpu().numpy()) if with_variance else None
            if fitc is not None and fitc[g] is not None:
                S, w = _c(fitc[g][0]), _c(fitc[g][1])
                _lib.check(self.lib.gpmpc_set_gp(self._h, g, S.shape[0], S.shape[1], S.ctypes.data, w.ctypes.data,
                                                 X.shape[0], X.ctypes.data, None if Linv is None else Linv.ctypes.data,
                                                 gp.lengthscale, gp.outputscale, gp.noise))
            else:
                alpha = _c(lay["alpha"].cpu().numpy())
                _lib.check(self.lib.gpmpc_set_gp(self._h, g, X.shape[0], X.shape[1], X.ctypes.data, alpha.ctypes.data,
                                                 0, None, None if Linv is None else Linv.ctypes.data,
                                                 gp.lengthscale, gp.outputscale, gp.noise))
            if with_variance and variance == "love" and (love_force or X.shape[0] > LOVE_CHOLESKY_ROWS):
                R = _c(gp.love_root(love_rank).cpu().numpy())
                _lib.check(self.lib.gpmpc_set_gp_variance_root(self._h, g, R.shape[0], R.shape[1], R.ctypes.data))
                self.love_ranks[g] = R.shape[1]
                self.love_roots[g] = R
        _lib.check(self.lib.gpmpc_use_gp(self._h, 1))
        self.gps = gps

    def reserve_gp(self, gp_id: int, capacity: int):
        """Room for up to ``capacity`` training rows of the handle's GP ``gp_id`` (gpmpc_gp_reserve;
        after ``set_gps``, which resets the capacity to the uploaded size; a synchronous setup call)."""
        _lib.check(self.lib.gpmpc_gp_reserve(self._h, int(gp_id), int(capacity)))

    def append_gp(self, gp_id: int, X, y) -> torch.Tensor:
        """Append training rows X (m, d), y (m,) to the handle's GP ``gp_id`` on the current stream
        (gpmpc_gp_append): one bordered-Cholesky update per block of up to 16 rows, hyperparameters
        unchanged.  cuda or host tensors (or arrays); no synchronisation of its own.  Returns the
        accepted flags, a device int32 tensor with one entry per block (1 accepted, 0 written as
        inert rows).  The Python GP objects are not touched (``GaussianProcess.append_data``)."""
        X = torch.as_tensor(X).to(self.device, torch.float64)
        y = torch.as_tensor(y).to(self.device, torch.float64).reshape(-1).contiguous()
        if X.ndim == 1:
            X = X[:, None]
        X = X.contiguous()
        m, d = X.shape
        if y.shape[0] != m:
            raise ValueError("X and y disagree on the number of rows")
        if d != self.spec.gp_dims[int(gp_id)]:
            raise ValueError(f"GP {gp_id} takes inputs of dimension {self.spec.gp_dims[int(gp_id)]}, got {d}")
        flags = torch.empty((m + 15) // 16, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gpmpc_gp_append(self._h, int(gp_id), m, X.data_ptr(), y.data_ptr(), flags.data_ptr(),
                                            self._stream()))
        return flags

    def drop_gp(self, gp_id: int, m: int) -> torch.Tensor:
        """Remove the ``m`` oldest training rows of the handle's GP ``gp_id`` on the current stream
        (gpmpc_gp_drop_oldest): one update of the inverse factor and the weights per block of up to
        16 rows, hyperparameters unchanged, no refactorisation and no synchronisation of its own; row
        ``j + m`` becomes row ``j`` and the capacity stays.  Needs ``reserve_gp`` and leaves at least
        one row.  Returns the status flags, a device int32 tensor with one entry per block (1: every
        pivot was finite and positive; 0: the GP's contents are unspecified, upload it again).  The
        Python GP objects are not touched (``GaussianProcess.drop_oldest``)."""
        m = int(m)
        flags = torch.empty(max((m + 15) // 16, 1), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gpmpc_gp_drop_oldest(self._h, int(gp_id), m, flags.data_ptr(), self._stream()))
        return flags

    def drop_rows(self, gp_id: int, idx) -> tuple[torch.Tensor, torch.Tensor]:
        """Remove the training rows ``idx`` names (int32 indices into the rows as they are now; a cuda or host
        tensor or an array) of the handle's GP ``gp_id`` on the current stream (gpmpc_gp_drop_rows): ``drop_gp`` for
        an arbitrary set, the kept rows keeping their order; no refactorisation and no synchronisation of its own.
        Needs ``reserve_gp`` and leaves at least one row.  Returns ``(dropped, ok)``, device int32 tensors: the rows
        actually dropped, ascending (m,), and the flag [1], 1 when the indices were distinct values in range and
        every pivot was finite and positive.  Indices that are not come out as the distinct ones in range, filled
        up with the lowest rows not among them, and ok 0 with the GP valid; after a 0 caused by a pivot the GP's
        contents are unspecified, upload it again.  The Python GP objects are not touched
        (``GaussianProcess.drop_rows``)."""
        idx = torch.as_tensor(idx).to(self.device, torch.int32).reshape(-1).contiguous()
        m = int(idx.shape[0])
        dropped = torch.empty(max(m, 1), dtype=torch.int32, device=self.device)
        ok = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gpmpc_gp_drop_rows(self._h, int(gp_id), m, idx.data_ptr() if m else None,
                                               dropped.data_ptr(), ok.data_ptr(), self._stream()))
        return dropped[:m], ok

    def redundant(self, m: int, scores: bool = False):
        """The ``m`` <= 256 training rows the handle's GPs would miss least (gpmpc_gp_redundant), one after the
        other: each pick is the row whose latent leave-one-out variance, the largest over the GPs divided by the
        outputscale, is smallest once the picks before it are gone, so of a cluster of near-copies all but one
        leave before a row that covers a region alone.  Ties go to the lower (older) index.  Returns the device
        int32 picks (m,), with ``scores=True`` also the (m,) scores at which they were picked and the int32 flag
        tensor [1] (0: a pivot was not finite and positive, and that GP skipped that pick).  On the current
        stream, no synchronisation of its own; nothing of the GPs changes."""
        m = int(m)
        pick = torch.empty(max(m, 1), dtype=torch.int32, device=self.device)   # (never empty: the refusal is the library's)
        score = torch.empty(max(m, 1), dtype=torch.float64, device=self.device) if scores else None
        ok = torch.empty(1, dtype=torch.int32, device=self.device) if scores else None
        _lib.check(self.lib.gpmpc_gp_redundant(self._h, m, pick.data_ptr(), _lib.ptr(score), _lib.ptr(ok), self._stream()))
        return (pick[:m], score[:m], ok) if scores else pick[:m]

    # ------------------------------------------------------------------ training data on the device
    def _diff_constants(self) -> tuple[float, float]:
        """(dt_diff, gravity) of ``GPMPC.preprocess_data``: the reference's literals 1/60 and 9.81 for quad3d
        (`gpmpc/gpmpc.py:113-151`), the model's own dt and gravity otherwise."""
        return (1 / 60, 9.81) if self.spec.name == "quad3d" else (self.spec.dt, self.spec.gravity)

    def _transitions(self, x, u, x_next=None):
        """x (P, nx), u (P, nu) and x_next (P, nx) as contiguous float64 device tensors."""
        x = torch.as_tensor(x).to(self.device, torch.float64).reshape(-1, self.nx).contiguous()
        u = torch.as_tensor(u).to(self.device, torch.float64).reshape(-1, self.nu).contiguous()
        if u.shape[0] != x.shape[0]:
            raise ValueError("x and u disagree on the number of transitions")
        if x_next is None:
            return x, u
        x_next = torch.as_tensor(x_next).to(self.device, torch.float64).reshape(-1, self.nx).contiguous()
        if x_next.shape[0] != x.shape[0]:
            raise ValueError("x and x_next disagree on the number of transitions")
        return x, u, x_next

    def _picks(self, pick, m, P):
        """(pick as an int32 device tensor or None, rows m): ``pick`` given, its length is m; else rows 0 .. m-1
        (all P by default)."""
        if pick is None:
            return None, int(P if m is None else m)
        pick = torch.as_tensor(pick).to(self.device, torch.int32).reshape(-1).contiguous()
        if m is not None and int(m) != pick.shape[0]:
            raise ValueError(f"pick holds {pick.shape[0]} indices, m is {m}")
        return pick, int(pick.shape[0])

    def preprocess(self, x, u, x_next, pick=None, m=None):
        """GP training inputs (m, sum d_g) and targets (m, n_gp) from transitions x (P, nx), u (P, nu),
        x_next (P, nx), on the current stream (gpmpc_preprocess): ``GPMPC.preprocess_data`` on the device, at the
        handle's prior parameters.  Row r comes from transition ``pick[r]`` (int32 indices; an index outside
        0 .. P-1 gives a row of NaN), or from transition r of the first ``m`` (default all) without ``pick``.
        cuda or host tensors (or arrays); no synchronisation of its own.  Returns device tensors."""
        x, u, x_next = self._transitions(x, u, x_next)
        pick, m = self._picks(pick, m, x.shape[0])
        inputs = torch.empty(max(m, 0), sum(self.spec.gp_dims), dtype=torch.float64, device=self.device)
        targets = torch.empty(max(m, 0), self.spec.n_gp, dtype=torch.float64, device=self.device)
        dt_diff, gravity = self._diff_constants()
        _lib.check(self.lib.gpmpc_preprocess(self._h, x.shape[0], x.data_ptr(), u.data_ptr(), x_next.data_ptr(), m,
                                             _lib.ptr(pick), dt_diff, gravity, inputs.data_ptr(), targets.data_ptr(),
                                             self._stream()))
        return inputs, targets

    def informative(self, x, u, m: int, scores: bool = False):
        """The ``m`` of the P <= batch points (x (P, nx), u (P, nu)) where the handle's GPs are least certain
        (gpmpc_gp_informative): a device int32 tensor (m,) of indices by decreasing score, the score being the
        largest exact posterior variance over the GPs, each divided by its outputscale (no likelihood noise; LOVE
        roots and FITC means are ignored).  Ties go to the lower index, a non-finite score ranks last.  The picks
        are the most uncertain points one by one; redundancy among them is not accounted for.  On the current
        stream, no synchronisation of its own.  ``scores=True`` also returns the (P,) scores."""
        x, u = self._transitions(x, u)
        P = x.shape[0]
        pick = torch.empty(max(int(m), 0), dtype=torch.int32, device=self.device)
        score = torch.empty(P, dtype=torch.float64, device=self.device) if scores else None
        _lib.check(self.lib.gpmpc_gp_informative(self._h, P, x.data_ptr(), u.data_ptr(), int(m), pick.data_ptr(),
                                                 _lib.ptr(score), self._stream()))
        return (pick, score) if scores else pick

    def select(self, x, u, m: int, gains: bool = False, resid: bool = False):
        """Greedy conditional-variance selection of ``m`` <= 256 of the P <= batch points (gpmpc_gp_select): each
        pick is the point with the largest score of ``informative`` once the picks before it count as observed
        (with the likelihood noise), so near-duplicates of a pick are not picked after it.  Pick 0 and its gain are
        ``informative``'s top pick and score, bit for bit.  Returns the device int32 picks (m,), then with
        ``gains=True`` the (m,) scores at which they were picked, with ``resid=True`` the (n_gp, P) posterior
        variances (no noise) of the GPs with the picks added, and last the int32 flag tensor [1] (0: a pivot was not
        finite and positive, and that GP skipped that pick).  On the current stream, no synchronisation of its own;
        nothing of the GPs changes."""
        x, u = self._transitions(x, u)
        P = x.shape[0]
        pick = torch.empty(max(int(m), 0), dtype=torch.int32, device=self.device)
        gain = torch.empty(max(int(m), 0), dtype=torch.float64, device=self.device) if gains else None
        res = torch.empty(self.spec.n_gp, P, dtype=torch.float64, device=self.device) if resid else None
        ok = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gpmpc_gp_select(self._h, P, x.data_ptr(), u.data_ptr(), int(m), pick.data_ptr(),
                                            _lib.ptr(gain), _lib.ptr(res), ok.data_ptr(), self._stream()))
        return tuple(t for t in (pick, gain, res, ok) if t is not None)

    def observe(self, x, u, x_next, pick=None, m=None, evict_oldest: bool = False):
        """``preprocess`` followed by an append of the m rows to every GP of the handle, in one call on the
        current stream (gpmpc_gp_observe; m <= batch): bit-identical to ``preprocess``, a column slice per GP,
        ``drop_gp`` where needed and ``append_gp``.  With ``evict_oldest`` and n + m above the capacity exactly
        the excess is dropped from the old end of every GP first.  Returns ``(inputs, targets, accepted,
        dropped_ok)``: the rows as ``preprocess`` returns them (the caller keeps the targets) and the int32 flags
        (n_gp, blocks) of ``append_gp`` and ``drop_gp`` (1 where nothing was dropped).  No synchronisation of its
        own.  The Python GP objects are not touched."""
        x, u, x_next = self._transitions(x, u, x_next)
        pick, m = self._picks(pick, m, x.shape[0])
        n_gp = self.spec.n_gp
        try:
            n, cap = self.gp_size(0)
        except _lib.GPMPCError:   # (an unset GP is the library's refusal below, like every other precondition)
            n, cap = 0, 0
        excess = max(n + m - cap, 0) if evict_oldest else 0
        inputs = torch.empty(max(m, 0), sum(self.spec.gp_dims), dtype=torch.float64, device=self.device)
        targets = torch.empty(max(m, 0), n_gp, dtype=torch.float64, device=self.device)
        accepted = torch.empty(n_gp, max((m + 15) // 16, 1), dtype=torch.int32, device=self.device)
        dropped_ok = torch.empty(n_gp, max((excess + 15) // 16, 1), dtype=torch.int32, device=self.device)
        dt_diff, gravity = self._diff_constants()
        _lib.check(self.lib.gpmpc_gp_observe(self._h, x.shape[0], x.data_ptr(), u.data_ptr(), x_next.data_ptr(), m,
                                             _lib.ptr(pick), dt_diff, gravity, int(bool(evict_oldest)),
                                             inputs.data_ptr(), targets.data_ptr(), accepted.data_ptr(),
                                             dropped_ok.data_ptr(), self._stream()))
        return inputs, targets, accepted, dropped_ok

    def refactor_gp(self, gp_id: int, y, lengthscale: float, outputscale: float, noise: float) -> torch.Tensor:
        """Factorise the handle's GP ``gp_id`` again from scratch on the current stream
        (gpmpc_gp_refactor): from the handle's own training inputs, the targets ``y`` (n,) of its n
        current rows in row order (``gp_size``; inert rows included, their entries are ignored) and
        the hyperparameters given.  With the GP's current hyperparameters it refreshes a factor that
        appends and drops have let drift; with new ones it applies a refit.  cuda or host tensors (or
        arrays); no synchronisation of its own.  Needs ``reserve_gp``.  Returns the status flag, a
        device int32 tensor [1] (1: every live target finite and every pivot finite and positive; 0:
        the GP's contents are unspecified, upload it again).  The Python GP objects are not touched
        (``GaussianProcess.set_hyperparameters``)."""
        y = self._targets(gp_id, y)
        flag = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gpmpc_gp_refactor(self._h, int(gp_id), y.data_ptr() if y.numel() else None,
                                              float(lengthscale), float(outputscale), float(noise), flag.data_ptr(),
                                              self._stream()))
        return flag

    def _targets(self, gp_id: int, y) -> torch.Tensor:
        """The n targets of GP ``gp_id``'s current rows on the device (an unset GP is the library's refusal,
        like every other precondition)."""
        y = torch.as_tensor(y).to(self.device, torch.float64).reshape(-1).contiguous()
        n = self.gp_size(gp_id)[0] if y.numel() else 0
        if y.numel() and y.shape[0] != n:
            raise ValueError(f"GP {gp_id} has {n} training rows, got {y.shape[0]} targets")
        return y

    def gp_mll(self, gp_id: int, y) -> torch.Tensor:
        """Marginal log likelihood per live row of the handle's GP ``gp_id`` and its gradient, a device
        tensor [4] = (MLL / n, d/d lengthscale, d/d outputscale, d/d noise), on the current stream
        (gpmpc_gp_mll): from the factor, inputs and weights the handle holds and the targets ``y`` (n,)
        of its n current rows (inert rows' entries are ignored).  Nothing of the GP changes; no
        synchronisation of its own.  Needs ``reserve_gp``."""
        y = self._targets(gp_id, y)
        out = torch.empty(4, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.gpmpc_gp_mll(self._h, int(gp_id), y.data_ptr() if y.numel() else None, out.data_ptr(),
                                         self._stream()))
        return out

    def fit_gp(self, gp_id: int, y, raw, lr: float, iterations: int, history=False):
        """Fit the hyperparameters of the handle's GP ``gp_id`` on the device (gpmpc_gp_fit): the loop
        of ``gpmpc.gp.fit_gp`` (Adam on -MLL / n over the raw softplus parameters, early stop at
        |dloss| < 1e-3) from ``raw`` (3,), on the targets ``y`` (n,) of the GP's n current rows, with
        no host round trip per iteration.  The call synchronises the current stream and leaves the GP
        refactorised at the fitted hyperparameters.  Returns ``(raw, iters, ok)``: the fitted raw
        parameters (numpy (3,); the ones passed in when ok is 0), the iterations run and the status.
        ``history=True`` appends the (iters, 4) array of (loss before the step, raw after it);
        a contiguous float64 device tensor of at least ``4 * iterations`` elements is written in place
        and returned whole.  Needs ``reserve_gp``.  The Python GP objects are not touched."""
        y = self._targets(gp_id, y)
        raw = np.array(raw, dtype=np.float64).reshape(-1).copy()
        if raw.shape[0] != 3:
            raise ValueError("raw must hold the three raw parameters (lengthscale, outputscale, noise)")
        iterations = int(iterations)
        hist = None
        if isinstance(history, torch.Tensor):
            if history.dtype != torch.float64 or history.device != self.device or not history.is_contiguous() \
                    or history.numel() < 4 * iterations:
                raise ValueError(f"history must be a contiguous float64 tensor of >= {4 * iterations} elements on {self.device}")
            hist = history
        elif history:
            hist = torch.empty(max(iterations, 1), 4, dtype=torch.float64, device=self.device)
        iters, ok = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.gpmpc_gp_fit(self._h, int(gp_id), y.data_ptr() if y.numel() else None, float(lr), iterations,
                                         raw.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(iters),
                                         ctypes.byref(ok), _lib.ptr(hist), self._stream()))
        if hist is None:
            return raw, iters.value, ok.value
        return raw, iters.value, ok.value, (hist if isinstance(history, torch.Tensor) else hist[:iters.value].cpu().numpy())

    def love_root_gp(self, gp_id: int, rank: int = 100, seed: int = 0, start=None) -> tuple[int, int]:
        """Build the LOVE variance root of the handle's GP ``gp_id`` on the device and install it
        (gpmpc_gp_love_root): Lanczos with full reorthogonalisation on k(X, X) + noise I, generated from
        the handle's own rows and current hyperparameters, so it follows appends, drops and refits
        without an upload.  The start vector is the seeded ``torch.randn`` draw of
        ``GaussianProcess.love_root(rank, seed)`` over the GP's n current rows (inert rows included),
        or ``start`` (n,); entries of inert rows are ignored.  The call synchronises the current
        stream.  Returns ``(rank, ok)``: the installed root's rank (at most ``min(rank, live rows)``)
        and 1, or ``(0, 0)`` with the handle, ``love_ranks`` and ``love_roots`` unchanged.  Needs
        ``reserve_gp``; a root already installed is replaced."""
        n = self.gp_size(gp_id)[0]
        if start is None:
            gen = torch.Generator(device="cpu").manual_seed(int(seed))
            start = torch.randn(n, dtype=torch.float64, generator=gen)
        q0 = torch.as_tensor(start).to(self.device, torch.float64).reshape(-1).contiguous()
        if q0.shape[0] != n:
            raise ValueError(f"GP {gp_id} has {n} training rows, got a start vector of {q0.shape[0]}")
        r, ok = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.gpmpc_gp_love_root(self._h, int(gp_id), int(rank), q0.data_ptr(), ctypes.byref(r),
                                               ctypes.byref(ok), self._stream()))
        if ok.value:
            self.love_ranks[int(gp_id)] = r.value
            self.love_roots[int(gp_id)] = self.variance_root(gp_id)
        return r.value, ok.value

    def variance_root(self, gp_id: int) -> np.ndarray:
        """The LOVE root installed for the handle's GP ``gp_id``, read back from the device
        (gpmpc_get_gp_variance_root): float64 (n, r); the library refuses when none is installed."""
        n, r = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.gpmpc_get_gp_variance_root(self._h, int(gp_id), ctypes.byref(n), ctypes.byref(r), None, None))
        R = torch.empty(n.value, r.value, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.gpmpc_get_gp_variance_root(self._h, int(gp_id), None, None, R.data_ptr(), self._stream()))
        return R.cpu().numpy()

    def drop_love_root(self, gp_id: int):
        """Back to the exact tightening variance for the handle's GP ``gp_id``
        (gpmpc_set_gp_variance_root with R = NULL): what the device-side updates ask for first."""
        _lib.check(self.lib.gpmpc_set_gp_variance_root(self._h, int(gp_id), 0, 0, None))
        self.love_ranks[int(gp_id)] = None
        self.love_roots[int(gp_id)] = None

    def fitc_gp(self, gp_id: int, idx, y, jitter: float = 0.0) -> int:
        """Build the FITC inducing-point mean of the handle's GP ``gp_id`` on the device and install it as the
        mean the solver reads (gpmpc_gp_fitc): the weights of the inducing rows ``X[idx]`` (M distinct row
        indices, 1 <= M <= n) from the handle's own training rows, its current hyperparameters and the
        targets ``y`` (n,) of its n current rows (``gp_size``; inert rows' entries are ignored), with ``jitter``
        added to the diagonal of K_ss (0: the reference's formula).  cuda or host tensors (or arrays), moved
        to the device if needed; runs on the current stream and synchronises it.  The exact GP stays in the
        handle beside the FITC mean: ``gp_size`` and the variance are unchanged.  Returns 1, or 0 with the
        handle and ``fitc_sizes`` unchanged (a pivot or a Gamma not positive, a target not finite, an index
        that names an inert row or lies outside 0 .. n-1).  Needs ``reserve_gp``; a FITC mean already
        installed is replaced on success."""
        idx = torch.as_tensor(idx).to(self.device, torch.int32).reshape(-1).contiguous()
        y = self._targets(gp_id, y)
        ok = ctypes.c_int32()
        _lib.check(self.lib.gpmpc_gp_fitc(self._h, int(gp_id), int(idx.shape[0]), idx.data_ptr() if idx.numel() else None,
                                          y.data_ptr() if y.numel() else None, float(jitter), ctypes.byref(ok),
                                          self._stream()))
        if ok.value:
            self.fitc_sizes[int(gp_id)] = int(idx.shape[0])
        return ok.value

    def inducing_gp(self, gp_id: int, M: int, tol: float = 0.0, gains: bool = False, resid: bool = False):
        """Choose up to ``M`` of the n training rows of the handle's GP ``gp_id`` as FITC inducing rows, on the
        device (gpmpc_gp_inducing): greedily by residual prior variance, a pivoted partial Cholesky of k(X, X) at
        the GP's current hyperparameters, which ends when no row's residual variance exceeds ``tol`` times the
        outputscale.  Near-copies of a picked row are never picked, and with ``tol > 0`` the picks give
        ``fitc_gp(..., jitter=0)`` pivots bounded below.  Inert rows are never picked.  Returns ``idx``, the device
        int32 picks in pick order (their count is its length, at most M), then with ``gains=True`` the scores at
        which they were picked (non-increasing up to rounding, 1.0 first) and with ``resid=True`` the (n,) residual
        variances (0 for an inert row).  The call synchronises the current stream first and returns with its work
        completed (it runs on a stream of the handle's own).  Needs ``reserve_gp``; nothing of the GP changes."""
        M = int(M)
        n = self.gp_size(gp_id)[0]
        idx = torch.empty(max(M, 1), dtype=torch.int32, device=self.device)   # (never empty: the refusal is the library's)
        gain = torch.empty(max(M, 1), dtype=torch.float64, device=self.device) if gains else None
        res = torch.empty(n, dtype=torch.float64, device=self.device) if resid else None
        torch.cuda.current_stream(self.device).synchronize()   # (nothing still queued on memory the outputs reuse)
        count = ctypes.c_int32()
        _lib.check(self.lib.gpmpc_gp_inducing(self._h, int(gp_id), M, float(tol), idx.data_ptr(), _lib.ptr(gain),
                                              _lib.ptr(res), ctypes.byref(count)))
        out = (idx[:count.value], None if gain is None else gain[:count.value], res)
        return out[0] if not (gains or resid) else tuple(t for t in out if t is not None)

    def drop_fitc(self, gp_id: int):
        """Back to the exact mean for the handle's GP ``gp_id`` (gpmpc_gp_fitc with M = 0): what the
        device-side updates ask for first.  Queued on the current stream, no synchronisation."""
        _lib.check(self.lib.gpmpc_gp_fitc(self._h, int(gp_id), 0, None, None, 0.0, None, self._stream()))
        self.fitc_sizes[int(gp_id)] = 0

    def fitc_size(self, gp_id: int) -> int:
        """Inducing rows of the FITC mean ``fitc_gp`` installed for GP ``gp_id``, 0 when none is (gpmpc_get_gp_fitc)."""
        m = ctypes.c_int32()
        _lib.check(self.lib.gpmpc_get_gp_fitc(self._h, int(gp_id), ctypes.byref(m), None, None, None))
        return m.value

    def fitc_mean(self, gp_id: int) -> tuple[np.ndarray, np.ndarray]:
        """(indices (M,) int32, weights (M,) float64) of the installed FITC mean, read back from the device."""
        m = self.fitc_size(gp_id)
        idx = torch.empty(m, dtype=torch.int32, device=self.device)
        w = torch.empty(m, dtype=torch.float64, device=self.device)
        if m:
            _lib.check(self.lib.gpmpc_get_gp_fitc(self._h, int(gp_id), None, idx.data_ptr(), w.data_ptr(), self._stream()))
        return idx.cpu().numpy(), w.cpu().numpy()

    def gp_size(self, gp_id: int) -> tuple[int, int]:
        """(training rows, capacity) of the handle's GP ``gp_id`` (gpmpc_gp_size)."""
        n, cap = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.gpmpc_gp_size(self._h, int(gp_id), ctypes.byref(n), ctypes.byref(cap)))
        return n.value, cap.value

    def gp_mean_grad(self, gp_id: int, z: torch.Tensor):
        """GP mean (P,) and input gradient (P, d) at z (P, d) through the linearisation's MFMA tile
        sums (the casadi mean + AD of `gpmpc/gp.py:72-85`, `gpmpc/gpmpc.py:189-209`)."""
        z = z.to(self.device, torch.float64).contiguous()
        P = z.shape[0]
        mean = torch.empty(P, dtype=torch.float64, device=self.device)
        grad = torch.empty(P, z.shape[1], dtype=torch.float64, device=self.device)
        _lib.check(self.lib.gpmpc_gp_mean_grad(self._h, int(gp_id), z.data_ptr(), P, mean.data_ptr(),
                                               grad.data_ptr(), self._stream()))
        return mean, grad

    def gp_predict(self, gp_id: int, z: torch.Tensor, with_noise: bool = False, mean: bool = True, var: bool = True):
        """Posterior mean (P,) and exact variance (P,) of the handle's GP ``gp_id`` at z (P, d)
        (gpmpc_gp_predict; ``with_noise`` adds the likelihood noise to the variance).  ``mean`` /
        ``var``: True allocates the output, False leaves it out (None is returned in its place), a
        contiguous float64 tensor of at least P elements on the solver's device is written in place.
        The variance needs the GP's Linv (``with_variance``)."""
        z = z.to(self.device, torch.float64).contiguous()
        P = z.shape[0]

        def out(o):
            if isinstance(o, torch.Tensor):
                if o.dtype != torch.float64 or o.device != self.device or not o.is_contiguous() or o.numel() < P:
                    raise ValueError(f"output must be a contiguous float64 tensor of >= {P} elements on {self.device}")
                return o
            return torch.empty(P, dtype=torch.float64, device=self.device) if o else None

        m, v = out(mean), out(var)
        _lib.check(self.lib.gpmpc_gp_predict(self._h, int(gp_id), z.data_ptr(), P, _lib.ptr(m), _lib.ptr(v),
                                             int(with_noise), self._stream()))
        return m, v

    def set_var_inputs(self, var_inputs):
        """Per-GP input map of the tightening variance (indices into z = [x; u]); see
        gpmpc_set_var_inputs.  ``spec.var_inputs`` (the reference's map) is the default."""
        for g, idx in enumerate(var_inputs):
            a = np.ascontiguousarray(idx, dtype=np.int32)
            _lib.check(self.lib.gpmpc_set_var_inputs(self._h, g, a.ctypes.data, len(a)))

    def set_tightening(self, enabled: bool, prob: float = 0.95, Ad=None, Bd=None, K=None):
        if not enabled:
            _lib.check(self.lib.gpmpc_set_tightening(self._h, 0, 0.0, None, None, None))
            return
        Ad, Bd, K = _c(Ad), _c(Bd), _c(K)
        self._keep += [Ad, Bd, K]
        _lib.check(self.lib.gpmpc_set_tightening(self._h, 1, inverse_cdf(prob, self.nx), Ad.ctypes.data,
                                                 Bd.ctypes.data, K.ctypes.data))

    STATS_SLOTS = 12

    def set_stats(self, buf: torch.Tensor | None):
        """Device int64 (B, 10) accumulator of SQP/QP iteration sums, status counts and the
        largest SQP / QP iteration counts of one solve (or None); see gpmpc_set_stats_buffer."""
        if buf is not None:
            assert buf.shape == (self.batch, self.STATS_SLOTS) and buf.dtype == torch.int64 and buf.device == self.device
        self._stats = buf
        _lib.check(self.lib.gpmpc_set_stats_buffer(self._h, None if buf is None else buf.data_ptr(), self.STATS_SLOTS))

    def set_launch(self, waves: int = 0):
        """SQP-kernel launch shape (gpmpc_set_launch): waves per instance (0 auto, 1, 2, 4; quad3d:
        0 or 4).  A performance option; results agree to rounding."""
        _lib.check(self.lib.gpmpc_set_launch(self._h, int(waves)))

    def launch_info(self) -> dict:
        """What a solve of this batch runs (gpmpc_get_launch_info, gpmpc_get_launch_segments): SQP
        waves per instance, horizon segments of its Newton solves, and whether a step with a variance
        launch runs as overlapped halves (then the profiling events bracket spans of the step, not
        single kernels)."""
        w, o, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.gpmpc_get_launch_info(self._h, self.batch, ctypes.byref(w), ctypes.byref(o)))
        _lib.check(self.lib.gpmpc_get_launch_segments(self._h, self.batch, ctypes.byref(g)))
        return {"waves": w.value, "segments": g.value, "overlapped": o.value == 1, "tail_boost": o.value == 2}

    def set_tuning(self, **opts):
        """Performance switches (gpmpc_set_tuning): lin_cache=0/1, order=0/1/2, overlap=0/1,
        var_split=0/1/4, event_fence=0/1, seg=0/1, tail=K, seg_pivot=k, var_trim=0/1.  Outputs do not depend on them (A/B knobs;
        var_trim: the tightening variances agree to rounding).

        shift=0/1 is the exception.  With 1, an instance whose previous solve ended with status 0 or 2
        and whose ``tstep`` has advanced by exactly one (modulo the reference length) starts its SQP
        from the stored solution and multipliers moved up one stage, the terminal stage duplicated;
        every other solve (first, after ``reset`` / ``set_iterate``, after a failed solve, repeated or
        jumped ``tstep``) runs as with 0.  The tightening and ``solution()`` still use the unshifted
        stored solution, so the converged result agrees to the solver tolerance while ``sqp_iter`` /
        ``qp_iter`` change; such a solve recomputes its first linearisation.  Default 0."""
        for k, v in opts.items():
            if k not in _lib.TUNE:
                raise ValueError(f"unknown tuning option {k!r} (one of {sorted(_lib.TUNE)})")
            _lib.check(self.lib.gpmpc_set_tuning(self._h, _lib.TUNE[k], int(v)))
            self.tuning[k] = int(v)

    def set_cost_output(self, enabled: bool = True) -> torch.Tensor | None:
        """Per-stage LINEAR_LS costs of every solve's new solution into ``self.stage_cost`` (B, H+1)
        (gpmpc_set_cost_buffer): 1/2 ||y_k - y_ref,k||^2_W with dt-scaled stage weights and the
        unscaled terminal weight (`gpmpc/gpmpc.py:231-239`); NaN for a failed solve."""
        self.stage_cost = (torch.full((self.batch, self.H + 1), float("nan"), dtype=torch.float64, device=self.device)
                           if enabled else None)
        _lib.check(self.lib.gpmpc_set_cost_buffer(self._h, None if self.stage_cost is None
                                                  else self.stage_cost.data_ptr()))
        return self.stage_cost

    def set_profiling(self, enabled: bool):
        _lib.check(self.lib.gpmpc_set_profiling(self._h, int(enabled)))

    def kernel_times(self) -> dict:
        """Summed HIP-event milliseconds of the variance / SQP kernels since the last call."""
        vm, sm = ctypes.c_double(), ctypes.c_double()
        vn, sn = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.gpmpc_kernel_times(self._h, ctypes.byref(vm), ctypes.byref(vn), ctypes.byref(sm),
                                               ctypes.byref(sn)))
        return {"var_ms": vm.value, "var_launches": vn.value, "sqp_ms": sm.value, "sqp_launches": sn.value}

    def kernel_time_list(self, cap: int = 4096) -> dict:
        """Per-launch HIP-event milliseconds of the variance / SQP kernels since the last call."""
        vm = (ctypes.c_double * cap)()
        sm = (ctypes.c_double * cap)()
        vn, sn = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.gpmpc_kernel_time_list(self._h, cap, vm, ctypes.byref(vn), sm, ctypes.byref(sn)))
        return {"var_ms": list(vm[:min(vn.value, cap)]), "sqp_ms": list(sm[:min(sn.value, cap)])}

    # ------------------------------------------------------------------ stepping
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def reset(self, reset_iterate: bool = False):
        _lib.check(self.lib.gpmpc_reset(self._h, self.batch, int(reset_iterate), self._stream()))

    def set_iterate(self, x: torch.Tensor, u: torch.Tensor):
        x = x.to(self.device, torch.float64).contiguous()
        u = u.to(self.device, torch.float64).contiguous()
        assert x.shape == (self.batch, self.H + 1, self.nx) and u.shape == (self.batch, self.H, self.nu)
        _lib.check(self.lib.gpmpc_set_iterate(self._h, self.batch, x.data_ptr(), u.data_ptr(), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()

    def solve(self, x0: torch.Tensor, tstep: torch.Tensor) -> torch.Tensor:
        """One batched select_action: returns u0 (B, nu); status etc. in the buffers."""
        if x0.shape != (self.batch, self.nx) or x0.dtype != torch.float64 or x0.device != self.device:
            raise ValueError(f"x0 must be a ({self.batch}, {self.nx}) float64 tensor on {self.device}")
        if tstep.shape != (self.batch,) or tstep.dtype != torch.int32 or tstep.device != self.device:
            raise ValueError(f"tstep must be a ({self.batch},) int32 tensor on {self.device}")
        x0 = x0.contiguous()
        _lib.check(self.lib.gpmpc_solve(self._h, self.batch, x0.data_ptr(), tstep.data_ptr(), self.u0.data_ptr(),
                                        self.status.data_ptr(), self.sqp_iter.data_ptr(), self.qp_iter.data_ptr(),
                                        self.res.data_ptr(), self._stream()))
        return self.u0

    def solution(self):
        x = torch.empty(self.batch, self.H + 1, self.nx, dtype=torch.float64, device=self.device)
        u = torch.empty(self.batch, self.H, self.nu, dtype=torch.float64, device=self.device)
        t = torch.empty(self.batch, self.H + 1, self.nx + self.nu, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.gpmpc_get_solution(self._h, self.batch, x.data_ptr(), u.data_ptr(), t.data_ptr(),
                                               self._stream()))
        return x, u, t

    def variance(self) -> torch.Tensor:
        """GP variances (B, H, n_gp) the last tightening used (gpmpc_get_variance): the variance
        kernel's output at the previous solution, likelihood noise included."""
        v = torch.empty(self.batch, self.H, self.spec.n_gp, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.gpmpc_get_variance(self._h, self.batch, v.data_ptr(), self._stream()))
        return v

    def plant_step(self, x: torch.Tensor, u: torch.Tensor, tstep: torch.Tensor | None = None,
                   params: dict | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """Synthetic plant: RK4 of the prior-form model with ``params`` (default: spec.true_params)."""
        p = _c(self.spec.param_vector(self.spec.true_params if params is None else params))
        out = torch.empty_like(x) if out is None else out
        _lib.check(self.lib.gpmpc_plant_step(self._h, x.shape[0], p.ctypes.data, x.data_ptr(), u.data_ptr(),
                                             out.data_ptr(), None if tstep is None else tstep.data_ptr(),
                                             self._stream()))
        return out

    def rollout(self, x0: torch.Tensor, u: torch.Tensor, with_gp: bool = True, var: bool = False):
        """Open-loop rollout of the model the MPC plans with (gpmpc_rollout): ``x0`` (P, nx) and ``u`` (P, T, nu)
        on the solver's device give ``x`` (P, T+1, nx), row 0 a copy of ``x0`` and row k+1 one RK4 step from
        ``(x_k, u_k)``: the discrete map of the SQP's shooting constraint, the GP means evaluated at every RK4
        substage as the solver reads them (a FITC mean included).  ``with_gp=False`` rolls the prior alone (the
        nominal MPC's model; no GP needs to be set).  With ``var=True`` also (P, T, n_gp): each GP's exact
        posterior variance without likelihood noise at ``z_k[gp_src_g]``, as ``gp_predict`` returns it.  P is
        independent of the solver's batch, and a trajectory's result does not depend on the others.  The inputs
        must be complete when the library reads them, so the call synchronises the current stream first; it
        returns with its work completed (it runs on a stream of the handle's own)."""
        x0 = x0.to(self.device, torch.float64).contiguous()
        u = u.to(self.device, torch.float64).contiguous()
        if x0.ndim != 2 or x0.shape[1] != self.nx:
            raise ValueError(f"x0 must be (P, nx={self.nx})")
        if u.ndim != 3 or u.shape[0] != x0.shape[0] or u.shape[2] != self.nu:
            raise ValueError(f"u must be (P={x0.shape[0]}, T, nu={self.nu})")
        P, T = int(u.shape[0]), int(u.shape[1])
        x = torch.empty(P, T + 1, self.nx, dtype=torch.float64, device=self.device)
        v = torch.empty(P, T, self.spec.n_gp, dtype=torch.float64, device=self.device) if var else None
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.gpmpc_rollout(self._h, P, T, x0.data_ptr(), u.data_ptr(), int(bool(with_gp)), x.data_ptr(),
                                          _lib.ptr(v)))
        return (x, v) if var else x

    def rollout_lin(self, x0: torch.Tensor, u: torch.Tensor, with_gp: bool = True, var: bool = False, cov: bool = False,
                    K=None, cov0: torch.Tensor | None = None, with_noise: bool = False) -> dict:
        """:meth:`rollout` with the Jacobians of every step (gpmpc_rollout_lin).  Returns a dict: ``x`` (P, T+1, nx)
        and, with ``var=True``, ``var`` (P, T, n_gp), both the bits :meth:`rollout` returns; ``A`` (P, T, nx, nx) and
        ``B`` (P, T, nx, nu), the exact derivative of the RK4 step at ``(x_k, u_k)``, GP input gradients included
        unless ``with_gp=False``.  With ``cov=True`` also ``cov`` (P, T+1, nx, nx): ``cov[:, 0]`` is ``cov0``
        (P, nx, nx; None: zero) and ``cov[:, k+1] = Phi_k cov[:, k] Phi_k^T + Bd diag(q_k) Bd^T`` with
        ``Phi_k = A_k + B_k K`` (``K`` (nu, nx), host; None: the open loop) and ``q_k`` the GP variances at
        ``(x_k, u_k)`` (plus the likelihood noise with ``with_noise=True``, once) under the tightening's weights.
        The variance and the covariance need every GP set with its Linv.  Synchronises the current stream first,
        as :meth:`rollout` does, and returns with its work completed."""
        x0 = x0.to(self.device, torch.float64).contiguous()
        u = u.to(self.device, torch.float64).contiguous()
        if x0.ndim != 2 or x0.shape[1] != self.nx:
            raise ValueError(f"x0 must be (P, nx={self.nx})")
        if u.ndim != 3 or u.shape[0] != x0.shape[0] or u.shape[2] != self.nu:
            raise ValueError(f"u must be (P={x0.shape[0]}, T, nu={self.nu})")
        P, T = int(u.shape[0]), int(u.shape[1])
        if K is not None:
            K = _c(K)
            if K.shape != (self.nu, self.nx):
                raise ValueError(f"K must be (nu={self.nu}, nx={self.nx})")
        if cov0 is not None:
            cov0 = cov0.to(self.device, torch.float64).contiguous()
            if tuple(cov0.shape) != (P, self.nx, self.nx):
                raise ValueError(f"cov0 must be (P={P}, nx={self.nx}, nx={self.nx})")

        def new(*shape):
            return torch.empty(*shape, dtype=torch.float64, device=self.device)

        out = {"x": new(P, T + 1, self.nx), "A": new(P, T, self.nx, self.nx), "B": new(P, T, self.nx, self.nu)}
        if var:
            out["var"] = new(P, T, self.spec.n_gp)
        if cov:
            out["cov"] = new(P, T + 1, self.nx, self.nx)
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.gpmpc_rollout_lin(self._h, P, T, x0.data_ptr(), u.data_ptr(), int(bool(with_gp)),
                                              out["x"].data_ptr(), out["A"].data_ptr(), out["B"].data_ptr(),
                                              _lib.ptr(out.get("var")), None if K is None else K.ctypes.data,
                                              _lib.ptr(cov0), int(bool(with_noise)), _lib.ptr(out.get("cov"))))
        return out

    def rollout_sample(self, x0: torch.Tensor, u: torch.Tensor, xref: torch.Tensor | None = None, K=None,
                       clip: bool = False, xi: torch.Tensor | None = None, with_gp: bool = True,
                       with_noise: bool = False, var: bool = False) -> dict:
        """One closed-loop sample per trajectory of the future the learned model believes in
        (gpmpc_rollout_sample): :meth:`rollout` with the input recomputed at every step,
        ``u_k = u[:, k] + K (x_k - xref[:, k])`` (``K`` (nu, nx), host, with ``xref`` (P, T+1, nx); both None: no
        feedback), clipped to the model's input box with ``clip=True``, and one draw of every GP's residual,
        ``sqrt(max(var_g + noise_g, 0)) xi[:, k, g]``, added to its mean at every RK4 substage of the step (``xi``
        (P, T, n_gp): the caller's standard-normal draws, None for no disturbance; the variance is the exact
        posterior variance at ``(x_k, u_k)`` with the applied input, plus the likelihood noise with
        ``with_noise=True``).  Returns a dict: ``x`` (P, T+1, nx), ``u`` (P, T, nu) the applied inputs and, with
        ``var=True``, ``var`` (P, T, n_gp) without likelihood noise.  With no ``xi``, no ``K`` and no clip ``x`` is
        :meth:`rollout`'s bits.  The disturbance and the variance need every GP set with its Linv.  Synchronises
        the current stream first, as :meth:`rollout` does, and returns with its work completed."""
        x0 = x0.to(self.device, torch.float64).contiguous()
        u = u.to(self.device, torch.float64).contiguous()
        if x0.ndim != 2 or x0.shape[1] != self.nx:
            raise ValueError(f"x0 must be (P, nx={self.nx})")
        if u.ndim != 3 or u.shape[0] != x0.shape[0] or u.shape[2] != self.nu:
            raise ValueError(f"u must be (P={x0.shape[0]}, T, nu={self.nu})")
        P, T = int(u.shape[0]), int(u.shape[1])
        if (K is None) != (xref is None):
            raise ValueError("K and xref go together (both given, or both None)")
        if K is not None:
            K = _c(K)
            if K.shape != (self.nu, self.nx):
                raise ValueError(f"K must be (nu={self.nu}, nx={self.nx})")
            xref = xref.to(self.device, torch.float64).contiguous()
            if tuple(xref.shape) != (P, T + 1, self.nx):
                raise ValueError(f"xref must be (P={P}, T+1={T + 1}, nx={self.nx})")
        if xi is not None:
            xi = xi.to(self.device, torch.float64).contiguous()
            if tuple(xi.shape) != (P, T, self.spec.n_gp):
                raise ValueError(f"xi must be (P={P}, T={T}, n_gp={self.spec.n_gp})")

        def new(*shape):
            return torch.empty(*shape, dtype=torch.float64, device=self.device)

        out = {"x": new(P, T + 1, self.nx), "u": new(P, T, self.nu)}
        if var:
            out["var"] = new(P, T, self.spec.n_gp)
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.gpmpc_rollout_sample(self._h, P, T, x0.data_ptr(), u.data_ptr(), _lib.ptr(xref),
                                                 None if K is None else K.ctypes.data, int(bool(clip)), _lib.ptr(xi),
                                                 int(bool(with_gp)), int(bool(with_noise)), out["x"].data_ptr(),
                                                 out["u"].data_ptr(), _lib.ptr(out.get("var"))))
        return out
