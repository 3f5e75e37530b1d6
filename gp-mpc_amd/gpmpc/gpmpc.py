"""GP-MPC controller on the MI355X (drop-in for ``gpmpc/gpmpc.py``).

:class:`GPMPC` keeps the reference's surface -- ``GPMPC(model, traj, prior_params, horizon,
q_mpc, r_mpc, sparse_gp, prob, max_gp_samples, seed, device)``, ``train_gp``, ``reset``,
``select_action(obs) -> action``, ``x_prev`` / ``u_prev``, ``prior_ctrl``,
``gaussian_process`` (`gpmpc/gpmpc.py:20-111,153-164,334-368`) -- and adds the batched
form ``select_action_batch(obs[B, nx]) -> actions[B, nu]`` on device tensors.  The
acados OCP (`gpmpc/gpmpc.py:166-320`) is replaced by the batched HIP solver
(``csrc/sqp_kernel.hip``); there is no code generation and no CPU fallback.

``model`` is a :class:`gpmpc.models.ModelSpec` or its name (``"quad3d"``, ``"quad2d"``,
``"cartpole"``); it takes the role of crazyflow's ``symbolic_attitude`` model object.
"""

from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import _lib
from .gp import LOVE_CHOLESKY_ROWS, GaussianProcess, fit_gp
from .models import ModelSpec, get_spec
from .mpc import MPC
from .solver import BatchSolver, STATUS_NAMES, inverse_cdf, predict_trajectory, setup_prior_dynamics


class GPMPC:
    """Implements a GP-MPC controller on the MI355X HIP solver."""

    # the reference's quadrotor hover input (`gpmpc/gpmpc.py:18`); an instance's U_EQ is its model's
    U_EQ: np.ndarray = np.array([0.3234, 0, 0, 0])
    # tightening variance mode: the constructor sets it ("love" unless told otherwise); a controller put
    # together without the constructor has no LOVE roots to look after (_update_gps)
    variance: str = "exact"
    # where the sparse (FITC) mean is built: "host" (precompute_sparse_posterior_mean, uploaded once; no
    # device-side update of the GPs) or "device" (BatchSolver.fitc_gp on the uploaded exact GPs, rebuilt after
    # every update); the jitter the device build adds to the diagonal of K_ss; its last draw of inducing rows.
    # fitc_select: how the device build chooses them, "random" (the reference's np_random.choice, one draw for all
    # GPs) or "greedy" (BatchSolver.inducing_gp per GP, down to a residual prior variance of fitc_tol outputscales;
    # fitc_idx is then a list of per-GP arrays)
    fitc: str = "host"
    fitc_jitter: float = 0.0
    fitc_idx: np.ndarray | list | None = None
    fitc_select: str = "random"
    fitc_tol: float = 1e-4

    def __init__(self, symbolic_model, traj: np.ndarray | None = None, prior_params: dict | None = None,
                 horizon: int = 25, q_mpc: list | None = None, r_mpc: list | None = None, sparse_gp: bool = False,
                 prob: float = 0.955, max_gp_samples: int = 30, seed: int = 1337, device: str = "cuda",
                 output_dir: Path | None = None, batch: int = 1, variance_inputs: str = "reference",
                 variance: str = "love", gp_capacity: int | None = None, fitc: str = "host",
                 fitc_jitter: float = 0.0, fitc_select: str = "random", fitc_tol: float = 1e-4, **solver_kw):
        spec = (symbolic_model if isinstance(symbolic_model, ModelSpec) else get_spec(symbolic_model)).copy()
        # "reference": the variance input map of `gpmpc/gpmpc.py:437-444` (for quad3d it indexes the
        # full state-input vector with the GP-input-space indices); "dynamics": each GP's own inputs
        if variance_inputs == "dynamics":
            spec.var_inputs = spec.gp_inputs
        elif variance_inputs != "reference":
            raise ValueError("variance_inputs must be 'reference' or 'dynamics'")
        self.model = spec
        # tightening variance.  Default "love": what the reference computes -- its
        # propagate_constraint_limits runs under gpytorch.settings.fast_pred_var() (gpmpc.py:442-444),
        # i.e. the exact Cholesky variance up to gpytorch's max_cholesky_size (800 training rows)
        # and the rank-100 Lanczos (LOVE) root above it; "exact": L^-1 k at every size.
        self.variance = variance
        if q_mpc is not None:
            spec.q_diag = np.asarray(q_mpc, dtype=np.float64)
        if r_mpc is not None:
            spec.r_diag = np.asarray(r_mpc, dtype=np.float64)
        assert len(spec.q_diag) == spec.nx and len(spec.r_diag) == spec.nu
        if prior_params is not None:
            missing = [k for k in spec.prior if k not in prior_params]
            if missing:
                raise ValueError(f"GPMPC requires prior_params with keys {sorted(spec.prior)}; missing {missing}")
            spec.prior = {k: float(prior_params[k]) for k in spec.prior}
        self.sparse = sparse_gp
        if fitc not in ("host", "device"):
            raise ValueError("fitc must be 'host' or 'device'")
        if fitc == "device" and not sparse_gp:
            raise ValueError("fitc='device' builds the sparse (FITC) mean: it needs sparse_gp=True")
        if fitc_select not in ("random", "greedy"):
            raise ValueError("fitc_select must be 'random' or 'greedy'")
        if fitc_select == "greedy" and not (sparse_gp and fitc == "device"):
            raise ValueError("fitc_select='greedy' picks the inducing rows on the device: it needs sparse_gp=True, "
                             "fitc='device'")
        self.fitc = fitc
        self.fitc_select = fitc_select
        self.fitc_tol = float(fitc_tol)
        self.fitc_jitter = float(fitc_jitter)
        self.fitc_idx = None
        self.output_dir = output_dir
        self.device = torch.device(device)
        self.dt = spec.dt
        self.T = int(horizon)
        self.Q, self.R = np.diag(spec.q_diag), np.diag(spec.r_diag)
        self.U_EQ = spec.u_eq.copy()
        self.traj = spec.reference_trajectory() if traj is None else np.asarray(traj, dtype=np.float64)
        self.ref_action = np.repeat(self.U_EQ[:, None], self.T, axis=1)
        self.traj_step = 0
        self.np_random = np.random.default_rng(seed)
        self.gp_idx = self._gp_columns(spec)
        # thrust map of the quadrotors (`gpmpc/gpmpc.py:45`); cartpole has none
        self.acc_symbolic_fn = self.setup_symbolic_acceleration(spec.prior) if "a" in spec.prior else None
        self.gaussian_process: list[GaussianProcess] | None = None
        self._requires_recompile = False
        self.prob = prob
        self.inverse_cdf = inverse_cdf(prob, spec.nx)
        self.max_gp_samples = max_gp_samples
        self.Bd = spec.bd_matrix()
        self.batch = int(batch)
        # training rows the solver handle's GPs get room for when they are uploaded (reset()), so that
        # append_data can extend them on the device; None: the uploaded size (no appending)
        self.gp_capacity = None if gp_capacity is None else int(gp_capacity)

        self.prior_ctrl = MPC(spec, traj=self.traj, horizon=self.T, q_mpc=list(spec.q_diag),
                              r_mpc=list(spec.r_diag), device=device, batch=batch, **solver_kw)
        dfdx, dfdu = spec.prior_jacobian(np.zeros(spec.nx), spec.u_eq)
        self.discrete_dfdx, self.discrete_dfdu, self.lqr_gain = setup_prior_dynamics(dfdx, dfdu, self.Q, self.R, self.dt)

        self.solver = BatchSolver(spec, self.T, self.batch, device=self.device, traj=self.traj, uh=-1e-8, **solver_kw)
        self.solver.set_tightening(True, prob, self.discrete_dfdx, self.discrete_dfdu, self.lqr_gain)
        self._x_prev = None
        self._u_prev = None
        self._has_prev = False
        self._tstep = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        # select_action's host staging: pinned buffers, so the observation / reference index go in and
        # the action / status come back as asynchronous copies with one synchronisation per call
        self._pinned = None
        if self.batch == 1 and torch.device(self.device).type == "cuda":
            self._pinned = (torch.empty(1, spec.nx, dtype=torch.float64, pin_memory=True),
                            torch.empty(1, dtype=torch.int32, pin_memory=True),
                            torch.empty(spec.nu, dtype=torch.float64, pin_memory=True),
                            torch.empty(1, dtype=torch.int32, pin_memory=True))
            self._x0_dev = torch.empty(1, spec.nx, dtype=torch.float64, device=self.device)

    @staticmethod
    def _gp_columns(spec: ModelSpec) -> list[list[int]]:
        """Column groups of the concatenated GP training inputs (`gpmpc/gpmpc.py:59`)."""
        cols, c = [], 0
        for d in spec.gp_dims:
            cols.append(list(range(c, c + d)))
            c += d
        return cols

    # ------------------------------------------------------------------ training data
    def setup_symbolic_acceleration(self, params: dict):
        """Prior thrust map T_c -> a T_c + b (`gpmpc/gpmpc.py:322-325`), a numpy callable."""
        a, b = float(params["a"]), float(params["b"])
        return lambda thrust_cmd: a * np.asarray(thrust_cmd, dtype=np.float64) + b

    def prior_dynamics(self, x: np.ndarray, u: np.ndarray) -> np.ndarray:
        """Continuous prior f(x, u) for rows of x (n, nx), u (n, nu) (crazyflow ``fc_func``)."""
        return self.model.prior_f(x, u)

    def preprocess_data(self, x: np.ndarray, u: np.ndarray, x_next: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """GP training inputs (N, sum d_g) and targets (N, n_gp) from transitions
        (`gpmpc/gpmpc.py:113-151`): numerically differentiated next state minus the prior.

        quad3d follows the reference literally, including its constants (g = 9.81 and
        dt = 1/60, not the model's dt) and the thrust target as the norm of the acceleration
        minus the prior thrust map.  quad2d / cartpole apply the same recipe to their GP
        outputs (thrust-acceleration norm and pitch rate; cart and pole accelerations).
        """
        x, u, x_next = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (x, u, x_next))
        spec = self.model
        if spec.name == "quad3d":
            g, dt = 9.81, 1 / 60
            x_dot = (x_next - x) / dt
            acc = np.sqrt(x_dot[:, 1] ** 2 + x_dot[:, 3] ** 2 + (x_dot[:, 5] + g) ** 2)
            acc_target = acc - self.acc_symbolic_fn(u[:, 0])
            f = self.prior_dynamics(x, u)
            phi_target = x_dot[:, 6] - f[:, 6]
            theta_target = x_dot[:, 7] - f[:, 7]
            inputs = np.column_stack([u[:, 0], x[:, 6], x[:, 9], u[:, 1], x[:, 7], x[:, 10], u[:, 2]])
            return inputs, np.column_stack([acc_target, phi_target, theta_target])
        dt = spec.dt
        x_dot = (x_next - x) / dt
        f = self.prior_dynamics(x, u)
        z = np.hstack([x, u])
        inputs = np.hstack([z[:, list(idx)] for idx in spec.gp_inputs])
        if spec.name == "quad2d":
            acc = np.sqrt(x_dot[:, 1] ** 2 + (x_dot[:, 3] + spec.gravity) ** 2)
            targets = np.column_stack([acc - self.acc_symbolic_fn(u[:, 0]), x_dot[:, 5] - f[:, 5]])
        else:  # cartpole: residual cart / pole accelerations
            targets = np.column_stack([x_dot[:, 1] - f[:, 1], x_dot[:, 3] - f[:, 3]])
        return inputs, targets

    # ------------------------------------------------------------------ GP management
    def train_gp(self, x: np.ndarray, y: np.ndarray, lr: float, iterations: int):
        """Fit one GP per output column on its input columns (`gpmpc/gpmpc.py:153-164`), on the
        controller's device (the MI355X); one all-reduce of the MLL gradient per Adam step
        when running data-parallel (gpmpc/distributed.py)."""
        x_train = torch.tensor(np.asarray(x, dtype=np.float64), device=self.device)
        y_train = torch.tensor(np.asarray(y, dtype=np.float64), device=self.device)
        gps = []
        from . import distributed as D

        _, size = D.world()
        if size > 1:   # the row-split gradient of fit_gp_allreduce is only valid on identical replicas
            D.assert_replicated(x, y)
        for i, idx in enumerate(self.gp_idx):
            gp = GaussianProcess(x_train[:, idx], y_train[:, i])
            if size > 1:   # data-parallel fit: one all-reduce of the MLL gradient per Adam step
                D.fit_gp_allreduce(gp, n_train=iterations, lr=lr)
            else:
                fit_gp(gp, n_train=iterations, lr=lr, device=self.device)
            gps.append(gp)
        self.set_gaussian_processes(gps)

    def set_gaussian_processes(self, gps: list[GaussianProcess]):
        for gp in gps:
            if gp.K is None:
                gp.K, gp.K_inv = gp.compute_covariances()
        self.gaussian_process = gps
        self._requires_recompile = True

    def _update_gps(self, update):
        """Run a device-side update of the handle's GPs (``update()``, whose result is returned) under
        the controller's variance mode.  The updates refuse a GP with a LOVE root installed, which
        belongs to the old training set or factor, so with ``variance="love"`` the roots are dropped
        first and afterwards every GP with more than ``LOVE_CHOLESKY_ROWS`` rows gets a root built on
        the device (``BatchSolver.love_root_gp``, which synchronises the stream); the others keep the
        exact variance, as ``set_gps`` chooses for their size.  If the update raises, the GPs are left
        on the exact variance.

        With ``sparse_gp=True, fitc="device"`` the FITC means are handled the same way: dropped before the
        update, which works on the exact GPs underneath, and built again afterwards from a fresh draw of
        inducing rows over the current training rows (``_build_fitc``)."""
        s = self.solver
        love = self.variance == "love"
        fitc = self.sparse and self.fitc == "device"
        if fitc:
            for g in range(self.model.n_gp):
                if s.fitc_sizes[g]:
                    s.drop_fitc(g)
        if love:
            for g in range(self.model.n_gp):
                if s.love_ranks[g] is not None:
                    s.drop_love_root(g)
        out = update()
        if love:
            for g in range(self.model.n_gp):
                if s.gp_size(g)[0] > LOVE_CHOLESKY_ROWS:
                    _, ok = s.love_root_gp(g, rank=s.love_rank)
                    if not ok:
                        raise _lib.GPMPCError(f"GP {g}: the LOVE root could not be built (a pivot was not positive); "
                                              "the GP is on the exact variance")
        if fitc:
            self._build_fitc()
        return out

    def _build_fitc(self):
        """The FITC mean of every GP on the solver handle, built on the device (``BatchSolver.fitc_gp``) on one
        draw of ``min(n, max_gp_samples)`` inducing rows over the handle's n current training rows: the
        ``np_random.choice`` call of ``precompute_sparse_posterior_mean``, so the same seed gives the same
        rows.  The draw is kept as ``fitc_idx``.

        With ``fitc_select="greedy"`` the rows are chosen on the device instead, per GP
        (``BatchSolver.inducing_gp`` with at most ``min(n, max_gp_samples)`` rows and ``fitc_tol``): ``fitc_idx``
        is then a list of per-GP int32 arrays, the GPs may end with different numbers of inducing rows
        (``solver.fitc_sizes``), and ``np_random`` is not consumed."""
        s = self.solver
        n = s.gp_size(0)[0]
        greedy = self.fitc_select == "greedy"
        if greedy:
            self.fitc_idx = [s.inducing_gp(g, min(s.gp_size(g)[0], self.max_gp_samples), self.fitc_tol).cpu().numpy()
                             for g in range(self.model.n_gp)]
        else:
            self.fitc_idx = np.asarray(self.np_random.choice(range(n), size=min(n, self.max_gp_samples), replace=False))
        for g, gp in enumerate(self.gaussian_process):
            if not s.fitc_gp(g, self.fitc_idx[g] if greedy else self.fitc_idx, gp.train_targets, self.fitc_jitter):
                hint = "; try fitc_jitter > 0" if self.fitc_jitter == 0.0 else ""
                raise _lib.GPMPCError(f"GP {g}: the FITC mean could not be built (a pivot or a Gamma was not positive, "
                                      f"or an inducing row is inert); the GP is on the exact mean{hint}")

    def drop_oldest(self, m: int) -> list[torch.Tensor]:
        """Remove the ``m`` oldest training rows of every GP on the solver handle, on the device
        (``BatchSolver.drop_gp``, queued on the current stream, no refactorisation), and of the Python
        GP objects with them (``GaussianProcess.drop_oldest``).  At least one row stays.  Returns the
        status flags per GP (device tensors; a 0 means that GP must be uploaded again).  In sparse
        (FITC) mode only with ``fitc="device"``, like ``append_data``; LOVE roots and FITC means as there."""
        if self.sparse and self.fitc != "device":
            raise _lib.GPMPCError("drop_oldest: not available in sparse (FITC) mode")
        assert self.gaussian_process is not None and not self._requires_recompile, \
            "GP model must be uploaded (call reset())"
        m = int(m)
        n = self.solver.gp_size(0)[0]
        if not 1 <= m < n:   # before any GP changes, so the handle's GPs stay in step
            raise ValueError(f"drop_oldest: m must be 1..{n - 1} (at least one row stays), got {m}")
        return self._update_gps(lambda: self._drop_oldest(m))

    def _drop_oldest(self, m: int) -> list[torch.Tensor]:
        flags = []
        for i in range(len(self.gp_idx)):
            flags.append(self.solver.drop_gp(i, m))
            self.gaussian_process[i].drop_oldest(m)
        return flags

    def drop_rows(self, idx) -> list[torch.Tensor]:
        """Remove the training rows ``idx`` names (distinct int32 indices into the current rows; a device or host
        tensor or an array) of every GP on the solver handle, on the device (``BatchSolver.drop_rows``, queued on
        the current stream, no refactorisation), and of the Python GP objects with them
        (``GaussianProcess.drop_rows``, from the rows the handle reports as dropped, so no index is read on the
        host): the mirror of ``drop_oldest`` for an arbitrary set, such as an outlier or the picks of
        ``BatchSolver.redundant``.  At least one row stays.  Returns the status flags per GP (device tensors [1]; a
        0 means the indices were not distinct values in range, or that GP must be uploaded again).  Sparse mode,
        LOVE roots and FITC means as for ``drop_oldest``."""
        if self.sparse and self.fitc != "device":
            raise _lib.GPMPCError("drop_rows: not available in sparse (FITC) mode")
        assert self.gaussian_process is not None and not self._requires_recompile, \
            "GP model must be uploaded (call reset())"
        idx = torch.as_tensor(idx).to(self.device, torch.int32).reshape(-1)
        m, n = int(idx.shape[0]), self.solver.gp_size(0)[0]
        if not 1 <= m < n:   # before any GP changes, so the handle's GPs stay in step
            raise ValueError(f"drop_rows: the number of rows must be 1..{n - 1} (at least one row stays), got {m}")
        return self._update_gps(lambda: self._drop_rows(idx))

    def _drop_rows(self, idx: torch.Tensor) -> list[torch.Tensor]:
        flags = []
        for i in range(len(self.gp_idx)):
            dropped, ok = self.solver.drop_rows(i, idx)
            self.gaussian_process[i].drop_rows(dropped)
            flags.append(ok)
        return flags

    def append_data(self, inputs: np.ndarray, targets: np.ndarray, evict_oldest: bool = False) -> list[torch.Tensor]:
        """Fold new observations into the uploaded GPs between two control steps, hyperparameters
        unchanged: ``inputs`` (m, sum d_g) and ``targets`` (m, n_gp) in GP-input space, as
        ``preprocess_data`` returns them.  Every GP on the solver handle is extended on the device
        (``BatchSolver.append_gp``, queued on the current stream) and the Python GP objects with it
        (``GaussianProcess.append_data``), so a later ``train_gp`` refit or upload sees all data.
        Returns the accepted flags per GP (device tensors).  Needs room (``gp_capacity``).  In
        sparse (FITC) mode the inducing weights belong to the old training set: with ``fitc="host"`` the call
        is not available; with ``fitc="device"`` the FITC means are dropped before the update and built again
        on the device afterwards, on a fresh draw of inducing rows (``_update_gps``, ``fitc_idx``).
        With ``variance="love"`` the LOVE roots follow the data: they are dropped before the update and
        built again on the device afterwards for every GP above ``LOVE_CHOLESKY_ROWS`` rows
        (``_update_gps``; that build synchronises the stream).

        ``evict_oldest=True`` makes the training set a sliding window: when the new rows would
        exceed the capacity, exactly the excess is dropped from the old end first
        (``drop_oldest``).  Appending more rows than the capacity holds stays an error."""
        if self.sparse and self.fitc != "device":
            raise _lib.GPMPCError("append_data: not available in sparse (FITC) mode")
        assert self.gaussian_process is not None and not self._requires_recompile, \
            "GP model must be uploaded (call reset())"
        inputs = np.atleast_2d(np.asarray(inputs, dtype=np.float64))
        targets = np.atleast_2d(np.asarray(targets, dtype=np.float64))
        if inputs.shape[1] != sum(self.model.gp_dims) or targets.shape != (inputs.shape[0], self.model.n_gp):
            raise ValueError(f"expected inputs (m, {sum(self.model.gp_dims)}) and targets (m, {self.model.n_gp})")
        n, cap = self.solver.gp_size(0)
        excess = n + inputs.shape[0] - cap
        # before any GP changes, so the handle's GPs stay in step (an eviction leaves at least one old row)
        if excess > 0 and (not evict_oldest or excess >= n):
            raise _lib.GPMPCError(f"append_data: capacity exceeded ({n} + {inputs.shape[0]} rows, capacity {cap}; "
                                  "construct GPMPC with gp_capacity)")

        def update():
            if excess > 0:
                self._drop_oldest(excess)
            flags = []
            for i, idx in enumerate(self.gp_idx):
                X = torch.tensor(inputs[:, idx], device=self.device)
                y = torch.tensor(targets[:, i], device=self.device)
                flags.append(self.solver.append_gp(i, X, y))
                self.gaussian_process[i].append_data(X, y)
            return flags

        return self._update_gps(update)

    def observe(self, x, u, x_next, pick=None, m: int | None = None, select: str | None = None,
                evict_oldest: bool = False, evict: str | None = None):
        """``preprocess_data`` followed by ``append_data`` without leaving the device: transitions x (P, nx),
        u (P, nu), x_next (P, nx) (device tensors as ``select_action_batch`` and ``plant_step`` produce them, or
        host arrays) become GP training rows on the device and are appended to every GP of the solver handle
        in one call (``BatchSolver.observe``, queued on the current stream).  The Python GP objects are extended
        from the returned device tensors (``GaussianProcess.append_data`` / ``drop_oldest``), so they stay in
        step without a host copy.

        ``select=None``: the rows are the transitions ``pick`` names (int32 indices), or the first ``m`` (default
        all).  ``select="variance"``: the ``m`` transitions where the GPs are least certain
        (``BatchSolver.informative``; at most ``batch`` transitions).  ``select="greedy"``: ``m`` <= 256 transitions
        chosen one after the other, each the least certain once the ones before it count as observed
        (``BatchSolver.select``), so a step's near-duplicates are not all taken.  ``evict_oldest``, the capacity check, the
        LOVE roots, the device-built FITC means and the refusals in sparse mode are ``append_data``'s.  Returns
        ``(inputs, targets, accepted, dropped_ok)`` as ``BatchSolver.observe`` does.

        ``evict="redundant"`` (instead of ``evict_oldest``; passing both is an error) chooses what leaves a full
        window: when the new rows would exceed the capacity, the excess (at most 256 rows) is the rows the GPs would
        miss least (``BatchSolver.redundant``), removed from every GP of the handle and from the Python GP objects
        (``drop_rows``) before the append, which then evicts nothing.  The eviction is decided before the new rows
        are seen.  ``dropped_ok`` then holds the (n_gp, 1) flags of ``BatchSolver.drop_rows``."""
        if self.sparse and self.fitc != "device":
            raise _lib.GPMPCError("observe: not available in sparse (FITC) mode")
        assert self.gaussian_process is not None and not self._requires_recompile, \
            "GP model must be uploaded (call reset())"
        if select not in (None, "variance", "greedy"):
            raise ValueError("select must be None, 'variance' or 'greedy'")
        if evict not in (None, "redundant"):
            raise ValueError("evict must be None or 'redundant'")
        if evict is not None and evict_oldest:
            raise ValueError("evict_oldest and evict both say what leaves a full window: pass one of them")
        s = self.solver
        x, u, x_next = s._transitions(x, u, x_next)
        if select is not None:
            if pick is not None or m is None:
                raise ValueError(f"select='{select}' chooses the rows itself: pass m, not pick")
            rows = int(m)
        else:
            pick, rows = s._picks(pick, m, x.shape[0])
        n, cap = s.gp_size(0)
        excess = n + rows - cap
        # before any GP changes, so the handle's GPs stay in step (an eviction leaves at least one old row)
        if excess > 0 and (not (evict_oldest or evict) or excess >= n):
            raise _lib.GPMPCError(f"observe: capacity exceeded ({n} + {rows} rows, capacity {cap}; "
                                  "construct GPMPC with gp_capacity)")
        if excess > 256 and evict == "redundant":
            raise ValueError(f"evict='redundant' chooses at most 256 rows per call, {excess} would have to leave")

        def update():
            p = s.informative(x, u, rows) if select == "variance" else s.select(x, u, rows)[0] if select == "greedy" else pick
            flags = None
            if excess > 0 and evict == "redundant":   # (decided on the GPs as they are: before the new rows are seen)
                flags = torch.stack(self._drop_rows(s.redundant(excess)))
            out = s.observe(x, u, x_next, pick=p, m=rows, evict_oldest=evict_oldest)
            inputs, targets = out[0], out[1]
            for i, idx in enumerate(self.gp_idx):
                if excess > 0 and flags is None:
                    self.gaussian_process[i].drop_oldest(excess)
                self.gaussian_process[i].append_data(inputs[:, idx], targets[:, i])
            return out if flags is None else (out[0], out[1], out[2], flags)

        return self._update_gps(update)

    def refresh_gps(self, hyperparameters: list | None = None) -> list[torch.Tensor]:
        """Factorise every GP on the solver handle again from scratch, on the device
        (``BatchSolver.refactor_gp``, queued on the current stream, no upload): from the handle's own
        inputs and the Python GP's ``train_targets``.  ``hyperparameters[g] = (lengthscale,
        outputscale, noise)`` applies new hyperparameters to GP g, on the handle and on the Python
        object (``GaussianProcess.set_hyperparameters``); by default every GP keeps its own, and the
        call only sheds the rounding that appends and drops have accumulated.  Returns the status
        flags per GP (device tensors; a 0 means that GP must be uploaded again).  Same preconditions
        as ``append_data``, LOVE roots and device-built FITC means rebuilt as there; in sparse (FITC) mode only with
        ``fitc="device"``."""
        if self.sparse and self.fitc != "device":
            raise _lib.GPMPCError("refresh_gps: not available in sparse (FITC) mode")
        assert self.gaussian_process is not None and not self._requires_recompile, \
            "GP model must be uploaded (call reset())"
        if hyperparameters is not None and len(hyperparameters) != len(self.gp_idx):
            raise ValueError(f"expected {len(self.gp_idx)} (lengthscale, outputscale, noise) triples")
        return self._update_gps(lambda: self._refresh_gps(hyperparameters))

    def _refresh_gps(self, hyperparameters: list | None) -> list[torch.Tensor]:
        flags = []
        for i, gp in enumerate(self.gaussian_process):
            hyp = (gp.lengthscale, gp.outputscale, gp.noise) if hyperparameters is None else \
                tuple(float(v) for v in hyperparameters[i])
            flags.append(self.solver.refactor_gp(i, gp.train_targets, *hyp))
            if hyperparameters is not None:
                gp.set_hyperparameters(*hyp)
        return flags

    def refit_hyperparameters(self, lr: float, iterations: int, fit: str = "torch") -> list[torch.Tensor]:
        """Refit the hyperparameters of the uploaded GPs on their current data and apply them on the
        device: no upload, and the controller needs no ``reset()``.

        ``fit="torch"``: ``fit_gp`` (``fit_gp_allreduce`` under more than one rank, as ``train_gp``
        chooses) on the Python GP's copy of the data, then ``refresh_gps``, whose flags are returned.
        ``fit="device"``: ``BatchSolver.fit_gp`` per GP, from the Python GP's current raw parameters
        on the handle's own factor, inputs and scratch; the fitted raw parameters are written into the
        Python GP objects (a GP whose fit failed keeps its own) and one int32 device flag per GP is
        returned, like ``refresh_gps``'.  Single rank only: the data-parallel fit stays the torch one.
        Either way LOVE roots (and, with ``fitc="device"``, FITC means) are dropped first and rebuilt on the
        device afterwards (``_update_gps``); in sparse (FITC) mode only with ``fitc="device"``."""
        if self.sparse and self.fitc != "device":
            raise _lib.GPMPCError("refit_hyperparameters: not available in sparse (FITC) mode")
        if fit not in ("torch", "device"):
            raise ValueError("fit must be 'torch' or 'device'")
        assert self.gaussian_process is not None and not self._requires_recompile, \
            "GP model must be uploaded (call reset())"
        from . import distributed as D

        _, size = D.world()
        if fit == "device":
            if size > 1:
                raise _lib.GPMPCError("refit_hyperparameters: fit='device' runs on one rank (the data-parallel fit is "
                                      "fit='torch')")

            def fit_all():
                flags = []
                for i, gp in enumerate(self.gaussian_process):
                    raw0 = [float(p) for p in gp.parameters()]
                    raw, _, ok = self.solver.fit_gp(i, gp.train_targets, raw0, lr, iterations)
                    if ok:
                        for p, r in zip(gp.parameters(), raw):
                            p.fill_(float(r))
                        gp.K, gp.K_inv, gp._dev = None, None, None
                    flags.append(torch.tensor([ok], dtype=torch.int32, device=self.device))
                return flags

            return self._update_gps(fit_all)
        for gp in self.gaussian_process:
            if size > 1:
                D.fit_gp_allreduce(gp, n_train=iterations, lr=lr)
            else:
                fit_gp(gp, n_train=iterations, lr=lr, device=self.device)
        return self.refresh_gps()

    def precompute_sparse_posterior_mean(self, n_samples: int):
        """FITC weights on random training rows (`gpmpc/gpmpc.py:377-400`), computed where the
        GP lives (the MI355X for a GP fitted by ``train_gp``)."""
        gps = self.gaussian_process
        n = gps[0].train_inputs[0].shape[0]
        rand_idx = self.np_random.choice(range(n), size=n_samples, replace=False)
        out = []
        for gp in gps:
            X = gp.train_inputs[0]
            y = gp.train_targets
            S = X[torch.as_tensor(rand_idx, device=X.device)]
            with torch.no_grad():
                K = gp.K.to(X.device)
                K_ss = gp.kernel(S)
                K_xs = gp.kernel(X, S)
                Gamma = torch.diagonal(K) - (K_xs * torch.linalg.solve(K_ss, K_xs.T).T).sum(1)
                KG = K_xs.T / Gamma            # K_sx Lambda^-1 without the dense diagonal matrix
                Sigma_inv = K_ss + KG @ K_xs
                w = torch.linalg.solve(Sigma_inv, KG @ y)
            # the solver evaluates sf2 * sum_j w_j exp(.): the reference's covSE already carries sf2
            out.append((S.cpu().numpy(), w.cpu().numpy()))
        return out

    # ------------------------------------------------------------------ control
    def reset(self):
        """Reset before running (`gpmpc/gpmpc.py:94-111`): upload new GPs, forget x_prev/u_prev."""
        self.traj_step = 0
        self._tstep.zero_()
        if self._requires_recompile:
            assert self.gaussian_process is not None, "GP must be trained before reinitializing"
            fitc = None
            device_fitc = self.sparse and self.fitc == "device"
            if self.sparse and not device_fitc:
                n = self.gaussian_process[0].train_targets.shape[0]
                fitc = self.precompute_sparse_posterior_mean(min(n, self.max_gp_samples))
            self.solver.set_gps(self.gaussian_process, with_variance=True, fitc=fitc, variance=self.variance)
            if (self.gp_capacity is not None and not self.sparse) or device_fitc:
                for g in range(self.model.n_gp):   # (a training set already past the capacity stays as uploaded)
                    self.solver.reserve_gp(g, max(self.gp_capacity or 0, self.solver.gp_size(g)[0]))
            if device_fitc:   # the exact GPs are uploaded: their FITC means are built where they live
                self._build_fitc()
            self._requires_recompile = False
            # new GPs: the reference builds a fresh AcadosOcpSolver (`gpmpc/gpmpc.py:97-108`), whose
            # memory -- iterate and multipliers -- starts from zero
            self.solver.reset(reset_iterate=True)
        else:
            # same GPs: acados keeps its memory across episodes (`gpmpc/gpmpc.py:94-111` does not
            # reset the solver), so the first solve is warm-started from the last iterate
            self.solver.reset(reset_iterate=False)
        self._x_prev = None
        self._u_prev = None
        self._has_prev = False

    @property
    def x_prev(self):
        if not self._has_prev:
            return None
        if self._x_prev is None:
            x, u, _ = self.solver.solution()
            self._x_prev = x[0].T.cpu().numpy() if self.batch == 1 else x.cpu().numpy()
            self._u_prev = u[0].T.cpu().numpy() if self.batch == 1 else u.cpu().numpy()
        return self._x_prev

    @property
    def u_prev(self):
        if not self._has_prev:
            return None
        _ = self.x_prev
        return self._u_prev

    def select_action(self, obs: np.ndarray) -> np.ndarray:
        """Solve the nonlinear MPC problem to get the next action (`gpmpc/gpmpc.py:334-368`)."""
        assert not self._requires_recompile, "GP model must be uploaded (call reset())"
        assert self.gaussian_process is not None, "Gaussian processes are not initialized"
        assert self.batch == 1, "select_action is the single-instance form; use select_action_batch"
        if self._pinned is None:
            x0 = torch.as_tensor(np.asarray(obs, dtype=np.float64).reshape(1, -1), device=self.device)
            self._tstep.fill_(self.traj_step)
            self.traj_step += 1
            u0 = self.solver.solve(x0, self._tstep)
            status = int(self.solver.status[0].item())
            u = u0[0].cpu().numpy()
        else:
            x_h, t_h, u_h, s_h = self._pinned
            x_h.numpy()[0] = np.asarray(obs, dtype=np.float64).reshape(-1)
            t_h[0] = self.traj_step
            self.traj_step += 1
            self._x0_dev.copy_(x_h, non_blocking=True)
            self._tstep.copy_(t_h, non_blocking=True)
            u0 = self.solver.solve(self._x0_dev, self._tstep)
            u_h.copy_(u0[0], non_blocking=True)
            s_h.copy_(self.solver.status[:1], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            status = int(s_h[0])
            u = u_h.numpy().copy()
        assert status in [0, 2], f"solver returned unexpected status {status} ({STATUS_NAMES.get(status)})."
        self._has_prev = True
        self._x_prev = self._u_prev = None
        return u

    def select_action_batch(self, obs: torch.Tensor, tstep: torch.Tensor | None = None, check: bool = False):
        """Batched select_action on device tensors: obs (B, nx) float64 -> actions (B, nu).

        ``tstep`` (B,) int32 gives each instance's reference index (default: the shared
        ``traj_step`` counter).  ``check=True`` synchronises and asserts status in {0, 2}.
        """
        assert not self._requires_recompile, "GP model must be uploaded (call reset())"
        if tstep is None:
            self._tstep.fill_(self.traj_step)
            tstep = self._tstep
            self.traj_step += 1
        u0 = self.solver.solve(obs, tstep)
        self._has_prev = True
        self._x_prev = self._u_prev = None
        if check:
            bad = ~((self.solver.status == 0) | (self.solver.status == 2))
            if bool(bad.any()):
                i = int(torch.nonzero(bad)[0])
                raise AssertionError(f"instance {i}: unexpected status {int(self.solver.status[i])}")
        return u0

    def predict_trajectory(self, x0, u, with_gp: bool = True, return_var: bool = False, return_cov: bool = False,
                           feedback=None, with_noise: bool = False):
        """What the controller believes will happen: the open-loop rollout of its model from ``x0`` under the
        inputs ``u`` (``BatchSolver.rollout``), the learned GP means included unless ``with_gp=False`` (the prior
        alone).  numpy in and out: one trajectory, ``x0`` (nx,) and ``u`` (T, nu), gives (T+1, nx); a batch,
        (P, nx) and (P, T, nu), gives (P, T+1, nx).  ``return_var=True`` adds the GPs' posterior variances along
        it, (T, n_gp) or (P, T, n_gp).  ``return_cov=True`` adds, last, the state covariance the model itself
        states along the prediction (``BatchSolver.rollout_lin``), (T+1, nx, nx) or (P, T+1, nx, nx), from zero at
        ``x0``: ``feedback=None`` propagates through the open loop's ``A_k``, ``feedback="lqr"`` through
        ``A_k + B_k K`` with the controller's ``lqr_gain`` (the tightening's assumption), an array is taken as
        ``K`` (nu, nx); ``with_noise=True`` adds the GPs' likelihood noise to their variances, once.  The GPs must
        be uploaded (``reset()`` after ``train_gp``)."""
        assert not (with_gp and getattr(self, "_requires_recompile", False)), "GP model must be uploaded (call reset())"
        if not return_cov:
            return predict_trajectory(self.solver, x0, u, with_gp=with_gp, return_var=return_var)
        K = self.lqr_gain if isinstance(feedback, str) and feedback == "lqr" else feedback
        if isinstance(K, str):
            raise ValueError('feedback is None, "lqr" or a gain (nu, nx)')
        return predict_trajectory(self.solver, x0, u, with_gp=with_gp, return_var=return_var, return_cov=True,
                                  feedback=K, with_noise=with_noise)

    def sample_trajectories(self, x0, u, n_samples: int, seed: int = 0, feedback=None, clip: bool = True,
                            with_noise: bool = True, with_gp: bool = True):
        """Futures drawn from what the GPs believe (``BatchSolver.rollout_sample``): every input trajectory is
        repeated ``n_samples`` times and each copy rolled out with its own draws of the GPs' residuals, one per GP
        and step, at the posterior variance of the point it has reached (plus the likelihood noise with
        ``with_noise``).  numpy in and out: one trajectory, ``x0`` (nx,) and ``u`` (T, nu), gives ``x``
        (n_samples, T+1, nx) and the applied inputs (n_samples, T, nu); a batch, (P, nx) and (P, T, nu), gives
        (P, n_samples, T+1, nx) and (P, n_samples, T, nu).  ``feedback`` is None (the inputs are applied as given),
        ``"lqr"`` (the controller's ``lqr_gain``) or a gain (nu, nx): the applied input is then
        ``u_k + K (x_k - xbar_k)`` around the mean prediction ``xbar = predict_trajectory(x0, u)``, clipped to the
        input box with ``clip``.  The draws are ``torch.randn`` on the device from a generator seeded with ``seed``:
        equal seeds give equal samples.  The GPs must be uploaded (``reset()`` after ``train_gp``)."""
        assert not getattr(self, "_requires_recompile", False), "GP model must be uploaded (call reset())"
        K = self.lqr_gain if isinstance(feedback, str) and feedback == "lqr" else feedback
        if isinstance(K, str):
            raise ValueError('feedback is None, "lqr" or a gain (nu, nx)')
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("n_samples must be at least 1")
        x0 = np.asarray(x0, dtype=np.float64)
        u = np.asarray(u, dtype=np.float64)
        single = x0.ndim == 1
        if single:
            if u.ndim != 2:
                raise ValueError("one trajectory takes x0 (nx,) and u (T, nu)")
            x0, u = x0[None], u[None]
        elif x0.ndim != 2 or u.ndim != 3 or u.shape[0] != x0.shape[0]:
            raise ValueError("a batch takes x0 (P, nx) and u (P, T, nu)")
        solver = self.solver
        dev = solver.device
        P, T = u.shape[:2]
        x0t = torch.as_tensor(np.ascontiguousarray(x0), device=dev).repeat_interleave(n_samples, dim=0)
        ut = torch.as_tensor(np.ascontiguousarray(u), device=dev).repeat_interleave(n_samples, dim=0)
        xref = None
        if K is not None:
            xbar = predict_trajectory(solver, x0, u, with_gp=with_gp)
            xref = torch.as_tensor(np.ascontiguousarray(xbar), device=dev).repeat_interleave(n_samples, dim=0)
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        xi = torch.randn(P * n_samples, T, self.model.n_gp, dtype=torch.float64, device=dev, generator=gen)
        out = solver.rollout_sample(x0t, ut, xref=xref, K=K, clip=clip, xi=xi, with_gp=with_gp, with_noise=with_noise)
        x = out["x"].cpu().numpy().reshape(P, n_samples, T + 1, -1)
        ua = out["u"].cpu().numpy().reshape(P, n_samples, T, -1)
        return (x[0], ua[0]) if single else (x, ua)

    def reference_trajectory(self) -> np.ndarray:
        """`gpmpc/gpmpc.py:509-514`."""
        indices = np.arange(self.traj_step, self.traj_step + self.T + 1) % self.traj.shape[-1]
        return self.traj[:, indices]

    @staticmethod
    def setup_constraints(sym, low, high):
        """Rows A sym - b of the box constraints (`gpmpc/gpmpc.py:327-332`)."""
        dim = low.shape[0]
        A = np.vstack((-np.eye(dim), np.eye(dim)))
        b = np.hstack((-low, high))
        return A @ sym - b

    setup_prior_dynamics = staticmethod(setup_prior_dynamics)
