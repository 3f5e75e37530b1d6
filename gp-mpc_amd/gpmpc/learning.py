"""Episodic GP-MPC learning loop on the MI355X (`scripts/run_gp_mpc.py:42-137`).

The reference runs one crazyflow environment on the CPU, collects transitions with the prior
MPC, fits the GPs, and re-runs with GP-MPC each epoch.  Here an "environment" is the batched
synthetic plant kernel (``BatchSolver.plant_step``: RK4 of the model with its true
parameters), so B episodes run at once on the GPU; transitions are gathered from all of them.

* :func:`run_evaluation` -- one closed-loop episode per instance (`run_gp_mpc.py:42-72`)
* :func:`run_online_episode` -- the same episode, learning while it runs: a few of every step's
  transitions are appended to the uploaded GPs on the device (``GPMPC.append_data``, or with
  ``device_data=True`` ``GPMPC.observe``, which preprocesses them on the device too); no
  counterpart in the reference, whose loop is episodic
* :func:`sample_data`    -- random transitions of an episode batch (`run_gp_mpc.py:75-83`)
* :func:`learn`          -- prior run, then per epoch: sample, ``preprocess_data``,
  ``train_gp`` (on the GPU; data-parallel under torch.distributed), ``reset``, test and
  train episodes (`run_gp_mpc.py:86-137`).  Under N ranks every rank runs its own contiguous
  shard of the instances and the newly sampled transitions are all-gathered each epoch, so
  every rank fits the same GPs on the same data.
* :func:`get_runtime` / :func:`save_runtime_csv` -- the runtime summary and CSV of
  `gpmpc/plotting.py:10-62`.
"""

from __future__ import annotations

import time
from pathlib import Path

import numpy as np
import torch

from .synthetic import initial_states


def run_evaluation(ctrl, x0: np.ndarray, steps: int, tstep0: np.ndarray | None = None, plant_solver=None) -> dict:
    """Closed-loop episodes of ``steps`` control steps for B instances at once.

    ``ctrl`` is a :class:`~gpmpc.gpmpc.GPMPC` or :class:`~gpmpc.mpc.MPC` with ``batch = B``;
    the plant is the synthetic true-parameter model of the same spec.  Returns numpy arrays
    ``obs`` (steps+1, B, nx), ``action`` (steps, B, nu), ``status`` (steps, B),
    ``inference_time_data`` (steps,) seconds per batched select_action (synchronised).
    """
    ctrl.reset()
    solver = plant_solver if plant_solver is not None else ctrl.solver
    dev = solver.device
    B = solver.batch
    obs = torch.tensor(np.asarray(x0, dtype=np.float64).reshape(B, -1), device=dev)
    ts = torch.tensor(np.zeros(B) if tstep0 is None else tstep0, dtype=torch.int32, device=dev)
    data = {"obs": [obs.cpu().numpy()], "action": [], "status": [], "inference_time_data": []}
    for _ in range(steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        u = ctrl.select_action_batch(obs, ts.clone())
        torch.cuda.synchronize(dev)
        data["inference_time_data"].append(time.perf_counter() - t0)
        data["action"].append(u.cpu().numpy())
        data["status"].append(ctrl.solver.status.cpu().numpy())
        obs = solver.plant_step(obs, u, ts)   # advances the reference index too
        data["obs"].append(obs.cpu().numpy())
    return {k: np.array(v) for k, v in data.items()}


def run_online_episode(ctrl, x0: np.ndarray, steps: int, append_per_step: int, seed: int,
                       tstep0: np.ndarray | None = None, sliding: bool = False, refresh_every: int = 0,
                       device_data: bool = False, select: str = "random", evict: str | None = None) -> dict:
    """A closed-loop episode that learns while it runs: after every plant step a seeded random
    choice of ``append_per_step`` of the step's B transitions is preprocessed
    (``GPMPC.preprocess_data``) and appended to the uploaded GPs (``GPMPC.append_data``, a
    bordered Cholesky update on the device), until the GPs' capacity (``gp_capacity``) is reached;
    the next control step runs on the extended model.  Hyperparameters stay as trained.

    ``sliding=True`` keeps learning past the capacity: every step still appends
    ``append_per_step`` rows, the oldest rows making room for them on the device
    (``append_data(evict_oldest=True)``), so the training set is a moving window of fixed size.

    ``device_data=True`` keeps the data where it is born: ``obs``, ``action`` and ``status`` live in
    preallocated device tensors that are copied out once at the end, and learning goes through
    ``GPMPC.observe`` (preprocessing and append on the device).  The host generator still draws the random
    picks, with the same call and seed as the host path, so both paths learn from the same transitions;
    the only upload per step is those picks, an int32 index tensor.  ``select="variance"`` (needs
    ``device_data=True``) picks the step's transitions where the GPs are least certain instead
    (``BatchSolver.informative``) and uploads nothing; ``select="greedy"`` (likewise) picks them one after the other,
    each conditioned on the ones before it (``BatchSolver.select``).  The two paths differ by rounding in the targets.

    ``evict="redundant"`` (needs ``device_data=True, sliding=True``) chooses what leaves the full window as well: the
    rows the GPs would miss least (``GPMPC.observe(evict="redundant")``, ``BatchSolver.redundant``) instead of the
    oldest.

    Returns the dict of :func:`run_evaluation` plus ``n_train`` (steps,), the training rows after
    each step; with ``device_data=True`` also ``pick``, the list of every step's picked indices."""
    if select not in ("random", "variance", "greedy"):
        raise ValueError("select must be 'random', 'variance' or 'greedy'")
    if select != "random" and not device_data:
        raise ValueError(f"select='{select}' picks on the device: it needs device_data=True")
    if evict not in (None, "redundant"):
        raise ValueError("evict must be None or 'redundant'")
    if evict is not None and not (device_data and sliding):
        raise ValueError(f"evict='{evict}' chooses the rows that leave on the device: it needs device_data=True, sliding=True")
    if device_data:
        return _run_online_episode_device(ctrl, x0, steps, append_per_step, seed, tstep0, sliding, refresh_every, select,
                                          evict)
    ctrl.reset()
    solver = ctrl.solver
    dev = solver.device
    B = solver.batch
    rng = np.random.default_rng(seed)
    obs = torch.tensor(np.asarray(x0, dtype=np.float64).reshape(B, -1), device=dev)
    ts = torch.tensor(np.zeros(B) if tstep0 is None else tstep0, dtype=torch.int32, device=dev)
    data = {"obs": [obs.cpu().numpy()], "action": [], "status": [], "inference_time_data": [], "n_train": []}
    for step in range(steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        u = ctrl.select_action_batch(obs, ts.clone())
        torch.cuda.synchronize(dev)
        data["inference_time_data"].append(time.perf_counter() - t0)
        data["action"].append(u.cpu().numpy())
        data["status"].append(solver.status.cpu().numpy())
        obs = solver.plant_step(obs, u, ts)   # advances the reference index too
        data["obs"].append(obs.cpu().numpy())
        n, cap = solver.gp_size(0)
        pick = rng.choice(B, min(append_per_step, B), replace=False)
        if not sliding:
            pick = pick[:max(cap - n, 0)]
        if len(pick):
            inputs, targets = ctrl.preprocess_data(data["obs"][-2][pick], data["action"][-1][pick],
                                                   data["obs"][-1][pick])
            ctrl.append_data(inputs, targets, evict_oldest=sliding)
        if refresh_every > 0 and (step + 1) % refresh_every == 0:
            ctrl.refresh_gps()
        data["n_train"].append(solver.gp_size(0)[0])
    return {k: np.array(v) for k, v in data.items()}


def _run_online_episode_device(ctrl, x0, steps, append_per_step, seed, tstep0, sliding, refresh_every, select,
                               evict=None) -> dict:
    """:func:`run_online_episode` with ``device_data=True``: the same loop on device tensors."""
    ctrl.reset()
    # what makes room in a full window: the oldest rows, or the rows evict names
    room_for = dict(evict=evict) if evict is not None else dict(evict_oldest=sliding)
    solver = ctrl.solver
    dev = solver.device
    B = solver.batch
    rng = np.random.default_rng(seed)
    obs = torch.empty(steps + 1, B, solver.nx, dtype=torch.float64, device=dev)
    action = torch.empty(steps, B, solver.nu, dtype=torch.float64, device=dev)
    status = torch.empty(steps, B, dtype=torch.int32, device=dev)
    obs[0].copy_(torch.as_tensor(np.asarray(x0, dtype=np.float64).reshape(B, -1)))
    ts = torch.tensor(np.zeros(B) if tstep0 is None else tstep0, dtype=torch.int32, device=dev)
    times, n_train, picks = [], [], []
    for step in range(steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        u = ctrl.select_action_batch(obs[step], ts.clone())
        torch.cuda.synchronize(dev)
        times.append(time.perf_counter() - t0)
        action[step].copy_(u)
        status[step].copy_(solver.status)
        solver.plant_step(obs[step], action[step], ts, out=obs[step + 1])   # advances the reference index too
        n, cap = solver.gp_size(0)
        room = None if sliding else max(cap - n, 0)
        if select == "random":
            pick = rng.choice(B, min(append_per_step, B), replace=False)
            if not sliding:
                pick = pick[:room]
            if len(pick):
                pick = torch.as_tensor(pick.astype(np.int32)).to(dev)
                ctrl.observe(obs[step], action[step], obs[step + 1], pick=pick, **room_for)
            picks.append(pick)
        else:
            m = min(append_per_step, B) if sliding else min(append_per_step, B, room)
            pick = np.zeros(0, dtype=np.int32)
            if m:
                # (the indices are read back after the episode; the rows they name are the appended inputs)
                pick = (solver.informative(obs[step], action[step], m) if select == "variance"
                        else solver.select(obs[step], action[step], m)[0])
                ctrl.observe(obs[step], action[step], obs[step + 1], pick=pick, **room_for)
            picks.append(pick)
        if refresh_every > 0 and (step + 1) % refresh_every == 0:
            ctrl.refresh_gps()
        n_train.append(solver.gp_size(0)[0])
    return {"obs": obs.cpu().numpy(), "action": action.cpu().numpy(), "status": status.cpu().numpy(),
            "inference_time_data": np.array(times), "n_train": np.array(n_train),
            "pick": [p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p, dtype=np.int32) for p in picks]}


def sample_data(data: dict, n_samples: int, rng: np.random.Generator):
    """Random transitions (x, u, x_next) from an episode batch (`scripts/run_gp_mpc.py:75-83`):
    the (step, instance) pairs are sampled without replacement."""
    steps, B = data["action"].shape[:2]
    n = steps * B
    idx = rng.choice(n, n_samples, replace=False) if n_samples < n else np.arange(n)
    k, b = idx // B, idx % B
    return data["obs"][k, b], data["action"][k, b], data["obs"][k + 1, b]


def tracking_cost(data: dict, traj: np.ndarray, tstep0: np.ndarray | None = None) -> float:
    """Mean squared position-state tracking error of an episode batch against the reference."""
    obs = data["obs"][1:]
    steps, B = obs.shape[:2]
    t0 = np.zeros(B, dtype=int) if tstep0 is None else np.asarray(tstep0, dtype=int)
    idx = (t0[None, :] + 1 + np.arange(steps)[:, None]) % traj.shape[1]
    ref = traj[:, idx].transpose(1, 2, 0)
    return float(((obs - ref) ** 2).sum(-1).mean())


def prediction_error(ctrl, data: dict, horizon: int, stride: int = 1, with_gp: bool = True) -> np.ndarray:
    """Multi-step prediction error of the controller's model on a recorded run: the standard check of a learned
    model, no counterpart in the reference.  ``data`` is a :func:`run_evaluation` dict, ``obs`` (S+1, B, nx) and
    ``action`` (S, B, nu).  Every window starting at s = 0, stride, 2 stride, ... <= S - horizon is rolled out
    open-loop from ``obs[s]`` under the recorded actions, all windows and instances in one
    ``ctrl.solver.rollout`` call (P = windows x B).  Returns (horizon, nx): the root mean square over windows and
    instances of ``x_pred[k] - obs[s + k]``, k = 1 .. horizon.  ``with_gp=False`` gives the prior's curve to set
    beside the learned model's."""
    x0, u, want = _prediction_windows(data, horizon, stride)
    solver = ctrl.solver
    x = solver.rollout(torch.as_tensor(np.ascontiguousarray(x0), device=solver.device),
                       torch.as_tensor(np.ascontiguousarray(u), device=solver.device), with_gp=with_gp)
    err = x.cpu().numpy()[:, 1:] - want[:, 1:]
    return np.sqrt((err ** 2).mean(axis=0))


def _prediction_windows(data: dict, horizon: int, stride: int):
    """The windows of :func:`prediction_error`: x0 (W B, nx), u (W B, horizon, nu) and the recorded states
    (W B, horizon+1, nx), window-major, then instance."""
    obs = np.asarray(data["obs"], dtype=np.float64)
    act = np.asarray(data["action"], dtype=np.float64)
    S, B = act.shape[:2]
    horizon, stride = int(horizon), int(stride)
    if horizon < 1 or stride < 1:
        raise ValueError("horizon and stride must be at least 1")
    if horizon > S:
        raise ValueError(f"horizon {horizon} exceeds the run's {S} steps")
    starts = np.arange(0, S - horizon + 1, stride)
    steps = starts[:, None] + np.arange(horizon + 1)[None, :]                       # (W, horizon+1)
    x0 = obs[starts].reshape(len(starts) * B, -1)                                    # window-major, then instance
    u = act[steps[:, :horizon]].transpose(0, 2, 1, 3).reshape(len(starts) * B, horizon, -1)
    want = obs[steps].transpose(0, 2, 1, 3).reshape(len(starts) * B, horizon + 1, -1)
    return x0, u, want


def prediction_calibration(ctrl, data: dict, horizon: int, stride: int = 1, feedback=None) -> np.ndarray:
    """Whether the model's own uncertainty matches its multi-step error on a recorded run.  The windows are
    :func:`prediction_error`'s, rolled out in one ``ctrl.solver.rollout_lin`` call with the state covariance
    propagated from zero and the likelihood noise included (``with_noise=True``); ``feedback`` is None (open loop),
    ``"lqr"`` (the controller's ``lqr_gain``) or a gain (nu, nx).  Returns (horizon, nx): the root mean square over
    windows and instances of ``(x_pred[k] - obs[s + k]) / sqrt(diag Sigma_k)``, k = 1 .. horizon.  Values near 1 mean
    calibrated uncertainty, above 1 overconfidence.  A state whose predicted variance is 0 somewhere (one the
    uncertainty has not reached yet) gives NaN at that step."""
    x0, u, want = _prediction_windows(data, horizon, stride)
    solver = ctrl.solver
    K = ctrl.lqr_gain if isinstance(feedback, str) and feedback == "lqr" else feedback
    if isinstance(K, str):
        raise ValueError('feedback is None, "lqr" or a gain (nu, nx)')
    out = solver.rollout_lin(torch.as_tensor(np.ascontiguousarray(x0), device=solver.device),
                             torch.as_tensor(np.ascontiguousarray(u), device=solver.device), cov=True, K=K,
                             with_noise=True)
    err = out["x"].cpu().numpy()[:, 1:] - want[:, 1:]
    var = np.diagonal(out["cov"].cpu().numpy()[:, 1:], axis1=-2, axis2=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        z2 = np.where(var > 0.0, err ** 2 / var, np.nan)
    return np.sqrt(z2.mean(axis=0))


def tightening_coverage(ctrl, x0, u, n_samples: int, seed: int = 0, feedback="lqr", with_noise: bool = True) -> np.ndarray:
    """Whether the linearised, diagonal covariance the tightening relies on covers what the model's own belief
    produces.  ``x0`` (nx,) / (P, nx) and ``u`` (T, nu) / (P, T, nu) as in ``ctrl.predict_trajectory``; ``x̄`` and
    ``cov`` come from ``ctrl.predict_trajectory(x0, u, return_cov=True, feedback=feedback, with_noise=with_noise)`` and
    the particles from ``ctrl.sample_trajectories(x0, u, n_samples, seed=seed, feedback=feedback,
    with_noise=with_noise)``, the same feedback and noise.  Returns (T+1, nx): for stage k and state i the fraction
    of particles (over samples and trajectories) with ``|x_k[i] - x̄_k[i]| <= icdf sqrt(cov_k[i][i])``, ``icdf`` the
    controller's ``inverse_cdf``.  Stage 0 and entries whose predicted variance is zero somewhere report NaN.  A value
    near the controller's ``prob`` means the tightening's half-width holds the sampled futures as often as it claims."""
    xbar, cov = ctrl.predict_trajectory(x0, u, return_cov=True, feedback=feedback, with_noise=with_noise)
    x, _ = ctrl.sample_trajectories(x0, u, n_samples, seed=seed, feedback=feedback, with_noise=with_noise)
    xbar, cov, x = np.asarray(xbar), np.asarray(cov), np.asarray(x)
    if xbar.ndim == 2:
        xbar, cov, x = xbar[None], cov[None], x[None]
    var = np.diagonal(cov, axis1=-2, axis2=-1)                                   # (P, T+1, nx)
    with np.errstate(invalid="ignore"):
        half = ctrl.inverse_cdf * np.sqrt(var)
    inside = np.abs(x - xbar[:, None]) <= half[:, None]                          # (P, S, T+1, nx)
    frac = inside.mean(axis=(0, 1))
    frac[~(var > 0.0).all(axis=0)] = np.nan
    frac[0] = np.nan
    return frac


def learn(n_epochs: int, ctrl, lr: float, gp_iterations: int, seed: int, samples_per_epoch: int,
          episode_len: int, x0: np.ndarray | None = None, tstep0: np.ndarray | None = None,
          report_prediction: int = 0):
    """Episodic learning (`scripts/run_gp_mpc.py:86-137`): epoch 0 runs the prior MPC; every
    epoch then fits the GPs on all data gathered so far and runs a test and a train episode
    batch with GP-MPC.  Returns (train_runs, test_runs, timing) dicts keyed by epoch.

    ``report_prediction=h > 0``: every epoch's test run also records :func:`prediction_error` at horizon h on
    itself, the learned model's curve and the prior's, under the key ``"prediction_error"`` of its dict:
    ``{"gp": (h, nx), "prior": (h, nx)}``, and beside it :func:`prediction_calibration` of the learned model (open
    loop) under the key ``"calibration"``, (h, nx).  Off by default, which leaves the returned runs as they were."""
    from . import distributed as D

    spec = ctrl.model
    rank, size = D.world()
    rng = np.random.default_rng(seed if size == 1 else [seed, rank])
    B = ctrl.batch
    if x0 is None:   # this rank's shard of the B * size instances
        ids = D.shard_range(B, rank)
        x0_all, t_all = initial_states(spec, ctrl.traj, B * size, seed=seed)
        x0, tstep0 = x0_all[ids.start:ids.stop], t_all[ids.start:ids.stop]
    train_runs, test_runs, timing = {}, {}, {}
    plant = ctrl.solver
    train_runs[0] = run_evaluation(ctrl.prior_ctrl, x0, episode_len, tstep0, plant_solver=plant)
    test_runs[0] = run_evaluation(ctrl.prior_ctrl, x0, episode_len, tstep0, plant_solver=plant)
    x_train = np.zeros((0, sum(spec.gp_dims)))
    y_train = np.zeros((0, spec.n_gp))
    for epoch in range(1, n_epochs + 1):
        state, actions, next_state = sample_data(train_runs[epoch - 1], samples_per_epoch, rng)
        inputs, targets = ctrl.preprocess_data(state, actions, next_state)
        # every rank's new transitions, in rank order (one all-gather per epoch)
        inputs, targets = D.gather_rows(inputs), D.gather_rows(targets)
        x_train = np.vstack((x_train, inputs))
        y_train = np.vstack((y_train, targets))
        t3 = time.perf_counter()
        ctrl.train_gp(x=x_train, y=y_train, lr=lr, iterations=gp_iterations)
        t4 = time.perf_counter()
        test_runs[epoch] = run_evaluation(ctrl, x0, episode_len, tstep0)
        t5 = time.perf_counter()
        train_runs[epoch] = run_evaluation(ctrl, x0, episode_len, tstep0)
        t6 = time.perf_counter()
        if report_prediction > 0:
            test_runs[epoch]["prediction_error"] = {
                "gp": prediction_error(ctrl, test_runs[epoch], report_prediction),
                "prior": prediction_error(ctrl, test_runs[epoch], report_prediction, with_gp=False)}
            test_runs[epoch]["calibration"] = prediction_calibration(ctrl, test_runs[epoch], report_prediction)
        timing[epoch] = {"train_gp": t4 - t3, "test": t5 - t4, "collect": t6 - t5, "n_train": len(x_train)}
    return train_runs, test_runs, timing


def get_runtime(test_runs: dict, train_runs: dict) -> dict:
    """Mean / std / max per-step inference time per epoch, first step dropped
    (`gpmpc/plotting.py:10-37`)."""
    epochs = sorted(test_runs)
    mean = np.zeros(len(epochs))
    std = np.zeros(len(epochs))
    mx = np.zeros(len(epochs))
    n_train = []
    for i, e in enumerate(epochs):
        rt = np.asarray(test_runs[e]["inference_time_data"][1:])
        mean[i], std[i], mx[i] = rt.mean(), rt.std(), rt.max()
        n_train.append(int(np.prod(train_runs[e]["action"].shape[:2])))
    return {"mean": mean, "std": std, "max": mx, "num_train_samples": n_train}


def save_runtime_csv(runtime: dict, num_points_per_epoch, save_dir: Path) -> Path:
    """runtime.csv with the reference's columns (`gpmpc/plotting.py:61-62`)."""
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    data = np.vstack((num_points_per_epoch, runtime["mean"], runtime["std"], runtime["max"])).T
    path = save_dir / "runtime.csv"
    np.savetxt(path, data, delimiter=",", header="Train Steps, Mean, Std, Max")
    return path
