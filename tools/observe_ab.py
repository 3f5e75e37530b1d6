#!/usr/bin/env python3
"""A/B of the learning part of the online loop: host preprocessing against the device path (GPMPC.observe).

Runs the closed loop of gpmpc.learning.run_online_episode (select_action_batch, plant_step) on a sliding window
and times, per control step, only the part that learns: from after the plant step to the end of the append,
between two device synchronisations.

    host    obs / action copied to the host, the picks drawn there, GPMPC.preprocess_data in numpy, the rows
            uploaded per GP and appended (GPMPC.append_data(evict_oldest=True)): run_online_episode's default
    device  obs / action copied into preallocated device tensors, the same picks drawn on the host and uploaded
            as an int32 index tensor, GPMPC.observe(evict_oldest=True): device_data=True

The two sides alternate in one process, `--repeats` runs each after `--warmup` untimed steps, every run on a fresh
controller; the window starts full, so every timed step drops and appends `--rows` rows.  Prints one JSON object:
the median run's ms per step for each side (a run's figure is the median over its steps), every run listed, the
ratio of the medians, and the solve's ms per step for scale.

    python tools/observe_ab.py                 # quad2d B=1024 H=30 capacity 400, 16 rows per step

`--select` changes the axis: every side is the device path, and the sides differ in who picks the step's rows.

    random    the host generator's picks, uploaded (the device side above)
    variance  GPMPC.observe(select="variance"): gpmpc_gp_informative, the top rows by variance one by one
    greedy    GPMPC.observe(select="greedy"): gpmpc_gp_select, each row conditioned on the rows before it

    python tools/observe_ab.py --select variance greedy

alternates the sides named, in the order given, and prints the same figures per side, the ratio of the last side's
median to the first's and the launches one selection queues (the gather, a variance launch per GP, and for greedy
the V launch, the start state and one launch per row).

`--evict` changes the axis again: every side is the device path with one selection (the first `--select` value,
greedy by default), and the sides differ in what leaves the full window.

    oldest     GPMPC.observe(evict_oldest=True): gpmpc_gp_drop_oldest inside gpmpc_gp_observe
    redundant  GPMPC.observe(evict="redundant"): gpmpc_gp_redundant (the start state and one launch per row), then
               gpmpc_gp_drop_rows on every GP (one launch that sorts, three per block of 16 rows)

    python tools/observe_ab.py --evict oldest redundant
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "gp-mpc_amd", ROOT):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def run(args, torch, device_data: bool, select: str = "random", evict: str = "oldest") -> dict:
    from gpmpc.gp import GaussianProcess
    from gpmpc.gpmpc import GPMPC
    from gpmpc.synthetic import DEFAULT_HYPERS, initial_states, make_training_data

    B = args.batch
    ctrl = GPMPC(args.model, horizon=args.horizon, batch=B, gp_capacity=args.capacity)
    spec = ctrl.model
    gps = []
    for i, (X, y) in enumerate(make_training_data(spec, args.capacity, seed=1)):
        # (on the device, as train_gp leaves them: the Python GPs then follow both paths without a host copy)
        gp = GaussianProcess(torch.tensor(X, device=ctrl.device), torch.tensor(y, device=ctrl.device))
        gp.set_hyperparameters(*DEFAULT_HYPERS[spec.name][i])
        gps.append(gp)
    ctrl.set_gaussian_processes(gps)
    ctrl.reset()
    solver = ctrl.solver
    dev = solver.device
    x0, phase = initial_states(spec, ctrl.traj, B)
    rng = np.random.default_rng(args.seed)
    steps = args.warmup + args.steps
    obs = torch.empty(steps + 1, B, spec.nx, dtype=torch.float64, device=dev)
    action = torch.empty(steps, B, spec.nu, dtype=torch.float64, device=dev)
    obs[0].copy_(torch.as_tensor(x0))
    ts = torch.tensor(phase, dtype=torch.int32, device=dev)
    host_obs = [obs[0].cpu().numpy()]
    learn_ms, solve_ms, bad = [], [], 0
    room_for = dict(evict="redundant") if evict == "redundant" else dict(evict_oldest=True)
    for step in range(steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        u = ctrl.select_action_batch(obs[step], ts.clone())
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        bad += int((~((solver.status == 0) | (solver.status == 2))).sum())
        solver.plant_step(obs[step], u, ts, out=obs[step + 1])
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        # ---- the learning part
        if device_data and select != "random":
            action[step].copy_(u)
            ctrl.observe(obs[step], action[step], obs[step + 1], m=min(args.rows, B), select=select, **room_for)
        elif device_data:
            action[step].copy_(u)
            pick = rng.choice(B, min(args.rows, B), replace=False)
            ctrl.observe(obs[step], action[step], obs[step + 1], pick=torch.as_tensor(pick.astype(np.int32)).to(dev),
                         **room_for)
        else:
            act = u.cpu().numpy()
            host_obs.append(obs[step + 1].cpu().numpy())
            pick = rng.choice(B, min(args.rows, B), replace=False)
            inputs, targets = ctrl.preprocess_data(host_obs[-2][pick], act[pick], host_obs[-1][pick])
            ctrl.append_data(inputs, targets, evict_oldest=True)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        if step >= args.warmup:
            learn_ms.append(1e3 * (t3 - t2))
            solve_ms.append(1e3 * (t1 - t0))
    assert solver.gp_size(0) == (args.capacity, args.capacity)
    return {"learn_ms_per_step": statistics.median(learn_ms), "learn_ms_min": min(learn_ms), "learn_ms_max": max(learn_ms),
            "solve_ms_per_step": statistics.median(solve_ms), "bad_status": bad}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="quad2d")
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--capacity", type=int, default=400)
    ap.add_argument("--rows", type=int, default=16, help="rows learned per step")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--select", nargs="+", choices=("random", "variance", "greedy"), default=None,
                    help="compare these selections on the device path instead of host against device")
    ap.add_argument("--evict", nargs="+", choices=("oldest", "redundant"), default=None,
                    help="compare these eviction rules on the device path (selection: the first --select value, greedy "
                         "by default)")
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("observe_ab.py measures on the GPU: no HIP device available")
    if args.evict:
        return main_evict(args, torch)
    if args.select:
        return main_select(args, torch)
    runs = {False: [], True: []}
    for _ in range(args.repeats):
        for device_data in (False, True):
            runs[device_data].append(run(args, torch, device_data))
    out = {"config": {k: getattr(args, k) for k in ("model", "horizon", "batch", "capacity", "rows", "steps", "warmup",
                                                     "repeats", "seed")}}
    for device_data, name in ((False, "host"), (True, "device")):
        rs = sorted(runs[device_data], key=lambda r: r["learn_ms_per_step"])
        med = dict(rs[len(rs) // 2])
        med["learn_ms_per_step_runs"] = [round(r["learn_ms_per_step"], 4) for r in runs[device_data]]
        out[name] = med
    out["host_over_device"] = out["host"]["learn_ms_per_step"] / out["device"]["learn_ms_per_step"]
    print(json.dumps(out))


def main_select(args, torch):
    from gpmpc.models import get_spec

    runs = {name: [] for name in args.select}
    for _ in range(args.repeats):
        for name in args.select:
            runs[name].append(run(args, torch, True, name))
    out = {"config": {k: getattr(args, k) for k in ("model", "horizon", "batch", "capacity", "rows", "steps", "warmup",
                                                     "repeats", "seed", "select")}}
    n_gp, m = get_spec(args.model).n_gp, min(args.rows, args.batch)
    launches = {"random": 0, "variance": 1 + n_gp + 2, "greedy": 1 + n_gp + 2 + m}
    for name in args.select:
        rs = sorted(runs[name], key=lambda r: r["learn_ms_per_step"])
        med = dict(rs[len(rs) // 2])
        med["learn_ms_per_step_runs"] = [round(r["learn_ms_per_step"], 4) for r in runs[name]]
        med["selection_launches"] = launches[name]
        out[name] = med
    first, last = args.select[0], args.select[-1]
    out[f"{last}_over_{first}"] = out[last]["learn_ms_per_step"] / out[first]["learn_ms_per_step"]
    print(json.dumps(out))


def main_evict(args, torch):
    from gpmpc.models import get_spec

    select = args.select[0] if args.select else "greedy"
    runs = {name: [] for name in args.evict}
    for _ in range(args.repeats):
        for name in args.evict:
            runs[name].append(run(args, torch, True, select, name))
    out = {"config": {k: getattr(args, k) for k in ("model", "horizon", "batch", "capacity", "rows", "steps", "warmup",
                                                     "repeats", "seed", "evict")}}
    out["config"]["select"] = select
    n_gp, m = get_spec(args.model).n_gp, min(args.rows, args.batch)
    blocks = (m + 15) // 16
    launches = {"oldest": 3 * blocks * n_gp, "redundant": 1 + m + (1 + 3 * blocks) * n_gp}
    for name in args.evict:
        rs = sorted(runs[name], key=lambda r: r["learn_ms_per_step"])
        med = dict(rs[len(rs) // 2])
        med["learn_ms_per_step_runs"] = [round(r["learn_ms_per_step"], 4) for r in runs[name]]
        med["eviction_launches"] = launches[name]
        out[name] = med
    first, last = args.evict[0], args.evict[-1]
    out[f"{last}_over_{first}"] = out[last]["learn_ms_per_step"] / out[first]["learn_ms_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
