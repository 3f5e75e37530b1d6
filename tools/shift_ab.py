#!/usr/bin/env python3
"""A/B of the one-stage shifted warm start (gpmpc_set_tuning GPMPC_TUNE_SHIFT) in the closed loop.

bench.py has no flag for the option, so this runs bench.py's timed loop (BatchSolver.solve +
plant_step, W untimed steps, K timed ones; default 5 / 20, the driver command's window) with the
option off and on, alternating, `--repeats` times each, and prints one JSON object per config:

    sqp_iter mean / max over the window, linearisations per solve (stats slot 9), status counts,
    the SQP kernel's milliseconds per step (HIP events: set_profiling / kernel_time_list),
    the slowest instance's in-kernel solve time per step and its ratio to the mean (stats slot 10),
    steps/s (instances x steps / wall time), every repeat listed, the median first.

    python tools/shift_ab.py                          # quad2d N=200 H=30 B=1024
    python tools/shift_ab.py --model cartpole --n-train 50 --horizon 20 --batch 256
    python tools/shift_ab.py --batch 128              # one shard of the eight-GPU split
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


def run(args, torch, spec, gps, lqr_mats, shift: int) -> dict:
    from gpmpc.solver import BatchSolver
    from gpmpc.synthetic import initial_states

    dev = torch.device("cuda", 0)
    B = args.batch
    solver = BatchSolver(spec, args.horizon, B, device=dev)
    solver.set_tuning(shift=shift)
    if args.lin_cache is not None:
        solver.set_tuning(lin_cache=args.lin_cache)
    solver.set_gps(gps, variance="love")
    solver.set_tightening(True, 0.95, *lqr_mats)
    solver.reset(reset_iterate=True)
    x0, phase = initial_states(spec, spec.reference_trajectory(), B, seed=1)
    obs = torch.tensor(x0, device=dev)
    tstep = torch.tensor(phase, dtype=torch.int32, device=dev)
    stats = torch.zeros(B, BatchSolver.STATS_SLOTS, dtype=torch.int64, device=dev)
    solver.set_stats(stats)

    def step():
        u0 = solver.solve(obs, tstep)
        solver.plant_step(obs, u0, tstep, out=obs)

    solver.set_profiling(True)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(dev)
    solver.kernel_time_list()
    stats.zero_()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    solver.set_profiling(False)
    kt = solver.kernel_time_list()
    st = stats.cpu().numpy().astype(np.float64)
    n = B * args.steps
    inst = st[:, 10] * 1e-5 / args.steps   # ms per step, per instance (100 MHz ticks)
    return {"steps_per_s": n / elapsed, "ms_per_step": 1e3 * elapsed / args.steps,
            "sqp_iter_mean": st[:, 0].sum() / n, "sqp_iter_max": int(st[:, 7].max()),
            "qp_iter_mean": st[:, 1].sum() / n, "lin_per_solve": st[:, 9].sum() / n,
            "status_counts": st[:, 2:7].sum(0).astype(int).tolist(),
            "sqp_kernel_ms_per_step": sum(kt["sqp_ms"]) / max(len(kt["sqp_ms"]), 1),
            "var_kernel_ms_per_step": sum(kt["var_ms"]) / max(len(kt["var_ms"]), 1),
            "slowest_instance_ms": float(inst.max()), "mean_instance_ms": float(inst.mean()),
            "slowest_over_mean": float(inst.max() / inst.mean()), "launch": solver.launch_info()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="quad2d")
    ap.add_argument("--n-train", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lin-cache", type=int, choices=[0, 1], default=None, help="GPMPC_TUNE_LIN_CACHE on both sides")
    args = ap.parse_args(argv)

    import torch

    from gpmpc.gp import GaussianProcess
    from gpmpc.models import get_spec
    from gpmpc.solver import setup_prior_dynamics
    from gpmpc.synthetic import DEFAULT_HYPERS, make_training_data

    spec = get_spec(args.model)
    gps = []
    for i, (X, y) in enumerate(make_training_data(spec, args.n_train, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS[spec.name][i])
        gps.append(gp)
    dfdx, dfdu = spec.prior_jacobian(np.zeros(spec.nx), spec.u_eq)
    lqr_mats = setup_prior_dynamics(dfdx, dfdu, np.diag(spec.q_diag), np.diag(spec.r_diag), spec.dt)

    runs = {0: [], 1: []}
    for _ in range(args.repeats):
        for shift in (0, 1):
            runs[shift].append(run(args, torch, spec, gps, lqr_mats, shift))
    out = {"config": {"model": spec.name, "n_train": args.n_train, "horizon": args.horizon, "batch": args.batch,
                      "steps": args.steps, "warmup": args.warmup, "lin_cache": args.lin_cache}}
    for shift, name in ((0, "off"), (1, "on")):
        rs = sorted(runs[shift], key=lambda r: r["steps_per_s"])
        med = dict(rs[len(rs) // 2])   # the median repeat's figures
        med["steps_per_s_runs"] = [round(r["steps_per_s"]) for r in runs[shift]]
        med["sqp_kernel_ms_per_step_runs"] = [round(r["sqp_kernel_ms_per_step"], 4) for r in runs[shift]]
        out[name] = med
    out["on_over_off"] = {k: out["on"][k] / out["off"][k] for k in ("steps_per_s", "sqp_iter_mean", "sqp_kernel_ms_per_step",
                                                                     "slowest_instance_ms", "mean_instance_ms")}
    out["steps_per_s_median"] = {k: statistics.median(r["steps_per_s"] for r in runs[s]) for s, k in ((0, "off"), (1, "on"))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
