#!/usr/bin/env python3
"""Timing of BatchSolver.rollout (gpmpc_rollout) beside the chain of plant steps.

Times, between two device synchronisations, one call of each side on the same inputs (x0 from initial_states, u near
u_eq):

    gp         rollout(with_gp=True)               the learned model, one launch
    gp_var     rollout(with_gp=True, var=True)     plus the gather and one variance launch per GP
    prior      rollout(with_gp=False)              the prior alone, one launch
    prior_var  rollout(with_gp=False, var=True)
    plant      T chained plant_step launches at the prior's parameters: the only comparable thing the library
               could do before, and what `prior` equals bit for bit

The sides alternate in one process: `--repeats` rounds, each timing every side `--calls` times after `--warmup`
untimed calls; a round's figure is the median over its calls.  Prints one JSON object: per side the median round's
ms per call, every round listed and the spread (max - min) / median over the rounds.

    python tools/rollout_ab.py                 # quad2d N=200 P=1024 T=30
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

SIDES = ("gp", "gp_var", "prior", "prior_var", "plant")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="quad2d")
    ap.add_argument("--train", type=int, default=200, help="training rows per GP")
    ap.add_argument("--trajectories", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--sides", nargs="+", choices=SIDES, default=list(SIDES))
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rollout_ab.py measures on the GPU: no HIP device available")
    from gpmpc.gp import GaussianProcess
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver
    from gpmpc.synthetic import DEFAULT_HYPERS, initial_states, make_training_data

    spec = get_spec(args.model)
    P, T = args.trajectories, args.steps
    s = BatchSolver(spec, 5, 2)
    gps = []
    for i, (X, y) in enumerate(make_training_data(spec, args.train, seed=1)):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gp.set_hyperparameters(*DEFAULT_HYPERS[spec.name][i])
        gps.append(gp)
    s.set_gps(gps)
    dev = s.device
    x0, _ = initial_states(spec, spec.reference_trajectory(), P)
    rng = np.random.default_rng(args.seed)
    x0t = torch.tensor(x0, device=dev)
    ut = torch.tensor(spec.u_eq + 0.1 * rng.standard_normal((P, T, spec.nu)), device=dev)
    us = [ut[:, k].contiguous() for k in range(T)]
    bufs = [torch.empty_like(x0t) for _ in range(2)]

    def plant():
        x = x0t
        for k in range(T):
            x = s.plant_step(x, us[k], params=spec.prior, out=bufs[k & 1])
        return x

    side = {"gp": lambda: s.rollout(x0t, ut), "gp_var": lambda: s.rollout(x0t, ut, var=True),
            "prior": lambda: s.rollout(x0t, ut, with_gp=False), "prior_var": lambda: s.rollout(x0t, ut, with_gp=False, var=True),
            "plant": plant}

    def timed(fn):
        ms = []
        for i in range(args.warmup + args.calls):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if i >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms)

    assert torch.equal(s.rollout(x0t, ut, with_gp=False)[:, -1], plant()), "the prior rollout is the chain of plant steps"
    rounds = {name: [] for name in args.sides}
    for _ in range(args.repeats):
        for name in args.sides:
            rounds[name].append(timed(side[name]))
    out = {"config": {k: getattr(args, k) for k in ("model", "train", "trajectories", "steps", "calls", "warmup", "repeats",
                                                     "seed")}}
    for name in args.sides:
        med = statistics.median(rounds[name])
        out[name] = {"ms_per_call": round(med, 4), "ms_per_call_rounds": [round(r, 4) for r in rounds[name]],
                     "spread": round((max(rounds[name]) - min(rounds[name])) / med, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
