#!/usr/bin/env python3
"""Timing of BatchSolver.rollout (gpmpc_rollout) beside the chain of plant steps, and of BatchSolver.rollout_lin
(gpmpc_rollout_lin) beside the plain rollout.

Times, between two device synchronisations, one call of each side on the same inputs (x0 from initial_states, u near
u_eq):

    gp         rollout(with_gp=True)               the learned model, one launch
    gp_var     rollout(with_gp=True, var=True)     plus the gather and one variance launch per GP
    prior      rollout(with_gp=False)              the prior alone, one launch
    prior_var  rollout(with_gp=False, var=True)
    plant      T chained plant_step launches at the prior's parameters: the only comparable thing the library
               could do before, and what `prior` equals bit for bit
    lin        rollout_lin(with_gp=True)           the states and the Jacobians A_k, B_k, one launch
    lin_var    rollout_lin(var=True)               plus the gather and the variance launches
    lin_cov    rollout_lin(cov=True, K=lqr, with_noise=True)   plus the covariance launch (variances in scratch)
    lin_prior  rollout_lin(with_gp=False)          the prior's Jacobians

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

SIDES = ("gp", "gp_var", "prior", "prior_var", "plant", "lin", "lin_var", "lin_cov", "lin_prior")


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
    from gpmpc.solver import BatchSolver, setup_prior_dynamics
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
    K = setup_prior_dynamics(*spec.prior_jacobian(np.zeros(spec.nx), spec.u_eq), np.diag(spec.q_diag), np.diag(spec.r_diag), spec.dt)[2]
    side.update({"lin": lambda: s.rollout_lin(x0t, ut), "lin_var": lambda: s.rollout_lin(x0t, ut, var=True),
                 "lin_cov": lambda: s.rollout_lin(x0t, ut, cov=True, K=K, with_noise=True),
                 "lin_prior": lambda: s.rollout_lin(x0t, ut, with_gp=False)})

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
    assert torch.equal(s.rollout_lin(x0t, ut)["x"], s.rollout(x0t, ut)), "rollout_lin's states are the rollout's"
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
