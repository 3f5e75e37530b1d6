#!/usr/bin/env python3
"""Timing of BatchSolver.rollout (gpmpc_rollout) beside the chain of plant steps, of BatchSolver.rollout_lin
(gpmpc_rollout_lin) beside the plain rollout, and of BatchSolver.rollout_sample (gpmpc_rollout_sample) beside the
step-by-step host loop it replaces.

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
    sample     rollout_sample(xref=rollout, K=lqr, clip=True, xi=randn, with_noise=True, var=True)   one launch
    sample_host  what could be done for the same end before: T times {feedback and clip in torch, rollout(T=1,
               var=True), the draw sqrt(var + noise) xi in torch, added to the new state through dt df/dgm at the
               equilibrium}: three launches, a drain and the torch glue per step (a first-order stand-in for the
               draw, which the library could not pass through the RK4 substages)

`--coverage S` instead prints learning.tightening_coverage of one controller of the model (GPs fitted on `--train`
rows, horizon `--steps`, S samples of each of 8 trajectories under the LQR gain) as JSON.

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

SIDES = ("gp", "gp_var", "prior", "prior_var", "plant", "lin", "lin_var", "lin_cov", "lin_prior", "sample", "sample_host")


def dfdgm(spec):
    """(n_gp, nx): the state derivative's sensitivity to each GP mean at the equilibrium, from the CPU oracle's model."""
    from oracle import gpmpc_oracle as O

    sd = spec.to_dict()
    dyn = O.Dynamics(sd, None)
    x, u = np.zeros(spec.nx), np.asarray(spec.u_eq, dtype=np.float64)
    gg = [np.zeros(len(idx)) for idx in sd["gp_inputs"]]
    rows = []
    for g in range(spec.n_gp):
        up, dn = [0.0] * spec.n_gp, [0.0] * spec.n_gp
        up[g], dn[g] = 0.5, -0.5
        rows.append(dyn._f(dyn.p, dyn.g, x, u, up, gg)[0] - dyn._f(dyn.p, dyn.g, x, u, dn, gg)[0])
    return np.array(rows)


def coverage(args, spec):
    from gpmpc.gpmpc import GPMPC
    from gpmpc.learning import tightening_coverage
    from gpmpc.synthetic import initial_states, make_training_data

    data = make_training_data(spec, args.train, seed=1)
    ctrl = GPMPC(spec.name, horizon=args.steps, batch=8, variance="exact")
    ctrl.train_gp(np.hstack([X for X, _ in data]), np.column_stack([y for _, y in data]), lr=0.05, iterations=20)
    ctrl.reset()
    x0, _ = initial_states(spec, ctrl.traj, 8)
    u = spec.u_eq + 0.1 * np.random.default_rng(args.seed).standard_normal((8, args.steps, spec.nu))
    out = {"config": {"model": spec.name, "train": args.train, "steps": args.steps, "trajectories": 8, "n_samples": args.coverage,
                      "seed": args.seed, "prob": ctrl.prob, "inverse_cdf": ctrl.inverse_cdf}}
    for fb in ("lqr", None):
        cov = tightening_coverage(ctrl, x0, u, args.coverage, seed=args.seed, feedback=fb)
        out["lqr" if fb else "open_loop"] = [[None if np.isnan(v) else round(float(v), 4) for v in row] for row in cov]
    print(json.dumps(out))


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
    ap.add_argument("--coverage", type=int, default=0, metavar="S", help="print the tightening_coverage table instead")
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
    if args.coverage:
        return coverage(args, spec)
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
    xref = s.rollout(x0t, ut)
    xit = torch.randn(P, T, spec.n_gp, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(args.seed))
    Kt = torch.tensor(K, device=dev).T.contiguous()
    lo, hi = torch.tensor(spec.u_lo, device=dev), torch.tensor(spec.u_hi, device=dev)
    noise = torch.tensor([DEFAULT_HYPERS[spec.name][i][2] for i in range(spec.n_gp)], dtype=torch.float64, device=dev)
    # dt df/dgm at the equilibrium, (n_gp, nx): central differences of the prior-form model in the GP means
    G = torch.tensor(spec.dt * dfdgm(spec), device=dev)

    def sample_host():
        x = x0t
        for k in range(T):
            uk = torch.minimum(torch.maximum(ut[:, k] + (x - xref[:, k]) @ Kt, lo), hi)
            xn, var = s.rollout(x, uk[:, None].contiguous(), var=True)
            x = xn[:, 1] + (torch.sqrt(torch.clamp(var[:, 0] + noise, min=0.0)) * xit[:, k]) @ G
        return x

    side.update({"sample": lambda: s.rollout_sample(x0t, ut, xref=xref, K=K, clip=True, xi=xit, with_noise=True, var=True),
                 "sample_host": sample_host})

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
    if "sample" in args.sides and "sample_host" in args.sides:   # how far the first-order stand-in ends from the launch
        out["sample_vs_host_max_abs"] = float((side["sample"]()["x"][:, -1] - sample_host()).abs().max())
    for name in args.sides:
        med = statistics.median(rounds[name])
        out[name] = {"ms_per_call": round(med, 4), "ms_per_call_rounds": [round(r, 4) for r in rounds[name]],
                     "spread": round((max(rounds[name]) - min(rounds[name])) / med, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
