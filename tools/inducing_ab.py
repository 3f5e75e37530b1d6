#!/usr/bin/env python3
"""A/B of how the FITC inducing rows are chosen: greedily on the device (gpmpc_gp_inducing) against random draws.

Uploads the exact GPs of `--model` on `--rows` synthetic training rows (gpmpc.synthetic.make_training_data, the
default hyperparameters), reserves them and, per GP, alternates `--repeats` times over the sides

    greedy   BatchSolver.inducing_gp(g, M, tol=0), then BatchSolver.fitc_gp(g, picks, y, jitter)
    tol      BatchSolver.inducing_gp(g, M, tol=--tol): the selection ends where it ends, then the same build
    random   `--draws` draws of M rows (numpy default_rng(seed + k).choice), each built with the same jitter

and reports, per GP and side: the time of the selection and of the build it feeds (a host clock around each call;
both calls are synchronous and return with their device work completed), every run listed with its median, the
number of inducing rows, and the mean gap, the largest absolute difference between the FITC mean and the exact GP
mean over the training rows (gpmpc_gp_predict before and after the build).  A random draw whose build fails its
pivot at the given jitter is reported as failed, not retried.  Prints one JSON object.

    python tools/inducing_ab.py                                      # quad2d, 400 rows, M = 30
    python tools/inducing_ab.py --model quad3d --rows 4000 --M 2000  # the large sparse configuration
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


def timed(torch, call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="quad2d")
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--M", type=int, default=30, help="inducing rows (the cap, for --tol)")
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--jitter", type=float, default=0.0)
    ap.add_argument("--draws", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1337)
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("inducing_ab.py measures on the GPU: no HIP device available")
    from gpmpc.gp import GaussianProcess
    from gpmpc.models import get_spec
    from gpmpc.solver import BatchSolver
    from gpmpc.synthetic import DEFAULT_HYPERS, make_training_data

    spec = get_spec(args.model)
    n, M = args.rows, min(args.M, args.rows)
    s = BatchSolver(spec, 5, 2)
    data = make_training_data(spec, n, seed=1)
    gps = []
    for i, (X, y) in enumerate(data):
        gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
        gps.append(gp.set_hyperparameters(*DEFAULT_HYPERS[spec.name][i]))
    s.set_gps(gps)
    out = {"config": {k: getattr(args, k) for k in ("model", "rows", "M", "tol", "jitter", "draws", "repeats", "seed")}}
    for g, (X, y) in enumerate(data):
        s.reserve_gp(g, n)
        Xt, yt = torch.tensor(X, device=s.device), torch.tensor(y, device=s.device)
        exact = s.gp_predict(g, Xt, var=False)[0].clone()

        def build(idx):
            """(ok, build ms, mean gap) of the FITC mean on idx; the exact mean is restored afterwards."""
            ok, ms = timed(torch, lambda: s.fitc_gp(g, idx, yt, args.jitter))
            if not ok:
                return 0, ms, None
            gap = float((s.gp_predict(g, Xt, var=False)[0] - exact).abs().max())
            s.drop_fitc(g)
            return 1, ms, gap

        sides = {"greedy": [], "tol": []}
        sides.update({f"random{k}": [] for k in range(args.draws)})
        s.inducing_gp(g, M, 0.0)   # (untimed: the first launches load the code objects)
        for _ in range(args.repeats):
            for name in sides:
                if name.startswith("random"):
                    idx = np.random.default_rng(args.seed + int(name[6:])).choice(n, M, replace=False).astype(np.int32)
                    sel_ms = 0.0
                else:
                    idx, sel_ms = timed(torch, lambda: s.inducing_gp(g, M, 0.0 if name == "greedy" else args.tol))
                ok, fitc_ms, gap = build(idx)
                sides[name].append(dict(rows=int(len(idx)), ok=ok, select_ms=sel_ms, fitc_ms=fitc_ms, gap=gap))
        res = {}
        for name, runs in sides.items():
            res[name] = dict(rows=runs[0]["rows"], ok=[r["ok"] for r in runs],
                             gap=runs[0]["gap"] if runs[0]["ok"] else "failed",
                             select_ms_runs=[round(r["select_ms"], 4) for r in runs],
                             select_ms=statistics.median(r["select_ms"] for r in runs),
                             fitc_ms_runs=[round(r["fitc_ms"], 4) for r in runs],
                             fitc_ms=statistics.median(r["fitc_ms"] for r in runs))
        out[f"gp{g}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
