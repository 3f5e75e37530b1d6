"""Cost of refitting an uploaded GP's hyperparameters: one ``BatchSolver.fit_gp`` (Adam on the device from
the handle's own factor, inputs and scratch, csrc/gp_fit.hip, ending in the refactorisation at the fitted
hyperparameters) against what ``GPMPC.refit_hyperparameters(fit="torch")`` does per GP:
``fit_gp(gp, n_train, lr, device="cuda")`` (a torch Cholesky, an autograd backward and a host
synchronisation per step) followed by ``BatchSolver.refactor_gp``.

Both are synchronous calls, so each is timed by the wall clock between two ``torch.cuda.synchronize()``:
the median of 5 repetitions after 1 warm-up, in the same process, each from raw parameters 0 (gpytorch's
start), 20 iterations at lr 0.1, where the loss still moves by more than the early stop's 1e-3 per step;
``iters`` reports the iterations either path ran (from the controller's default hyperparameters at lr 0.01
the rule ends both fits after 17, 2 and 2 iterations at the three default sizes).  ``mll_ms`` is one ``BatchSolver.gp_mll``
(gp_fit_grad_kernel, gp_fit_finish_kernel and the one-thread kernel that stores the hyperparameters)
between two HIP events, the median of 20 after 5 warm-up calls.  The GP is the model's second one (d = 3)
at capacity N.  A record, not a pass mark.

  python tools/fit_bench.py [model:N ...]   (GPU only; default quad2d:200 quad2d:1000 quad3d:4000)
"""

import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "gp-mpc_amd"), str(ROOT), str(ROOT / "tools")]
from append_bench import timed  # noqa: E402
from gpmpc.gp import GaussianProcess, fit_gp  # noqa: E402
from gpmpc.models import get_spec  # noqa: E402
from gpmpc.solver import BatchSolver  # noqa: E402
from gpmpc.synthetic import DEFAULT_HYPERS, make_training_data  # noqa: E402

WARMUP, REPS, G, ITERS, LR = 1, 5, 1, 20, 0.1


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def bench(name: str, N: int) -> dict:
    spec = get_spec(name)
    data = make_training_data(spec, N, seed=3)
    hyp = DEFAULT_HYPERS[name]
    gps = [GaussianProcess(torch.tensor(X), torch.tensor(y)).set_hyperparameters(*hyp[g])
           for g, (X, y) in enumerate(data)]
    s = BatchSolver(spec, 10, 4)
    s.set_gps(gps)
    s.reserve_gp(G, N)
    y = torch.tensor(data[G][1], device="cuda")
    raw0 = [0.0, 0.0, 0.0]
    res = {}

    def device():
        res["device"] = s.fit_gp(G, y, raw0, LR, ITERS)

    def host():
        gp = GaussianProcess(torch.tensor(data[G][0]), torch.tensor(data[G][1]))
        for p, r in zip(gp.parameters(), raw0):
            p.fill_(r)
        it = fit_gp(gp, n_train=ITERS, lr=LR, device="cuda")
        flag = s.refactor_gp(G, y, gp.lengthscale, gp.outputscale, gp.noise)
        res["torch"] = ([float(p) for p in gp.parameters()], it, int(flag.cpu()[0]))

    wall(device, WARMUP)
    dev = wall(device, REPS)
    wall(host, WARMUP)
    tor = wall(host, REPS)
    timed(lambda r: s.gp_mll(G, y), 5)
    mll = timed(lambda r: s.gp_mll(G, y), 20)
    rd, rt = np.array(res["device"][0]), np.array(res["torch"][0])
    return {"model": name, "gp": G, "N": N, "iterations": ITERS, "lr": LR,
            "device_ms_median": float(np.median(dev)), "device_ms_min": float(min(dev)),
            "torch_ms_median": float(np.median(tor)), "torch_ms_min": float(min(tor)),
            "mll_ms_median": float(np.median(mll)), "mll_ms_min": float(min(mll)),
            "iters": [int(res["device"][1]), int(res["torch"][1])], "ok": [int(res["device"][2]), res["torch"][2]],
            "raw_max_abs_diff": float(np.abs(rd - rt).max())}


def main():
    cases = [a.split(":") for a in sys.argv[1:]] or [("quad2d", 200), ("quad2d", 1000), ("quad3d", 4000)]
    for name, N in cases:
        print(json.dumps(bench(name, int(N))), flush=True)


if __name__ == "__main__":
    main()
