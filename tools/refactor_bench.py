"""Cost of refactorising an uploaded GP on the device: one ``BatchSolver.refactor_gp`` (a blocked
Cholesky factorisation and triangular inverse from the handle's own rows, csrc/gp_refactor.hip)
against the re-upload of the same rows through ``gpmpc_set_gp`` (K, its inverse and Cholesky factor
on the host, repack, reallocate, synchronous upload: what ``BatchSolver.set_gps`` does per GP).

Both are bracketed by HIP events on the handle's stream (torch's current stream), 20 repetitions
after 5 warm-up repetitions, in the same process on the same rows; the GP is the model's second one
(d = 3), at capacity N, with the Python GP's cached covariances dropped before each upload (new data
or new hyperparameters invalidate them).  ``launches`` is the refactorisation's kernel count,
2 ceil(N / 16) + 4.  A record, not a pass mark.

  python tools/refactor_bench.py [model:N ...]   (GPU only; default quad2d:200 quad2d:1000 quad3d:4000)
"""

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "gp-mpc_amd"), str(ROOT), str(ROOT / "tools")]
from append_bench import timed, upload_one  # noqa: E402
from gpmpc.gp import GaussianProcess  # noqa: E402
from gpmpc.models import get_spec  # noqa: E402
from gpmpc.solver import BatchSolver  # noqa: E402
from gpmpc.synthetic import DEFAULT_HYPERS, make_training_data  # noqa: E402

WARMUP, REPS, G = 5, 20, 1


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
    flags = []
    timed(lambda r: flags.append(s.refactor_gp(G, y, *hyp[G])), WARMUP)
    ref = timed(lambda r: flags.append(s.refactor_gp(G, y, *hyp[G])), REPS)
    ok = int(torch.cat(flags).sum())
    timed(lambda r: upload_one(s, G, gps[G]), WARMUP)
    up = timed(lambda r: upload_one(s, G, gps[G]), REPS)
    return {"model": name, "gp": G, "N": N, "launches": 2 * ((N + 15) // 16) + 4,
            "refactor_ms_median": float(np.median(ref)), "refactor_ms_min": float(min(ref)),
            "upload_ms_median": float(np.median(up)), "upload_ms_min": float(min(up)), "ok": ok, "calls": len(flags)}


def main():
    cases = [a.split(":") for a in sys.argv[1:]] or [("quad2d", 200), ("quad2d", 1000), ("quad3d", 4000)]
    for name, N in cases:
        print(json.dumps(bench(name, int(N))), flush=True)


if __name__ == "__main__":
    main()
