"""Cost of folding 16 new rows into an uploaded GP: one 16-row ``BatchSolver.append_gp`` (a bordered
Cholesky update on the device, csrc/gp_append.hip) against the re-upload of the same enlarged GP
through ``gpmpc_set_gp`` (K, its inverse and Cholesky factor on the host, repack, reallocate,
synchronous upload: what ``BatchSolver.set_gps`` does per GP).

Both are bracketed by HIP events on the handle's stream (torch's current stream), 20 repetitions
after 5 warm-up repetitions; the GP is the model's second one (d = 3).  The appends of the
repetitions follow one another, so the GP grows from N to N + 16 * 25 rows while they run; the
re-upload is always of N + 16 rows, with the Python GP's cached covariances dropped before each
repetition (new data invalidates them).  A record, not a pass mark.

  python tools/append_bench.py [model:N ...]      (GPU only; default quad2d:200 quad2d:1000 quad3d:4000)
"""

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "gp-mpc_amd"), str(ROOT)]
from gpmpc import _lib  # noqa: E402
from gpmpc.gp import GaussianProcess  # noqa: E402
from gpmpc.models import get_spec  # noqa: E402
from gpmpc.solver import BatchSolver  # noqa: E402
from gpmpc.synthetic import DEFAULT_HYPERS, make_training_data  # noqa: E402

WARMUP, REPS, M, G = 5, 20, 16, 1


def upload_one(s: BatchSolver, g: int, gp: GaussianProcess):
    """BatchSolver.set_gps for one GP: host factorisation (device_layout) and gpmpc_set_gp."""
    gp.K, gp.K_inv, gp._dev = None, None, None
    lay = gp.device_layout("cpu")
    X = np.ascontiguousarray(gp.train_inputs[0].numpy())
    alpha = np.ascontiguousarray(lay["alpha"].numpy())
    Linv = np.ascontiguousarray(lay["Linv"].numpy())
    _lib.check(s.lib.gpmpc_set_gp(s._h, g, X.shape[0], X.shape[1], X.ctypes.data, alpha.ctypes.data, 0, None,
                                  Linv.ctypes.data, gp.lengthscale, gp.outputscale, gp.noise))


def timed(fn, reps):
    ms = []
    for r in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(r)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def bench(name: str, N: int) -> dict:
    spec = get_spec(name)
    total = N + M * (WARMUP + REPS)
    data = make_training_data(spec, total, seed=3)
    hyp = DEFAULT_HYPERS[name]

    def gp_of(g, n):
        X, y = data[g]
        return GaussianProcess(torch.tensor(X[:n]), torch.tensor(y[:n])).set_hyperparameters(*hyp[g])

    s = BatchSolver(spec, 10, 4)
    s.set_gps([gp_of(g, N) for g in range(spec.n_gp)])
    s.reserve_gp(G, total)
    X, y = (torch.tensor(a, device="cuda") for a in data[G])
    flags = []

    def append(r, base):
        lo = N + M * (base + r)
        flags.append(s.append_gp(G, X[lo:lo + M], y[lo:lo + M]))

    timed(lambda r: append(r, 0), WARMUP)
    app = timed(lambda r: append(r, WARMUP), REPS)
    accepted = int(torch.cat(flags).sum())
    big = gp_of(G, N + M)
    timed(lambda r: upload_one(s, G, big), WARMUP)
    up = timed(lambda r: upload_one(s, G, big), REPS)
    return {"model": name, "gp": G, "N": N, "rows": M, "append_ms_median": float(np.median(app)),
            "append_ms_min": float(min(app)), "upload_ms_median": float(np.median(up)), "upload_ms_min": float(min(up)),
            "accepted_blocks": accepted, "blocks": WARMUP + REPS}


def main():
    cases = [a.split(":") for a in sys.argv[1:]] or [("quad2d", 200), ("quad2d", 1000), ("quad3d", 4000)]
    for name, N in cases:
        print(json.dumps(bench(name, int(N))), flush=True)


if __name__ == "__main__":
    main()
