"""Cost of a sliding training window on an uploaded GP: one 16-row ``BatchSolver.drop_gp`` (a rank-16
update of the inverse factor on the device, csrc/gp_drop.hip), one "drop 16 + append 16" round
(``drop_gp`` then ``append_gp``: the window moves, the size stays), and the re-upload of the same
final rows through ``gpmpc_set_gp`` (K, its inverse and Cholesky factor on the host, repack,
reallocate, synchronous upload: what ``BatchSolver.set_gps`` does per GP).

All three are bracketed by HIP events on the handle's stream (torch's current stream), 20
repetitions after 5 warm-up repetitions; the GP is the model's second one (d = 3).  The plain drops
run on a GP uploaded with N + 16 * 25 rows, so the last timed one leaves N rows; the rounds run on
N rows at capacity N throughout; the re-upload is always of N rows, with the Python GP's cached
covariances dropped before each repetition (new data invalidates them).  A record, not a pass mark.

  python tools/drop_bench.py [model:N ...]      (GPU only; default quad2d:200 quad2d:1000 quad3d:4000)
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

WARMUP, REPS, M, G = 5, 20, 16, 1


def bench(name: str, N: int) -> dict:
    spec = get_spec(name)
    extra = M * (WARMUP + REPS)
    data = make_training_data(spec, N + extra, seed=3)
    hyp = DEFAULT_HYPERS[name]

    def gp_of(g, lo, hi):
        X, y = data[g]
        return GaussianProcess(torch.tensor(X[lo:hi]), torch.tensor(y[lo:hi])).set_hyperparameters(*hyp[g])

    s = BatchSolver(spec, 10, 4)
    flags = []
    # plain drops: N + extra rows down to N
    s.set_gps([gp_of(g, 0, N + extra) for g in range(spec.n_gp)])
    s.reserve_gp(G, N + extra)
    timed(lambda r: flags.append(s.drop_gp(G, M)), WARMUP)
    drop = timed(lambda r: flags.append(s.drop_gp(G, M)), REPS)
    assert s.gp_size(G) == (N, N + extra)
    # rounds at a fixed size: N rows, capacity N
    s.set_gps([gp_of(g, 0, N) for g in range(spec.n_gp)])
    s.reserve_gp(G, N)
    X, y = (torch.tensor(a, device="cuda") for a in data[G])

    def round_(r, base):
        lo = N + M * (base + r)
        flags.append(s.drop_gp(G, M))
        flags.append(s.append_gp(G, X[lo:lo + M], y[lo:lo + M]))

    timed(lambda r: round_(r, 0), WARMUP)
    rnd = timed(lambda r: round_(r, WARMUP), REPS)
    assert s.gp_size(G) == (N, N)
    ok = int(torch.cat(flags).sum())
    final = gp_of(G, extra, N + extra)
    timed(lambda r: upload_one(s, G, final), WARMUP)
    up = timed(lambda r: upload_one(s, G, final), REPS)
    return {"model": name, "gp": G, "N": N, "rows": M, "drop_ms_median": float(np.median(drop)),
            "drop_ms_min": float(min(drop)), "round_ms_median": float(np.median(rnd)), "round_ms_min": float(min(rnd)),
            "upload_ms_median": float(np.median(up)), "upload_ms_min": float(min(up)), "ok_blocks": ok,
            "blocks": len(flags)}


def main():
    cases = [a.split(":") for a in sys.argv[1:]] or [("quad2d", 200), ("quad2d", 1000), ("quad3d", 4000)]
    for name, N in cases:
        print(json.dumps(bench(name, int(N))), flush=True)


if __name__ == "__main__":
    main()
