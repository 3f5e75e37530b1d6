"""Time to put a fresh LOVE variance root in place after an append of 16 rows: the host path against the
device path (csrc/gp_love.hip), alternated in one process.

host      what a controller without ``gpmpc_gp_love_root`` has to do once the training set has changed:
          ``GaussianProcess.love_root(rank)`` in torch on cuda tensors (the Python GP's covariance cache is
          gone after ``append_data``, so it rebuilds K and, as ``compute_covariances`` does, its inverse),
          the root's copy to the host and ``gpmpc_set_gp_variance_root``.  ``host_lanczos`` is the same with
          the covariance cache kept, i.e. the Lanczos loop, the eigendecomposition and the upload alone.
device    ``gpmpc_gp_love_root`` on a start vector already on the device (the call synchronises); with
          ``device_readback`` the host copy ``BatchSolver.love_root_gp`` also takes for ``love_roots``.

Each is a synchronous piece of work, timed by the wall clock between two ``torch.cuda.synchronize()``: REPS
repetitions a side after one warm-up each, in the order host, device, host, device, ...  The GP is the
model's second one (d = 3, no breakdown: the root has the full rank).  ``launches_per_iteration`` is what
``launch_gp_love_iteration`` queues.  A record, not a pass mark.

  python tools/love_root_ab.py [model:N ...]       (GPU only; default quad2d:1000 quad3d:4000)
  python tools/love_root_ab.py --trace model:N     three device builds and nothing else, for a kernel trace
"""

import ctypes
import json
import sys
import time
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

REPS, G, RANK, M = 5, 1, 100, 16
LAUNCHES_PER_ITERATION = 6   # matvec, three orthogonalisation steps, decide, next (gp_love.hip)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def setup(name: str, N: int):
    """A handle whose GPs hold N rows after an append of M, and GP G's Python twin on the device."""
    spec = get_spec(name)
    data = make_training_data(spec, N, seed=3)
    hyp = DEFAULT_HYPERS[name]
    gps = [GaussianProcess(torch.tensor(X[:N - M]), torch.tensor(y[:N - M])).set_hyperparameters(*hyp[g])
           for g, (X, y) in enumerate(data)]
    s = BatchSolver(spec, 10, 4)
    s.set_gps(gps)
    X, y = data[G]
    s.reserve_gp(G, N)
    assert s.append_gp(G, X[N - M:], y[N - M:]).cpu().tolist() == [1]
    gp = GaussianProcess(torch.tensor(X, device="cuda"), torch.tensor(y, device="cuda")).set_hyperparameters(*hyp[G])
    gen = torch.Generator(device="cpu").manual_seed(0)
    q0 = torch.randn(N, dtype=torch.float64, generator=gen).cuda()
    return s, gp, q0


def device_call(s, q0):
    r, ok = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(s.lib.gpmpc_gp_love_root(s._h, G, RANK, q0.data_ptr(), ctypes.byref(r), ctypes.byref(ok), s._stream()))
    assert ok.value == 1
    return r.value


def bench(name: str, N: int) -> dict:
    s, gp, q0 = setup(name, N)
    res = {}

    def host(keep_cache):
        if not keep_cache:
            gp.K, gp.K_inv = None, None   # (as GaussianProcess.append_data leaves them)
        R = np.ascontiguousarray(gp.love_root(RANK).cpu().numpy())
        _lib.check(s.lib.gpmpc_set_gp_variance_root(s._h, G, R.shape[0], R.shape[1], R.ctypes.data))
        res["host_rank"] = R.shape[1]

    def device():
        res["device_rank"] = device_call(s, q0)

    def device_readback():
        s.love_root_gp(G, RANK, start=q0)

    sides = {"host": lambda: host(False), "host_lanczos": lambda: host(True), "device": device,
             "device_readback": device_readback}
    for fn in sides.values():
        wall(fn)
    ms = {k: [] for k in sides}
    for _ in range(REPS):
        for k, fn in sides.items():
            ms[k].append(wall(fn))
    out = {"model": name, "gp": G, "N": N, "rank": RANK, "reps": REPS, "ranks": [res["host_rank"], res["device_rank"]],
           "launches_per_iteration": LAUNCHES_PER_ITERATION, "khat_bytes_per_product": 8 * ((N + 15) // 16 * 16) ** 2}
    for k, v in ms.items():
        out[k + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    out["host_over_device"] = out["host_ms"]["median"] / out["device_ms"]["median"]
    out["host_lanczos_over_device"] = out["host_lanczos_ms"]["median"] / out["device_ms"]["median"]
    return out


def main():
    args = sys.argv[1:]
    if args and args[0] == "--trace":
        name, N = args[1].split(":")
        s, _, q0 = setup(name, int(N))
        for _ in range(3):
            device_call(s, q0)
        torch.cuda.synchronize()
        return
    cases = [a.split(":") for a in args] or [("quad2d", 1000), ("quad3d", 4000)]
    for name, N in cases:
        print(json.dumps(bench(name, int(N))), flush=True)


if __name__ == "__main__":
    main()
