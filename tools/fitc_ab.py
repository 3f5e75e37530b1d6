"""Time to put a fresh FITC inducing-point mean in place after the training data changed: the host path against
the device path (csrc/gp_fitc.hip), alternated in one process.

host      what a controller without ``gpmpc_gp_fitc`` has to do: ``GPMPC.precompute_sparse_posterior_mean`` in
          torch on cuda tensors (two dense ``linalg.solve``; the Python GP's covariance cache is gone after a
          change of the data, so ``compute_covariances`` rebuilds K and its inverse and ``device_layout`` the
          factor) and the ``gpmpc_set_gp`` upload of S, w, X and Linv.  ``host_cached`` is the same with K and
          the layout kept, i.e. the two solves and the upload alone.
device    ``gpmpc_gp_fitc`` on the uploaded exact GP, indices and targets already on the device (the call
          synchronises), jitter = JITTER x outputscale.

Each is a synchronous piece of work, timed by the wall clock between two ``torch.cuda.synchronize()``: REPS
repetitions a side after one warm-up each, in the order host, host_cached, device, ...  The GP is the model's
second one (d = 3).  ``mfma_flops`` counts the two M^2 n loops (V: mpad (mpad + 16) npad, lower tiles of L^-1
only; B: mpad (mpad + 16) npad, lower tiles only).  A record, not a pass mark.

  python tools/fitc_ab.py [model:N:M ...]       (GPU only; default quad2d:1000:400 quad3d:4000:2000)
  python tools/fitc_ab.py --trace model:N:M     three device builds and nothing else, for a kernel trace
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
from gpmpc.gpmpc import GPMPC  # noqa: E402
from gpmpc.models import get_spec  # noqa: E402
from gpmpc.solver import BatchSolver  # noqa: E402
from gpmpc.synthetic import DEFAULT_HYPERS, make_training_data  # noqa: E402

REPS, G, JITTER = 5, 1, 1e-8


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def setup(name: str, N: int, M: int):
    """A handle whose GPs hold N rows, reserved; GP G's Python twin on the device; indices and targets there."""
    spec = get_spec(name)
    data = make_training_data(spec, N, seed=3)
    hyp = DEFAULT_HYPERS[name]
    gps = [GaussianProcess(torch.tensor(X), torch.tensor(y)).set_hyperparameters(*hyp[g]) for g, (X, y) in enumerate(data)]
    s = BatchSolver(spec, 10, 4)
    s.set_gps(gps)
    s.reserve_gp(G, N)
    X, y = data[G]
    gp = GaussianProcess(torch.tensor(X, device="cuda"), torch.tensor(y, device="cuda")).set_hyperparameters(*hyp[G])
    idx = torch.tensor(np.random.default_rng(1337).choice(range(N), size=M, replace=False).astype(np.int32), device="cuda")
    return s, gp, idx, torch.tensor(y, device="cuda"), hyp[G]


def device_call(s, idx, y, jitter):
    ok = ctypes.c_int32()
    _lib.check(s.lib.gpmpc_gp_fitc(s._h, G, idx.shape[0], idx.data_ptr(), y.data_ptr(), jitter, ctypes.byref(ok), s._stream()))
    return ok.value


def bench(name: str, N: int, M: int) -> dict:
    s, gp, idx, y, hyp = setup(name, N, M)
    sh = BatchSolver(get_spec(name), 10, 4)   # the host side's uploads go to a handle of their own
    res = {}
    me = type("Me", (), {})()
    me.gaussian_process = [gp]

    def host(keep_cache):
        if not keep_cache:
            gp.K, gp.K_inv, gp._dev = None, None, None   # (as a change of the data leaves them)
        if gp.K is None:
            gp.K, gp.K_inv = gp.compute_covariances()
        me.np_random = np.random.default_rng(1337)
        S, w = GPMPC.precompute_sparse_posterior_mean(me, M)[0]
        lay = gp.device_layout("cpu")
        X = np.ascontiguousarray(gp.train_inputs[0].cpu().numpy())
        Linv = np.ascontiguousarray(lay["Linv"].cpu().numpy())
        S, w = np.ascontiguousarray(S), np.ascontiguousarray(w)
        _lib.check(sh.lib.gpmpc_set_gp(sh._h, G, S.shape[0], S.shape[1], S.ctypes.data, w.ctypes.data, X.shape[0],
                                       X.ctypes.data, Linv.ctypes.data, gp.lengthscale, gp.outputscale, gp.noise))
        res["host_finite"] = bool(np.isfinite(w).all())

    def device():
        res["device_ok"] = device_call(s, idx, y, JITTER * hyp[1])

    sides = {"host": lambda: host(False), "host_cached": lambda: host(True), "device": device}
    for fn in sides.values():
        wall(fn)
    ms = {k: [] for k in sides}
    for _ in range(REPS):
        for k, fn in sides.items():
            ms[k].append(wall(fn))
    mpad, npad = (M + 15) // 16 * 16, (N + 15) // 16 * 16
    out = {"model": name, "gp": G, "N": N, "M": M, "reps": REPS, "jitter": JITTER * hyp[1], "device_ok": res["device_ok"],
           "host_weights_finite": res["host_finite"], "launches": 4 * (mpad // 16) + 9,
           "mfma_flops": {"V": mpad * (mpad + 16) * npad, "B": mpad * (mpad + 16) * npad}}
    for k, v in ms.items():
        out[k + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    out["host_over_device"] = out["host_ms"]["median"] / out["device_ms"]["median"]
    out["host_cached_over_device"] = out["host_cached_ms"]["median"] / out["device_ms"]["median"]
    return out


def main():
    args = sys.argv[1:]
    if args and args[0] == "--trace":
        name, N, M = args[1].split(":")
        s, _, idx, y, hyp = setup(name, int(N), int(M))
        for _ in range(3):
            device_call(s, idx, y, JITTER * hyp[1])
        torch.cuda.synchronize()
        return
    cases = [a.split(":") for a in args] or [("quad2d", 1000, 400), ("quad3d", 4000, 2000)]
    for name, N, M in cases:
        print(json.dumps(bench(name, int(N), int(M))), flush=True)


if __name__ == "__main__":
    main()
