"""Cross-stream ordering of the C ABI (include/gpmpc_mi355x.h, "Streams"): the table of every call that takes a
stream, and the harness of tests/test_gpu_stream_order.py.

The rule under test: a call that takes the handle and a stream ends by recording the handle's event on its stream
(csrc/capi.hip StreamMark), and a call on another stream first waits for that event (order_after_last).  TABLE
names every function of the header with a `void* stream` parameter as ORDERED (it follows the rule, and
test_gpu_stream_order.py runs it both as the second call behind a writer and as the delayed first call before one)
or EXEMPT (with the reason); tests/test_stream_order_cpu.py holds the table against the header, so a new entry point
fails there until it is classified.

`ordered(env, case)` makes a missing wait visible in two ways.  Stream A is held up by a delay (torch.cuda._sleep,
calibrated by events); `first` is queued on A behind it and `second` on another stream B, both through the C ABI
with pointers staged beforehand, so nothing between the delay and the last record copies from the host.  Then
  (a) after the event recorded on B behind `second` has completed, the delay's end event must be complete: with the
      wait in place B's work follows A's, without it B finishes while the delay still runs;
  (b) for asynchronous calls the delay's end event must still be pending when `second` returns to the host
      (otherwise the delay was too short to show anything: the case fails, it does not pass by default);
  (c) every output of both calls and a probe of the handle afterwards (predict and mean_grad of both GPs at 7 points,
      the solution, an installed LOVE root and FITC mean) equal, bit for bit, the same two calls made on one stream
      with a synchronise between them on an identically prepared handle;
and, so that (c) means something, the same comparison against the calls in the other order (or with one of them left
out, where the other order is refused) must differ in at least one array.

Every buffer a pair touches is allocated before the pair starts (gpmpc_gp_reserve at CAP rows, the scratch of
informative / select / redundant / observe by the fixture's timing pass), and no setup call runs with work in
flight: a missing wait gives wrong numbers, never an access outside an allocation.  The synchronous builders
(gpmpc_gp_love_root, gpmpc_gp_fitc with M >= 1) allocate what they install inside the call, by design.
"""

from __future__ import annotations

import ctypes
import re
import time
from dataclasses import dataclass
from pathlib import Path

import numpy as np

HEADER = Path(__file__).resolve().parents[1] / "include" / "gpmpc_mi355x.h"
ORDERED, EXEMPT = "ordered", "exempt"

# function -> (kind, what of the handle it reads or writes on the device / why it is exempt)
TABLE = {
    "gpmpc_gp_append": (ORDERED, "writes rows, weights, factor (moves it to the second buffer) and tile pack"),
    "gpmpc_gp_drop_oldest": (ORDERED, "rewrites rows, weights, factor and tile pack through the drop scratch"),
    "gpmpc_gp_drop_rows": (ORDERED, "as gpmpc_gp_drop_oldest, and the sorted set in the drop scratch"),
    "gpmpc_gp_refactor": (ORDERED, "rewrites weights, factor and tile pack; the second factor buffer is its work space"),
    "gpmpc_gp_mll": (ORDERED, "reads rows and factor, writes the fit scratch"),
    "gpmpc_gp_fit": (ORDERED, "gpmpc_gp_refactor's writes, repeatedly; synchronises its stream"),
    "gpmpc_gp_love_root": (ORDERED, "reads rows and factor, builds Khat in the second factor buffer; synchronises its stream"),
    "gpmpc_get_gp_variance_root": (ORDERED, "reads the installed root (replaced by synchronous calls only: no "
                                            "asynchronous call writes what it reads)"),
    "gpmpc_gp_fitc": (ORDERED, "reads rows and factor, builds V in the second factor buffer; with M >= 1 "
                               "synchronises its stream, with M = 0 queues nothing and only switches the mean back"),
    "gpmpc_get_gp_fitc": (ORDERED, "reads the installed overlay"),
    "gpmpc_reset": (ORDERED, "clears has_prev, t_prev and, if asked, iterate and multipliers"),
    "gpmpc_set_iterate": (ORDERED, "writes iterate, clears multipliers and t_prev"),
    "gpmpc_solve": (ORDERED, "reads every GP, reads and writes iterate, multipliers, variances, tightening, caches"),
    "gpmpc_get_solution": (ORDERED, "reads iterate and tightening"),
    "gpmpc_get_variance": (ORDERED, "reads the tightening variances"),
    "gpmpc_gp_predict": (ORDERED, "reads rows, weights and factor"),
    "gpmpc_gp_mean_grad": (ORDERED, "reads the tile pack"),
    "gpmpc_gp_posterior": (EXEMPT, "takes no handle: every buffer is the caller's"),
    "gpmpc_plant_step": (ORDERED, "nothing of the handle since its parameters travel by value; ordered because its "
                                  "inputs are gpmpc_solve's outputs and its tstep the next solve's input (its record is "
                                  "deferred until a call arrives on another stream)"),
    "gpmpc_preprocess": (EXEMPT, "the model parameters travel by value in the kernel arguments: nothing of the "
                                 "handle is read on the device"),
    "gpmpc_gp_informative": (ORDERED, "reads rows and factor of every GP, writes the observe scratch"),
    "gpmpc_gp_select": (ORDERED, "reads rows and factor of every GP, writes the observe and select scratch"),
    "gpmpc_gp_redundant": (ORDERED, "reads the factor of every GP, writes its scratch"),
    "gpmpc_gp_observe": (ORDERED, "gpmpc_gp_append's writes for every GP, through the observe scratch"),
}


def stream_functions(header: Path = HEADER) -> list[str]:
    """Every function the header declares with a `void* stream` parameter, in declaration order."""
    text = re.sub(r"/\*.*?\*/", " ", header.read_text(), flags=re.S)
    out = []
    for name, params in re.findall(r"\bgpmpc_status\s+(gpmpc_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", params):
            out.append(name)
    return out


# ------------------------------------------------------------------------------------------------ sizes (the issue's)
H, B = 5, 8
N0, CAP = 28, 64          # rows uploaded per GP, rows reserved
M_APP, M_DROP = 5, 3      # 28 + 5 crosses a multiple of 16: the factor moves to the second buffer
RANK, M_FITC = 8, 8
M_PICK, P_PTS = 3, 8      # informative / select / redundant picks, candidate points
P_OBS, M_OBS = 8, 5
NPROBE = 7
SF2, SN2 = 1.0, 1e-3
ELL = (0.2, 2.0)
ELL_NEW, ELL_NEWER = 1.3, 0.8   # factors on GP 0's lengthscale: the writer's refactor, and a second one
DROP_IDX = (17, 2, 9)           # valid at every row count a pair can reach (25 .. 33)
FITC_IDX = tuple(range(0, 24, 3))

# The delay: DELAY_MULT times the largest device or host time of an asynchronous call, at least DELAY_FLOOR_MS.
# Measured serially at these shapes on one MI355X (test_call_times_and_the_delay prints the table): the slowest
# asynchronous call is gpmpc_solve, 0.58 ms on the device (0.02 ms on the host); gpmpc_gp_observe 0.09 / 0.05 ms, the
# drops 0.07 / 0.03 ms, every other one below 0.06 ms on either side; the synchronous ones 0.22 ms (fit, LOVE root) and
# 0.09 ms (FITC).  Between the delay's record and the return of `second` the host issues two calls and the device
# runs at most one of them, so 20 x the slowest (11.7 ms) leaves a factor of 10 over a pair.  The floor covers what
# that table cannot show, a host thread descheduled on a shared machine between the two calls (scheduler quanta are a
# few ms, so 30 ms is several of them), and it is what sets the delay at these shapes; a case then costs about 40 ms.
# Both are robustness margins, not bounds: condition (b) fails a case whose delay ran out.
DELAY_MULT = 20.0
DELAY_FLOOR_MS = 30.0
DELAY_CAP_MS = 400.0       # the delay is bounded: a calibration gone wrong must not stall the suite


class Call:
    """One C-ABI call with its pointers staged: issue(stream) makes it and returns its host outputs; `outs` are the
    device outputs (pre-filled with NaN / -77, so an output that was not written compares as such)."""

    def __init__(self, fn, label, issue, outs, sync=False, keep=()):
        assert fn in TABLE, fn
        self.fn, self.label, self.issue, self.outs, self.sync, self.keep = fn, label, issue, outs, sync, keep


@dataclass
class Case:
    id: str
    make: object            # env -> (first, second[, third]): stages the calls' device inputs and outputs
    state: str = "base"     # "base", "love1" (a LOVE root on GP 1), "fitc1" (a FITC mean on GP 1)
    sens: str = "swap"      # the run (c) must differ from: the other order, or "omit_first" / "omit_second"
    first_null: bool = False   # `first` on the default stream (NULL) instead of A


class Delay:
    """A bounded device delay on a stream: torch.cuda._sleep where torch has it, else a chain of matmuls;
    its rate is measured with events, never assumed."""

    def __init__(self, torch):
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is None:
            self.mat = torch.randn(1024, 1024, device="cuda")
        self.per_ms = None
        for unit in (1 << 20, 1 << 24) if self.sleep else (8, 64):
            self._run(unit)   # (the first launch loads the code object)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._run(unit)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms > 0:
                self.per_ms = unit / ms
            if ms >= 2.0:
                break
        assert self.per_ms, "the delay op could not be calibrated"

    def _run(self, units):
        if self.sleep:
            self.sleep(int(units))
        else:
            m = self.mat
            for _ in range(int(units)):
                m = (m @ self.mat).mul_(1.0 / 1024)

    def queue(self, stream, ms):
        assert 0 < ms <= DELAY_CAP_MS, ms
        with self.torch.cuda.stream(stream):
            self._run(max(1, int(ms * self.per_ms)))

    def measure(self, ms):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cur = torch.cuda.current_stream()
        e0.record(cur)
        self.queue(cur, ms)
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


class Env:
    """The handle of the issue's shapes and everything the calls are staged from."""

    def __init__(self):
        import torch

        from gpmpc import _lib
        from gpmpc.gp import GaussianProcess
        from gpmpc.models import get_spec
        from gpmpc.solver import BatchSolver
        from gpmpc.synthetic import initial_states, make_training_data
        from helpers import lqr
        import observe_ref as OR

        self.torch, self._lib = torch, _lib
        self.spec = spec = get_spec("quad2d")
        self.s = BatchSolver(spec, H, B)
        self.lib, self.h = self.s.lib, self.s._h
        self.dev = self.s.device
        pool = make_training_data(spec, CAP, seed=11)
        self.X = [np.ascontiguousarray(X) for X, _ in pool]
        self.y = [np.ascontiguousarray(y) for _, y in pool]
        self.gps = []
        for g in range(2):
            gp = GaussianProcess(torch.tensor(self.X[g][:N0]), torch.tensor(self.y[g][:N0]))
            gp.set_hyperparameters(ELL[g], SF2, SN2)
            self.gps.append(gp)
        self.mats = lqr(spec)
        rng = np.random.default_rng(5)
        x0, phase = initial_states(spec, spec.reference_trajectory(), B)
        self.x0 = self.t(x0)
        self.x0a = self.t(x0 + 0.02 * rng.standard_normal(x0.shape))
        self.x0b = self.t(x0 + 0.02 * rng.standard_normal(x0.shape))
        self.tstep = self.t(phase, torch.int32)
        self.y_dev = [self.t(y) for y in self.y]               # targets of the pool's rows, CAP of them
        self.Z = [self.t(np.ascontiguousarray(rng.uniform(X[:N0].min(0), X[:N0].max(0), (NPROBE, X.shape[1]))))
                  for X in self.X]
        px, pu = OR.transitions(spec, P_OBS, seed=9)
        self.px, self.pu = self.t(px), self.t(pu)
        self.pxn = self.s.plant_step(self.px, self.pu)
        self.xit = self.t(x0[:, None, :] + 0.01 * rng.standard_normal((B, H + 1, spec.nx)))
        self.uit = self.t(np.asarray(spec.u_eq)[None, None, :] + 0.01 * rng.standard_normal((B, H, spec.nu)))
        self.q0 = self.t(rng.standard_normal(CAP))
        self.p_true = np.ascontiguousarray(spec.param_vector(spec.true_params), dtype=np.float64)
        self.p_prior = np.ascontiguousarray(spec.param_vector(spec.prior), dtype=np.float64)
        torch.cuda.synchronize()
        self.delay = Delay(torch)
        self.times: dict = {}
        self.delay_ms = None
        self.A = self.Bs = self.Bnull = None

    # ------------------------------------------------------------------ staging helpers
    def t(self, a, dtype=None):
        torch = self.torch
        return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device=self.dev)

    def fout(self, *shape):
        return self.torch.full(shape, float("nan"), dtype=self.torch.float64, device=self.dev)

    def iout(self, *shape):
        return self.torch.full(shape, -77, dtype=self.torch.int32, device=self.dev)

    def check(self, status):
        self._lib.check(status)

    # ------------------------------------------------------------------ the handle's state before a pair
    def prepare(self, state="base"):
        """Upload, reserve, tighten, reset, the state's overlay, two solves (the second one tightened, so every
        buffer a probe reads has been written since the reset), synchronise."""
        torch, s = self.torch, self.s
        torch.cuda.synchronize()
        s.set_gps(self.gps)
        for g in range(2):
            s.reserve_gp(g, CAP)
        s.set_tightening(True, 0.95, *self.mats)
        s.reset(reset_iterate=True)
        if state == "love1":
            r, ok = ctypes.c_int32(), ctypes.c_int32()
            self.check(self.lib.gpmpc_gp_love_root(self.h, 1, RANK, self.q0.data_ptr(), ctypes.byref(r), ctypes.byref(ok),
                                                   s._stream()))
            assert ok.value == 1 and r.value == RANK, (r.value, ok.value)
        elif state == "fitc1":
            assert s.fitc_gp(1, np.array(FITC_IDX, dtype=np.int32), self.y_dev[1][:N0], jitter=1e-6) == 1
        else:
            assert state == "base", state
        # (from two different states: the variances the second solve's tightening used, at the first one's solution,
        # are then not the ones a third solve computes at the second one's)
        s.solve(self.x0a, self.tstep)
        s.solve(self.x0, self.tstep)
        torch.cuda.synchronize()

    def probe(self):
        """The handle's state as later calls see it: predictions of both GPs, the solution, installed overlays."""
        torch, s = self.torch, self.s
        out = {}
        for g in range(2):
            m, v = s.gp_predict(g, self.Z[g], with_noise=True)
            tm, tg = s.gp_mean_grad(g, self.Z[g])
            out.update({f"probe.gp{g}.mean": m, f"probe.gp{g}.var": v, f"probe.gp{g}.tmean": tm, f"probe.gp{g}.grad": tg})
            out[f"probe.gp{g}.size"] = np.array(s.gp_size(g))
            n, r = ctypes.c_int32(), ctypes.c_int32()
            if self.lib.gpmpc_get_gp_variance_root(self.h, g, ctypes.byref(n), ctypes.byref(r), None, None) == 0:
                out[f"probe.gp{g}.root"] = s.variance_root(g)
            if s.fitc_size(g):
                out[f"probe.gp{g}.fitc_idx"], out[f"probe.gp{g}.fitc_w"] = s.fitc_mean(g)
        out["probe.x"], out["probe.u"], out["probe.tight"] = s.solution()
        torch.cuda.synchronize()
        return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}

    # ------------------------------------------------------------------ the calls, staged
    def append(self, g=0):
        X, y, acc = self.t(self.X[g][N0:N0 + M_APP]), self.t(self.y[g][N0:N0 + M_APP]), self.iout(1)
        return Call("gpmpc_gp_append", f"append{g}", lambda st: self.check(self.lib.gpmpc_gp_append(
            self.h, g, M_APP, X.data_ptr(), y.data_ptr(), acc.data_ptr(), st)), dict(accepted=acc), keep=(X, y))

    def drop_oldest(self, g=0):
        ok = self.iout(1)
        return Call("gpmpc_gp_drop_oldest", f"drop_oldest{g}", lambda st: self.check(self.lib.gpmpc_gp_drop_oldest(
            self.h, g, M_DROP, ok.data_ptr(), st)), dict(ok=ok))

    def drop_rows(self, g=0):
        idx, dropped, ok = self.t(DROP_IDX, self.torch.int32), self.iout(M_DROP), self.iout(1)
        return Call("gpmpc_gp_drop_rows", f"drop_rows{g}", lambda st: self.check(self.lib.gpmpc_gp_drop_rows(
            self.h, g, M_DROP, idx.data_ptr(), dropped.data_ptr(), ok.data_ptr(), st)), dict(dropped=dropped, ok=ok),
            keep=(idx,))

    def refactor(self, g=0, scale=ELL_NEW):
        ok = self.iout(1)
        return Call("gpmpc_gp_refactor", f"refactor{g}x{scale}", lambda st: self.check(self.lib.gpmpc_gp_refactor(
            self.h, g, self.y_dev[g].data_ptr(), ELL[g] * scale, SF2, SN2, ok.data_ptr(), st)), dict(ok=ok))

    def mll(self, g=0):
        out = self.fout(4)
        return Call("gpmpc_gp_mll", f"mll{g}", lambda st: self.check(self.lib.gpmpc_gp_mll(
            self.h, g, self.y_dev[g].data_ptr(), out.data_ptr(), st)), dict(mll=out))

    def fit(self, g=0):
        hist = self.fout(2, 4)
        start = np.log(np.expm1(np.array([ELL[g], SF2, SN2 - 1e-6])))

        def issue(st):
            raw, iters, ok = start.copy(), ctypes.c_int32(), ctypes.c_int32()
            self.check(self.lib.gpmpc_gp_fit(self.h, g, self.y_dev[g].data_ptr(), 0.05, 2,
                                             raw.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(iters),
                                             ctypes.byref(ok), hist.data_ptr(), st))
            return dict(raw=raw, iters=iters.value, ok=ok.value)

        return Call("gpmpc_gp_fit", f"fit{g}", issue, dict(hist=hist), sync=True)

    def love_root(self, g=0):
        def issue(st):
            r, ok = ctypes.c_int32(), ctypes.c_int32()
            self.check(self.lib.gpmpc_gp_love_root(self.h, g, RANK, self.q0.data_ptr(), ctypes.byref(r), ctypes.byref(ok), st))
            return dict(rank=r.value, ok=ok.value)

        return Call("gpmpc_gp_love_root", f"love_root{g}", issue, {}, sync=True)

    def get_root(self, g):
        R = self.fout(CAP * RANK)
        return Call("gpmpc_get_gp_variance_root", f"get_root{g}", lambda st: self.check(
            self.lib.gpmpc_get_gp_variance_root(self.h, g, None, None, R.data_ptr(), st)), dict(R=R))

    def fitc(self, g=0):
        idx = self.t(FITC_IDX, self.torch.int32)

        def issue(st):
            ok = ctypes.c_int32()
            self.check(self.lib.gpmpc_gp_fitc(self.h, g, M_FITC, idx.data_ptr(), self.y_dev[g].data_ptr(), 1e-6,
                                              ctypes.byref(ok), st))
            return dict(ok=ok.value)

        return Call("gpmpc_gp_fitc", f"fitc{g}", issue, {}, sync=True, keep=(idx,))

    def fitc_off(self, g):
        return Call("gpmpc_gp_fitc", f"fitc_off{g}", lambda st: self.check(self.lib.gpmpc_gp_fitc(
            self.h, g, 0, None, None, 0.0, None, st)), {})

    def get_fitc(self, g):
        idx, w = self.iout(M_FITC), self.fout(M_FITC)

        def issue(st):
            m = ctypes.c_int32()
            self.check(self.lib.gpmpc_get_gp_fitc(self.h, g, ctypes.byref(m), idx.data_ptr(), w.data_ptr(), st))
            return dict(M=m.value)

        return Call("gpmpc_get_gp_fitc", f"get_fitc{g}", issue, dict(idx=idx, w=w))

    def reset(self):
        return Call("gpmpc_reset", "reset", lambda st: self.check(self.lib.gpmpc_reset(self.h, B, 1, st)), {})

    def set_iterate(self):
        return Call("gpmpc_set_iterate", "set_iterate", lambda st: self.check(self.lib.gpmpc_set_iterate(
            self.h, B, self.xit.data_ptr(), self.uit.data_ptr(), st)), {})

    def solve(self, x0=None, ts=None):
        u0, res = self.fout(B, self.spec.nu), self.fout(B, 4)
        status, sqp, qp = self.iout(B), self.iout(B), self.iout(B)
        x0 = self.x0b if x0 is None else x0
        ts = self.tstep + 1 if ts is None else ts
        return Call("gpmpc_solve", "solve", lambda st: self.check(self.lib.gpmpc_solve(
            self.h, B, x0.data_ptr(), ts.data_ptr(), u0.data_ptr(), status.data_ptr(), sqp.data_ptr(),
            qp.data_ptr(), res.data_ptr(), st)), dict(u0=u0, status=status, sqp_iter=sqp, qp_iter=qp, res=res),
            keep=(x0, ts))

    def get_solution(self):
        nx, nu = self.spec.nx, self.spec.nu
        x, u, tight = self.fout(B, H + 1, nx), self.fout(B, H, nu), self.fout(B, H + 1, nx + nu)
        return Call("gpmpc_get_solution", "get_solution", lambda st: self.check(self.lib.gpmpc_get_solution(
            self.h, B, x.data_ptr(), u.data_ptr(), tight.data_ptr(), st)), dict(x=x, u=u, tight=tight))

    def get_variance(self):
        var = self.fout(B, H, 2)
        return Call("gpmpc_get_variance", "get_variance", lambda st: self.check(self.lib.gpmpc_get_variance(
            self.h, B, var.data_ptr(), st)), dict(var=var))

    def predict(self, g=0):
        mean, var = self.fout(NPROBE), self.fout(NPROBE)
        return Call("gpmpc_gp_predict", f"predict{g}", lambda st: self.check(self.lib.gpmpc_gp_predict(
            self.h, g, self.Z[g].data_ptr(), NPROBE, mean.data_ptr(), var.data_ptr(), 1, st)), dict(mean=mean, var=var))

    def mean_grad(self, g=0):
        mean, grad = self.fout(NPROBE), self.fout(NPROBE, self.spec.gp_dims[g])
        return Call("gpmpc_gp_mean_grad", f"mean_grad{g}", lambda st: self.check(self.lib.gpmpc_gp_mean_grad(
            self.h, g, self.Z[g].data_ptr(), NPROBE, mean.data_ptr(), grad.data_ptr(), st)), dict(mean=mean, grad=grad))

    def plant(self, params, label, x, tstep, u=None):
        """One plant step from x with the host parameter vector `params`; its x_next is in outs (the next step's x)."""
        xn = self.fout(B, self.spec.nx)
        u = self.pu if u is None else u
        return Call("gpmpc_plant_step", label, lambda st: self.check(self.lib.gpmpc_plant_step(
            self.h, B, params.ctypes.data, x.data_ptr(), u.data_ptr(), xn.data_ptr(), tstep.data_ptr(), st)),
            dict(x_next=xn, tstep=tstep), keep=(params, x, u))

    def informative(self):
        pick, score = self.iout(M_PICK), self.fout(P_PTS)
        return Call("gpmpc_gp_informative", "informative", lambda st: self.check(self.lib.gpmpc_gp_informative(
            self.h, P_PTS, self.px.data_ptr(), self.pu.data_ptr(), M_PICK, pick.data_ptr(), score.data_ptr(), st)),
            dict(pick=pick, score=score))

    def select(self):
        pick, gain, resid, ok = self.iout(M_PICK), self.fout(M_PICK), self.fout(2, P_PTS), self.iout(1)
        return Call("gpmpc_gp_select", "select", lambda st: self.check(self.lib.gpmpc_gp_select(
            self.h, P_PTS, self.px.data_ptr(), self.pu.data_ptr(), M_PICK, pick.data_ptr(), gain.data_ptr(),
            resid.data_ptr(), ok.data_ptr(), st)), dict(pick=pick, gain=gain, resid=resid, ok=ok))

    def redundant(self):
        pick, score, ok = self.iout(M_PICK), self.fout(M_PICK), self.iout(1)
        return Call("gpmpc_gp_redundant", "redundant", lambda st: self.check(self.lib.gpmpc_gp_redundant(
            self.h, M_PICK, pick.data_ptr(), score.data_ptr(), ok.data_ptr(), st)), dict(pick=pick, score=score, ok=ok))

    def observe(self):
        inputs, targets = self.fout(M_OBS, sum(self.spec.gp_dims)), self.fout(M_OBS, 2)
        acc, dok = self.iout(2, 1), self.iout(2, 1)
        dt_diff, gravity = self.s._diff_constants()
        return Call("gpmpc_gp_observe", "observe", lambda st: self.check(self.lib.gpmpc_gp_observe(
            self.h, P_OBS, self.px.data_ptr(), self.pu.data_ptr(), self.pxn.data_ptr(), M_OBS, None, dt_diff, gravity, 0,
            inputs.data_ptr(), targets.data_ptr(), acc.data_ptr(), dok.data_ptr(), st)),
            dict(inputs=inputs, targets=targets, accepted=acc, dropped_ok=dok))

    def plant_pair(self):
        """Two plant steps in a row with different parameters, the second from the first's x_next, one tstep."""
        ts = self.tstep.clone()
        first = self.plant(self.p_true, "plant_true", self.px, ts)
        return first, self.plant(self.p_prior, "plant_prior", first.outs["x_next"], ts)

    def plant_then_solve(self):
        """The control loop's hand-over on two streams: the plant step's x_next and tstep are the solve's inputs."""
        ts = self.tstep.clone()
        first = self.plant(self.p_true, "plant_true", self.x0b, ts)
        return first, self.solve(first.outs["x_next"], ts)

    def solve_then_plant(self):
        """The other half of the loop: the solve's u0 is the plant step's input."""
        first = self.solve()
        return first, self.plant(self.p_true, "plant_true", self.x0b, self.tstep.clone(), u=first.outs["u0"])

    # ------------------------------------------------------------------ timing pass, delay, stream pairs
    def every_call(self):
        """One staged call of every ORDERED function, with the state it needs: what the timing pass runs."""
        plan = [("base", c) for c in (self.append, self.drop_oldest, self.drop_rows, self.refactor, self.mll, self.fit,
                                      self.love_root, self.fitc, self.reset, self.set_iterate, self.solve,
                                      self.get_solution, self.get_variance, self.predict, self.mean_grad,
                                      lambda: self.plant_pair()[0], self.informative, self.select, self.redundant,
                                      self.observe)]
        plan += [("love1", lambda: self.get_root(1)), ("fitc1", lambda: self.get_fitc(1)), ("fitc1", lambda: self.fitc_off(1))]
        return plan

    def time_calls(self):
        """Device time (events) and host time to return of every call, serially, after one untimed pass that loads
        the code objects and allocates the handle's first-use scratch.  Sets the delay."""
        torch = self.torch
        for timed in (False, True):
            for state, make in self.every_call():
                self.prepare(state)
                c = make()
                torch.cuda.synchronize()
                cur = torch.cuda.current_stream()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(cur)
                t0 = time.perf_counter()
                c.issue(cur.cuda_stream)
                t1 = time.perf_counter()
                e1.record(cur)
                e1.synchronize()
                if timed:
                    self.times[c.label] = dict(fn=c.fn, sync=c.sync, dev_ms=e0.elapsed_time(e1), host_ms=(t1 - t0) * 1e3)
        torch.cuda.synchronize()
        assert {t["fn"] for t in self.times.values()} == {f for f, (k, _) in TABLE.items() if k == ORDERED}
        self.worst_ms = max(max(t["dev_ms"], t["host_ms"]) for t in self.times.values() if not t["sync"])
        self.delay_ms = max(DELAY_FLOOR_MS, DELAY_MULT * self.worst_ms)
        self.delay_measured_ms = self.delay.measure(self.delay_ms)

    def report(self):
        lines = [f"{'call':<16}{'function':<30}{'device ms':>10}{'host ms':>10}  sync"]
        for label, t in self.times.items():
            lines.append(f"{label:<16}{t['fn']:<30}{t['dev_ms']:>10.3f}{t['host_ms']:>10.3f}  {'yes' if t['sync'] else ''}")
        lines.append(f"largest asynchronous time {self.worst_ms:.3f} ms; delay = max({DELAY_FLOOR_MS} ms, {DELAY_MULT} x it) = "
                     f"{self.delay_ms:.1f} ms asked for, {self.delay_measured_ms:.1f} ms measured "
                     f"({'torch.cuda._sleep' if self.delay.sleep else 'matmul chain'}, {self.delay.per_ms:.4g} units per ms)")
        return "\n".join(lines)

    def concurrent(self, a, b):
        """Whether work on b completes while a is held up: a tiny torch op on b behind a delay on a."""
        torch = self.torch
        t = torch.zeros(8, device=self.dev)
        torch.cuda.synchronize()
        self.delay.queue(a, self.delay_ms)
        end = torch.cuda.Event()
        end.record(a)
        with torch.cuda.stream(b):
            t.add_(1.0)
        eb = torch.cuda.Event()
        eb.record(b)
        eb.synchronize()
        ok = not end.query()
        torch.cuda.synchronize()
        return ok

    def pick_streams(self):
        """Two non-default streams that run side by side (the control: on streams that share a hardware queue a
        missing wait would be masked), and a stream that runs beside the default stream.  Up to 8 fresh pairs."""
        import pytest

        torch = self.torch
        for _ in range(8):
            a, b = torch.cuda.Stream(), torch.cuda.Stream()
            if self.concurrent(a, b):
                self.A, self.Bs = a, b
                break
        else:
            pytest.fail("no concurrent stream pair: of 8 fresh pairs none let a tiny op on B complete while the delay ran on A")
        null = torch.cuda.default_stream()
        assert null.cuda_stream == 0
        for b in [self.Bs] + [torch.cuda.Stream() for _ in range(7)]:
            if self.concurrent(null, b):
                self.Bnull = b
                return
        pytest.fail("no stream ran beside the default stream: 8 streams all waited for the delay queued on it")


# ------------------------------------------------------------------------------------------------ runs and checks
def collect(calls, hosts):
    import torch

    out = {}
    for c, host in zip(calls, hosts):
        for k, v in c.outs.items():
            out[f"{c.label}.{k}"] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        for k, v in (host or {}).items():
            out[f"{c.label}.{k}"] = np.asarray(v)
    return out


def run_serial(env, case, order, refusals=False):
    """The case's calls `order` (indices into make's tuple) on one stream with a synchronise after each.  With
    `refusals` a call the library refuses in this order counts as a result (its outputs stay unwritten)."""
    torch = env.torch
    env.prepare(case.state)
    calls = case.make(env)
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream().cuda_stream
    picked, hosts = [calls[i] for i in order], []
    for c in picked:
        try:
            hosts.append(c.issue(cur))
        except env._lib.GPMPCError:
            if not refusals:
                raise
            hosts.append(dict(refused=1))
        torch.cuda.synchronize()
    res = collect(picked, hosts)
    res.update(env.probe())
    return res


def run_streams(env, case):
    """Steps 1 to 7: stage, synchronise, delay on A, delay_end, first on A, second on B, eB; a third call goes back
    to A.  Returns the results and what conditions (a) and (b) saw."""
    torch = env.torch
    env.prepare(case.state)
    calls = case.make(env)
    first, second = calls[0], calls[1]
    sa = torch.cuda.default_stream() if case.first_null else env.A
    sb = env.Bnull if case.first_null else env.Bs
    torch.cuda.synchronize()
    env.delay.queue(sa, env.delay_ms)
    delay_end = torch.cuda.Event()
    delay_end.record(sa)
    hosts = [first.issue(sa.cuda_stream)]
    hosts.append(second.issue(sb.cuda_stream))
    done_at_return = delay_end.query()
    eB = torch.cuda.Event()
    eB.record(sb)
    for c in calls[2:]:
        hosts.append(c.issue(sa.cuda_stream))
    eB.synchronize()
    done_after_b = delay_end.query()
    torch.cuda.synchronize()
    res = collect(calls, hosts)
    res.update(env.probe())
    return res, dict(calls=len(calls), done_at_return=done_at_return, done_after_b=done_after_b, first_sync=first.sync,
                     second_sync=second.sync)


def differing(a, b):
    keys = sorted(set(a) & set(b))
    return [k for k in keys if a[k].shape != b[k].shape or bits(a[k]) != bits(b[k])] + sorted(set(a) ^ set(b))


def ordered(env, case):
    """Conditions (a), (b), (c) and the sensitivity of (c), reported together."""
    got, seen = run_streams(env, case)
    order = tuple(range(seen["calls"]))
    want = run_serial(env, case, order)
    other = {"swap": tuple(reversed(order)), "omit_first": order[1:], "omit_second": order[:1] + order[2:]}[case.sens]
    sens = run_serial(env, case, other, refusals=True)
    failures = []
    if not seen["first_sync"] and not seen["second_sync"] and seen["done_at_return"]:
        failures.append("(b) the delay had ended when `second` returned to the host: it showed nothing")
    if seen["second_sync"] and not seen["done_at_return"]:
        failures.append("(a) the synchronous `second` returned while the delay on the other stream still ran: it did not wait")
    if not seen["done_after_b"]:
        failures.append("(a) `second` completed on its stream while the delay ahead of `first` still ran: it did not wait")
    bad = differing(got, want)
    if bad:
        failures.append("(c) differs from the serial run in " + ", ".join(bad))
    common = [k for k in want if k in sens]
    if not [k for k in common if want[k].shape != sens[k].shape or bits(want[k]) != bits(sens[k])]:
        failures.append(f"the pair's results do not depend on the order ({case.sens} run is identical in {len(common)} arrays)")
    assert not failures, f"{case.id}: " + "; ".join(failures)
