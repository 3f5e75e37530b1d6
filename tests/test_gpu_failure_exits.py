"""The SQP kernel's in-loop failure exits on the MI355X, in every compiled variant of the helper-wave
protocol: the failure script of tests/failure_cases.py (its verdicts on the C++ restatement are pinned
by tests/test_failure_exits_cpu.py) against the restatement and against a twin handle of the same
launch shape that gets the clean inputs.

The exits (SqpKernel::run): obs outside the stage-0 box (A, before the loop), QP failure out of the IPM
(B+-: NaN mu / refused factorisation, through the status exchange of the multi-wave shapes), NaN
status at the residual test (C, D: a NaN in the stored iterate) and the IPM limit on every QP (E,
status 2).  A failed solve is a legal call whose result is a status code: the iterate is kept bit for
bit, u0 is its first input, the multipliers restart, the next solve runs untightened and recomputes
its first linearisation, and no other instance of the batch sees any of it.

The IPM iteration at which B+- are refused is printed beside the restatement's, not asserted: a
diverging IPM amplifies rounding.
"""

import numpy as np
import pytest

import failure_cases as fc
from helpers import lqr, problem, product_gps

pytestmark = pytest.mark.gpu

KEYS = ("u0", "status", "sqp_iter", "qp_iter", "res", "x", "u")
FAILED = (fc.A, fc.BP, fc.BM, fc.C, fc.D)
LAUNCHES = ((1, 0), (2, 0), (2, 1), (4, 0), (4, 1))
# one case per compiled variant: waves 1 / 2 / 4, segment solve off / on, split-lane IPM (H <= 31) or not; quad3d
VARIANTS = [(s, l) for s in fc.SHAPES if s[0] != "quad3d" for l in LAUNCHES] + [(fc.SHAPES[-1], None)]


def launch_id(launch):
    return "auto" if launch is None else f"w{launch[0]}s{launch[1]}"


def variant_id(v):
    return f"{fc.shape_id(v[0])}-{launch_id(v[1])}"


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not fc.cpu_ref_built():
        pytest.skip("oracle/lib/libcpuref.so not built (make -C oracle)")
    return torch


class GpuBackend:
    """A BatchSolver behind the three calls ``failure_cases.drive`` makes; every solve's outputs on the host."""

    def __init__(self, torch, shape, opts=fc.OPTS, launch=None, batch=fc.B, **tuning):
        from gpmpc.solver import BatchSolver

        name, N, H = shape
        self.torch = torch
        self.spec, data, hyp = problem(name, N)
        gs = self.gs = BatchSolver(self.spec, H, batch, **opts.kw())
        gs.set_gps(product_gps(data, hyp))
        gs.set_tightening(True, 0.95, *lqr(self.spec))
        if launch is not None:
            gs.set_launch(launch[0])
            gs.set_tuning(seg=launch[1])
        if tuning:
            gs.set_tuning(**tuning)
        self.stats = torch.zeros(batch, gs.STATS_SLOTS, dtype=torch.int64, device="cuda")
        gs.set_stats(self.stats)
        gs.set_cost_output(True)
        gs.reset(reset_iterate=True)
        if launch is not None:   # the variant this case is about is the one that runs
            info = gs.launch_info()
            segments = 1 if launch[1] == 0 or launch[0] == 1 else (3 if launch[0] == 4 else 2)
            assert info["waves"] == launch[0] and info["segments"] == segments, info

    def solve(self, obs, tstep):
        torch, gs = self.torch, self.gs
        gs.solve(torch.tensor(obs, device="cuda"), torch.tensor(tstep, dtype=torch.int32, device="cuda"))
        x, u, t = gs.solution()
        out = dict(x=x, u=u, tight=t, u0=gs.u0, status=gs.status, sqp_iter=gs.sqp_iter, qp_iter=gs.qp_iter, res=gs.res,
                   cost=gs.stage_cost, stats=self.stats)
        return {k: v.cpu().numpy().copy() for k, v in out.items()}

    def iterate(self):
        x, u, _ = self.gs.solution()
        return x.cpu().numpy().copy(), u.cpu().numpy().copy()

    def set_iterate(self, x, u):
        self.gs.set_iterate(self.torch.tensor(x), self.torch.tensor(u))


def run_pair(torch, shape, launch, plant="u0", opts=fc.OPTS):
    """(planted handle's five solves, twin's, restatement's planted run)."""
    _, obs, phase = fc.clean_run(shape, opts)
    got = fc.drive(GpuBackend(torch, shape, opts, launch), problem(shape[0], shape[1])[0], obs, phase, plant, opts.b_state)
    twin = fc.drive(GpuBackend(torch, shape, opts, launch), problem(shape[0], shape[1])[0], obs, phase)
    return got, twin, fc.planted_run(shape, plant, opts)


def assert_bits(a, b, what, rows=slice(None), keys=KEYS):
    for k in keys:
        np.testing.assert_array_equal(a[k][rows], b[k][rows], err_msg=f"{what}: {k}")


def assert_kept(o, rows, what):
    """Rows of a failed solve: iterate and first input kept bit for bit (NaN included), cost row NaN."""
    xb, ub = o["before"]
    np.testing.assert_array_equal(o["x"][rows], xb[rows], err_msg=what)
    np.testing.assert_array_equal(o["u"][rows], ub[rows], err_msg=what)
    np.testing.assert_array_equal(o["u0"][rows], ub[rows, 0], err_msg=what)
    assert np.isnan(o["cost"][rows]).all(), what


def close(a, b):
    """max |a - b| / (1 + max |b|)"""
    return float(np.abs(a - b).max() / (1.0 + np.abs(b).max()))


@pytest.mark.parametrize("variant", VARIANTS, ids=variant_id)
def test_failing_solves_in_every_variant(variant):
    torch = _torch()
    shape, launch = variant
    got, twin, ref = run_pair(torch, shape, launch)
    at = variant_id(variant)
    clean = list(fc.CLEAN)
    f, n, h = got[fc.FAILING], got[fc.NEXT], got[fc.HEALED]
    for b, name in ((fc.BP, "B+"), (fc.BM, "B-")):
        print(f"{at} {name}: IPM stops at {int(f['qp_iter'][b])} (restatement {int(ref[fc.FAILING]['qp_iter'][b])})")
    # status and SQP iterations: the restatement's, every instance, every solve
    for s in range(5):
        np.testing.assert_array_equal(got[s]["status"], ref[s]["status"], err_msg=f"{at} solve {s}")
        np.testing.assert_array_equal(got[s]["sqp_iter"], ref[s]["sqp_iter"], err_msg=f"{at} solve {s}")
        # independence: the clean instances are the twin's, bit for bit
        assert_bits(got[s], twin[s], f"{at} solve {s}, clean instances vs twin", rows=clean)
        # bookkeeping: one status count per solve
        before = got[s - 1]["stats"] if s else np.zeros_like(got[s]["stats"])
        want = before[:, 2:7].copy()
        want[np.arange(fc.B), got[s]["status"]] += 1
        np.testing.assert_array_equal(got[s]["stats"][:, 2:7], want, err_msg=f"{at} solve {s}: status counts")
    assert [int(v) for v in f["status"][list(FAILED)]] == [4, 4, 4, 1, 1], f["status"]
    assert_kept(f, list(FAILED), at)
    assert_kept(dict(n, before=(f["x"], f["u"])), [fc.C, fc.D], at)   # C and D stay non-finite until the iterate is set
    assert np.isnan(f["x"][fc.D]).sum() + np.isnan(f["u"][fc.D]).sum() == 1 and np.isnan(f["u"][fc.C]).sum() == 1
    assert np.isfinite(f["cost"][clean]).all()
    # the solve after a failed one runs untightened and recomputes its first linearisation (stats slot 9:
    # sqp_iter + 1 linearisations, against sqp_iter on a cache hit)
    lin = n["stats"][:, 9] - f["stats"][:, 9]
    for b in FAILED:
        assert not n["tight"][b].any(), (at, b)
        assert lin[b] == n["sqp_iter"][b] + 1, (at, b, lin[b], n["sqp_iter"][b])
    for b in clean:
        assert n["tight"][b].any(), (at, b)
        assert lin[b] == n["sqp_iter"][b], (at, b, lin[b], n["sqp_iter"][b])
    # recovery: A and B+- at the next solve, everyone once the iterate is finite again
    assert [int(v) for v in n["status"][list(FAILED)]] == [0, 0, 0, 1, 1], n["status"]
    assert (h["status"] == 0).all(), h["status"]
    for o, r, rows in ((n, ref[fc.NEXT], [b for b in range(fc.B) if b not in (fc.C, fc.D)]), (h, ref[fc.HEALED], list(range(fc.B)))):
        assert np.isfinite(o["x"][rows]).all() and np.isfinite(o["u"][rows]).all() and np.isfinite(o["u0"][rows]).all()
        ex, eu = close(o["x"][rows], r["x"][rows]), close(o["u"][rows], r["u"][rows])
        print(f"{at}: recovered solve vs restatement x {ex:.2e} u {eu:.2e}")
        assert ex <= 1e-5 and eu <= 1e-5, (at, ex, eu)


D_VARIANTS = [(fc.SHAPES[0], (1, 0)), (fc.SHAPES[0], (4, 1)), (fc.SHAPES[-1], None)]


@pytest.mark.parametrize("plant", fc.PLANTS)
@pytest.mark.parametrize("variant", D_VARIANTS, ids=variant_id)
def test_nan_in_a_converged_iterate_is_status_1(variant, plant):
    """Case D: the repeated solve with a NaN in u_0, u_{H-1} or x_H of the stored iterate is GPMPC_NAN at
    SQP iteration 0, before any QP: never a success (0, 2) with a NaN first input, nor the QP's failure
    (4: what the residual norms gave when they dropped the NaN and handed it to the IPM)."""
    torch = _torch()
    shape, launch = variant
    _, obs, phase = fc.clean_run(shape)
    got = fc.drive(GpuBackend(torch, shape, fc.OPTS, launch), problem(shape[0], shape[1])[0], obs, phase, plant)
    f = got[fc.FAILING]
    print(f"{variant_id(variant)} {plant}: status {f['status'].tolist()} sqp_iter {f['sqp_iter'].tolist()} qp_iter {f['qp_iter'].tolist()}")
    assert f["status"][fc.D] == 1 and f["sqp_iter"][fc.D] == 0 and f["qp_iter"][fc.D] == 0, f["status"]
    assert f["status"][fc.C] == 1
    assert_kept(f, [fc.C, fc.D], plant)
    np.testing.assert_array_equal(f["status"], fc.planted_run(shape, plant)[fc.FAILING]["status"])
    assert (got[fc.HEALED]["status"] == 0).all()


@pytest.mark.parametrize("launch", [(1, 0), (4, 1)], ids=launch_id)
def test_every_qp_at_the_ipm_limit(launch):
    """Case E (cartpole H = 32, qp_max_iter 50, max_iter 5): B+- end every QP at the IPM limit and the
    solve at the SQP limit -- status 2, 250 IPM iterations, a stored (finite) iterate."""
    torch = _torch()
    got, twin, ref = run_pair(torch, fc.CASE_E_SHAPE, launch, opts=fc.OPTS_E)
    f = got[fc.FAILING]
    others = [b for b in range(fc.B) if b not in (fc.BP, fc.BM)]
    for s in range(5):
        # (B+- leave the failing solve at the SQP limit of 5, and the restatement's own next solves of them end
        # at or on that limit: their later statuses hang on rounding and are held to {0, 2} only)
        rows = list(range(fc.B)) if s <= fc.FAILING else others
        np.testing.assert_array_equal(got[s]["status"][rows], ref[s]["status"][rows], err_msg=f"solve {s}")
        np.testing.assert_array_equal(got[s]["sqp_iter"][rows], ref[s]["sqp_iter"][rows], err_msg=f"solve {s}")
        assert_bits(got[s], twin[s], f"solve {s}, clean instances vs twin", rows=list(fc.CLEAN))
    for b in (fc.BP, fc.BM):
        assert (f["status"][b], f["sqp_iter"][b], f["qp_iter"][b]) == (2, 5, 250)
        assert np.isfinite(f["x"][b]).all() and np.isfinite(f["u"][b]).all() and np.isfinite(f["cost"][b]).all()
    assert (got[fc.HEALED]["status"][others] == 0).all() and np.isin(got[fc.HEALED]["status"], (0, 2)).all()


# ---------------------------------------------------------------- the dispatch paths, same contract
def tiled(shape, n, shift=0):
    """The clean observations and phases of a shape, repeated to a batch of n: instance i plays the part
    i % 8 of the script on the observations of instance (i + shift) % 8."""
    _, obs, phase = fc.clean_run(shape)
    idx = (np.arange(n) + shift) % fc.B
    return np.ascontiguousarray(obs[:, idx]), np.ascontiguousarray(phase[idx])


def n_cu(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def test_order_by_cost_at_a_small_batch():
    """set_tuning(order=2) ranks even a batch that fits one round of workgroups: against order 0, every
    output of the failure script is bit-identical."""
    torch = _torch()
    shape = fc.SHAPES[0]
    _, obs, phase = fc.clean_run(shape)
    runs = [fc.drive(GpuBackend(torch, shape, order=order), problem(shape[0], shape[1])[0], obs, phase, "u0") for order in (2, 0)]
    assert (runs[0][fc.FAILING]["status"][list(FAILED)] != 0).all()
    for s in range(5):
        assert_bits(runs[0][s], runs[1][s], f"solve {s}", keys=KEYS + ("tight", "cost"))


def test_two_rounds_of_workgroups():
    """quad3d (one instance per CU), B = CUs + 5: the launch is cost-ordered over two rounds; failures in
    both halves of the ranking (the cheapest warm-up solves, which the ranking leaves to the second
    round, are those of instance 6's observations: the shift gives them the part of B+).  Order 1
    against 0: bit-identical."""
    torch = _torch()
    shape = fc.SHAPES[-1]
    n = n_cu(torch) + 5
    obs, phase = tiled(shape, n, shift=fc.CLEAN[1] - fc.BP)
    spec = problem(shape[0], shape[1])[0]
    runs = [fc.drive(GpuBackend(torch, shape, batch=n, order=order), spec, obs, phase, "u0") for order in (1, 0)]
    f = runs[0][fc.FAILING]
    cost = 5 * runs[0][1]["sqp_iter"] + 2 * runs[0][1]["qp_iter"]        # what ranked the failing solve (kCostLin = 5)
    rank = np.lexsort((np.arange(n), -cost))
    first = set(rank[: n_cu(torch)].tolist())
    failed = np.flatnonzero(np.isin(f["status"], (1, 4)))
    assert len(failed) == sum(len(fc.pattern(b, n)) for b in FAILED)
    assert any(b in first for b in failed) and any(b not in first for b in failed)
    for s in range(5):
        assert_bits(runs[0][s], runs[1][s], f"solve {s}", keys=KEYS + ("tight", "cost"))


def test_tail_boost():
    """quad2d H = 5, B = 2 CUs + 8 (one wave per instance in one round), tail = 4: the four costliest
    instances of the previous solve run as two-wave segment solves.  B+- fail twice in a row, so the
    second time they are the boosted ones (a failed QP costs more IPM iterations than any clean solve)
    while A, C and D fail unboosted.  Against tail = 0: the instances not boosted so far are
    bit-identical; a boosted one runs another kernel (results agree to rounding,
    tests/test_gpu_launch.py), so its status, SQP iterations and kept state are identical and what it
    solves agrees to 1e-6 (1 + |.|).  (The first failing solve boosts the C instances -- the costliest
    of the warm-up -- so the NaN exit runs boosted too.)"""
    torch = _torch()
    shape = fc.SHAPES[0]
    n = 2 * n_cu(torch) + 8
    obs, phase = tiled(shape, n)
    spec = problem(shape[0], shape[1])[0]
    runs = []
    for tail in (4, 0):
        be = GpuBackend(torch, shape, batch=n, tail=tail)
        info = be.gs.launch_info()
        assert info["waves"] == 1 and info["tail_boost"] == (tail != 0), info
        out = [be.solve(obs[0], phase), be.solve(obs[1], phase + 1)]
        x, u = fc.plant_nan(*be.iterate(), "u0")
        be.set_iterate(x, u)
        out.append(be.solve(*fc.failing_inputs(spec, obs[1], obs[2], phase + 2)))
        x, u = be.iterate()
        out.append(dict(be.solve(*fc.failing_inputs(spec, obs[2], obs[3], phase + 3)), before=(x, u)))
        out.append(be.solve(obs[4], phase + 4))
        runs.append(out)
    on, off = runs
    ever = np.zeros(n, dtype=bool)     # boosted at this solve or before: no longer comparable bit for bit
    for s in range(5):
        prev = on[s - 1] if s else {k: np.zeros(n, dtype=np.int64) for k in ("sqp_iter", "qp_iter")}   # (after a reset: no cost yet)
        cost = 3 * prev["sqp_iter"] + 2 * prev["qp_iter"]                 # StateDev::cost of a quad2d solve (kCostLin = 3)
        boosted = np.lexsort((np.arange(n), -cost))[:4]                   # decreasing cost, ties by instance id
        fresh = boosted[~ever[boosted]]
        ever[boosted] = True
        rest = np.flatnonzero(~ever)
        assert_bits(on[s], off[s], f"solve {s}, unboosted", rows=rest, keys=KEYS + ("tight", "cost"))
        assert_bits(on[s], off[s], f"solve {s}, boosted", rows=boosted, keys=("status", "sqp_iter"))
        ok = boosted[np.isin(off[s]["status"][boosted], (0, 2))]
        if len(ok):
            assert close(on[s]["x"][ok], off[s]["x"][ok]) <= 1e-6 and close(on[s]["u"][ok], off[s]["u"][ok]) <= 1e-6
        if s == 3:
            bpm = np.concatenate([fc.pattern(fc.BP, n), fc.pattern(fc.BM, n)])
            assert np.isin(boosted, bpm).all(), boosted
            assert (on[s]["status"][boosted] == 4).all() and (on[s]["status"][fc.pattern(fc.A, n)] == 4).all()
            assert (on[s]["status"][fc.pattern(fc.C, n)] == 1).all()
            assert_kept(on[s], boosted, "boosted, failed")
            assert len(fresh) >= 1
            assert_bits(on[s], off[s], "boosted, failed", rows=fresh, keys=("u0", "x", "u"))
    assert np.isin(on[4]["status"][np.setdiff1d(np.arange(n), np.concatenate([fc.pattern(fc.C, n), fc.pattern(fc.D, n)]))], (0, 2)).all()


def test_shift_after_an_in_loop_failure():
    """shift = 1: the solve after an in-loop failure (B+-, and the NaN exits) is not shifted -- for those
    instances bit-identical to shift = 0 -- while the clean instances' ordinary + 1 step is."""
    torch = _torch()
    shape = fc.SHAPES[0]
    _, obs, phase = fc.clean_run(shape)
    spec = problem(shape[0], shape[1])[0]
    runs = []
    for shift in (1, 0):
        be = GpuBackend(torch, shape, shift=shift)
        out = [be.solve(obs[0], phase)]
        be.set_iterate(*fc.plant_nan(*be.iterate(), "u0"))      # (an explicit iterate is not shifted either)
        out.append(be.solve(*fc.failing_inputs(spec, obs[0], obs[1], phase + 1)))
        out.append(be.solve(obs[2], phase + 2))
        runs.append(out)
    on, off = runs
    keys = KEYS + ("tight",)
    assert_bits(on[0], off[0], "first solve", keys=keys)
    assert_bits(on[1], off[1], "the failing solve, after set_iterate", keys=keys)
    assert [int(v) for v in on[1]["status"][list(FAILED)]] == [4, 4, 4, 1, 1], on[1]["status"]
    assert_bits(on[2], off[2], "the solve after a failed solve", rows=list(FAILED), keys=keys)
    assert np.isin(on[2]["status"][list(fc.CLEAN)], (0, 2)).all() and np.isin(off[2]["status"][list(fc.CLEAN)], (0, 2)).all()
    for b in fc.CLEAN:
        assert not np.array_equal(on[2]["x"][b], off[2]["x"][b]), f"instance {b}: an ordinary + 1 step was not shifted"
