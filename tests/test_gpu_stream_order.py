"""Cross-stream ordering of every stream-taking call of the C ABI on the MI355X (include/gpmpc_mi355x.h, "Streams").

Each case queues `first` on stream A behind a delay and `second` on stream B through the C ABI and checks
stream_order_util.ordered's conditions: (a) B's work completes only after the delay, (b) the delay was still running
when `second` returned, (c) every output and the handle's state afterwards are bit-identical to the two calls made
serially, and the serial run in the other order (or without one call) differs, so that (c) can fail.  quad2d, H = 5,
B = 8, 28 rows per GP with room for 64, sf2 = 1, sn2 = 1e-3.

SECOND: every ordered call as `second` behind an asynchronous writer of what it reads or writes (a refactor of GP 0
at a new lengthscale for the GP state, gpmpc_solve or gpmpc_set_iterate for the iterate; the LOVE root and the FITC
mean are written by their synchronous builders only).  FIRST: every ordered call as the delayed `first` before a
conflicting asynchronous writer.  Then the default stream as A, a chain A -> B -> A, and gpmpc_get_solution on B
behind a step that uses the handle's side stream, with no synchronise between.

Against the library before gpmpc_gp_predict, gpmpc_gp_mean_grad and gpmpc_plant_step joined the rule, 13 of the 55
tests failed, each on (a) and on (c) (the chain on (c) alone), and no other: the ten cases with predict or mean_grad
in them (second-refactor-predict, second-refactor-mean_grad, first-predict-append, first-mean_grad-append,
first-predict-drop_rows, first-append-predict, first-append-mean_grad, first-drop_rows-predict, null-append-predict,
chain-append-refactor-predict) and the three with plant_step (plant-true-prior, where the first launch integrated
with the second call's parameters, second-solve-plant, first-plant-solve).  Against a build whose order_after_last
never waits, 48 fail: every test but the five whose `first` is synchronous (the host has then drained A before
`second` is issued, so those five can only show the data).
"""

import pytest

import stream_order_util as SO
from stream_order_util import Case

pytestmark = pytest.mark.gpu

SECOND = [
    Case("second-refactor-append", lambda e: (e.refactor(), e.append())),
    Case("second-refactor-drop_oldest", lambda e: (e.refactor(), e.drop_oldest())),
    Case("second-refactor-drop_rows", lambda e: (e.refactor(), e.drop_rows())),
    Case("second-refactor-refactor", lambda e: (e.refactor(), e.refactor(0, SO.ELL_NEWER))),
    Case("second-refactor-mll", lambda e: (e.refactor(), e.mll())),
    Case("second-refactor-fit", lambda e: (e.refactor(), e.fit())),
    # the root depends on the refactor through the lengthscale; afterwards a refactor is refused: left out instead
    Case("second-refactor-love_root", lambda e: (e.refactor(), e.love_root()), sens="omit_first"),
    Case("second-refactor-fitc", lambda e: (e.refactor(), e.fitc()), sens="omit_first"),   # (as for the root)
    # the removal queues nothing and touches GP 1's mean only: what depends on the pair's order is the wait alone
    Case("second-refactor-fitc_off", lambda e: (e.refactor(), e.fitc_off(1)), state="fitc1", sens="omit_first"),
    Case("second-refactor-predict", lambda e: (e.refactor(), e.predict())),
    Case("second-refactor-mean_grad", lambda e: (e.refactor(), e.mean_grad())),
    Case("second-refactor-informative", lambda e: (e.refactor(), e.informative())),
    Case("second-refactor-select", lambda e: (e.refactor(), e.select())),
    Case("second-refactor-redundant", lambda e: (e.refactor(), e.redundant())),
    Case("second-refactor-observe", lambda e: (e.refactor(), e.observe())),
    Case("second-refactor-solve", lambda e: (e.refactor(), e.solve())),
    Case("second-love_root-get_root", lambda e: (e.love_root(), e.get_root(0))),   # (before the root: the copy is refused)
    Case("second-fitc-get_fitc", lambda e: (e.fitc(), e.get_fitc(0))),
    Case("second-solve-get_solution", lambda e: (e.solve(), e.get_solution())),
    Case("second-solve-get_variance", lambda e: (e.solve(), e.get_variance())),
    Case("second-set_iterate-solve", lambda e: (e.set_iterate(), e.solve())),
    Case("second-solve-set_iterate", lambda e: (e.solve(), e.set_iterate())),
    Case("second-solve-reset", lambda e: (e.solve(), e.reset())),
    Case("plant-true-prior", lambda e: e.plant_pair()),
    Case("second-solve-plant", lambda e: e.solve_then_plant()),
]

FIRST = [
    Case("first-predict-append", lambda e: (e.predict(), e.append())),
    Case("first-mean_grad-append", lambda e: (e.mean_grad(), e.append())),
    Case("first-predict-drop_rows", lambda e: (e.predict(), e.drop_rows())),
    Case("first-append-predict", lambda e: (e.append(), e.predict())),
    Case("first-append-mean_grad", lambda e: (e.append(), e.mean_grad())),
    Case("first-drop_rows-predict", lambda e: (e.drop_rows(), e.predict())),
    Case("first-append-solve", lambda e: (e.append(), e.solve())),
    Case("first-observe-solve", lambda e: (e.observe(), e.solve())),
    Case("first-append-refactor", lambda e: (e.append(), e.refactor())),
    Case("first-drop_oldest-append", lambda e: (e.drop_oldest(), e.append())),
    Case("first-drop_rows-append", lambda e: (e.drop_rows(), e.append())),
    Case("first-mll-refactor", lambda e: (e.mll(), e.refactor())),
    Case("first-fit-refactor", lambda e: (e.fit(), e.refactor())),
    Case("first-love_root-solve", lambda e: (e.love_root(), e.solve())),
    # nothing asynchronous writes the root: the solve is the writer of the list that reads it too
    Case("first-get_root-solve", lambda e: (e.get_root(1), e.solve()), state="love1", sens="omit_second"),
    Case("first-fitc-fitc_off", lambda e: (e.fitc(), e.fitc_off(0))),
    Case("first-get_fitc-fitc_off", lambda e: (e.get_fitc(1), e.fitc_off(1)), state="fitc1"),
    # the other order is refused (an append under a FITC mean): the append is left out instead
    Case("first-fitc_off-append", lambda e: (e.fitc_off(1), e.append(1)), state="fitc1", sens="omit_second"),
    Case("first-reset-solve", lambda e: (e.reset(), e.solve())),
    Case("first-get_solution-solve", lambda e: (e.get_solution(), e.solve())),
    Case("first-get_variance-solve", lambda e: (e.get_variance(), e.solve())),
    Case("first-informative-refactor", lambda e: (e.informative(), e.refactor())),
    Case("first-select-refactor", lambda e: (e.select(), e.refactor())),
    Case("first-redundant-drop_rows", lambda e: (e.redundant(), e.drop_rows())),
    Case("first-plant-solve", lambda e: e.plant_then_solve()),   # (the plant step's deferred record, made up by the solve)
]

OTHER = [
    Case("null-append-predict", lambda e: (e.append(), e.predict()), first_null=True),
    Case("chain-append-refactor-predict", lambda e: (e.append(), e.refactor(), e.predict())),
]

CASES = SECOND + FIRST + OTHER


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = SO.Env()
    e.time_calls()
    e.pick_streams()
    return e


def test_call_times_and_the_delay(env):
    """The serial times of every ordered call and the delay sized from them (printed: run with -s)."""
    print("\n" + env.report())
    assert env.delay_ms >= SO.DELAY_MULT * env.worst_ms and env.delay_ms <= SO.DELAY_CAP_MS
    # the calibration holds: the delay op lasts about what was asked for (clocks move: half of it still leaves
    # DELAY_MULT / 2 times the slowest call)
    assert 0.5 * env.delay_ms <= env.delay_measured_ms <= 2 * SO.DELAY_CAP_MS, (env.delay_ms, env.delay_measured_ms)
    assert env.A.cuda_stream != 0 and env.Bs.cuda_stream != 0 and env.A.cuda_stream != env.Bs.cuda_stream


def test_the_cases_cover_every_ordered_call_in_both_positions(env):
    staged = {c.id: c.make(env) for c in SECOND + FIRST}   # (staging calls nothing of the library)
    firsts, seconds = {calls[0].fn for calls in staged.values()}, {calls[1].fn for calls in staged.values()}
    ordered = {n for n, (k, _) in SO.TABLE.items() if k == SO.ORDERED}
    assert ordered - firsts == set() and ordered - seconds == set(), (ordered - firsts, ordered - seconds)
    # behind a writer: the first call of a SECOND case is asynchronous, or the synchronous builder of what is read
    for c in SECOND:
        first = staged[c.id][0]
        assert not first.sync or first.fn in ("gpmpc_gp_love_root", "gpmpc_gp_fitc"), c.id
    # before a writer: the second call of a FIRST case is asynchronous
    for c in FIRST:
        assert not staged[c.id][1].sync, c.id


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_ordered(env, case):
    SO.ordered(env, case)


def _side_stream_step(env, s, batch, x0, ts, steps, synchronise):
    """`steps` solves of `batch` instances on A from a reset, then gpmpc_get_solution on B: with a synchronise
    before it, or with nothing but the handle's event between the two streams."""
    import torch

    nx, nu = s.spec.nx, s.spec.nu
    x = torch.full((batch, s.H + 1, nx), float("nan"), dtype=torch.float64, device="cuda")
    u = torch.full((batch, s.H, nu), float("nan"), dtype=torch.float64, device="cuda")
    t = torch.full((batch, s.H + 1, nx + nu), float("nan"), dtype=torch.float64, device="cuda")
    u0 = torch.empty(batch, nu, dtype=torch.float64, device="cuda")
    st = torch.empty(batch, dtype=torch.int32, device="cuda")
    s.reset(reset_iterate=True)
    torch.cuda.synchronize()
    a, b = env.A.cuda_stream, env.Bs.cuda_stream
    for k in range(steps):
        tk = ts + k
        torch.cuda.synchronize()   # (tk is staged on the current stream)
        env.check(s.lib.gpmpc_solve(s._h, batch, x0.data_ptr(), tk.data_ptr(), u0.data_ptr(), st.data_ptr(), None, None,
                                    None, a))
        if synchronise or k < steps - 1:
            torch.cuda.synchronize()
    env.check(s.lib.gpmpc_get_solution(s._h, batch, x.data_ptr(), u.data_ptr(), t.data_ptr(), b))
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in (x, u, t, u0, st)]


def test_get_solution_on_another_stream_behind_a_side_stream_step(env):
    """A step that forks to the handle's side stream and joins back (the overlapped halves at quad2d H = 30, n = 200,
    B = 1100, the shape of test_overlapped_step_is_bit_exact; and a tail-boosted step, one wave per instance in one
    round, its batch read from gpmpc_get_launch_info), then gpmpc_get_solution on stream B with no synchronise: the
    solve is the delay.  Data only, against the same run with a synchronise before the copy."""
    import ctypes

    import numpy as np
    import torch

    from gpmpc.solver import BatchSolver
    from helpers import initial_states, lqr, problem, product_gps

    Bmax = 1100
    spec, data, hyp = problem("quad2d", 200)
    s = BatchSolver(spec, 30, Bmax)
    s.set_gps(product_gps(data, hyp))
    s.set_tightening(True, 0.95, *lqr(spec))
    x0, ph = initial_states(spec, spec.reference_trajectory(), Bmax)
    x0, ts = torch.tensor(x0, device="cuda"), torch.tensor(ph, dtype=torch.int32, device="cuda")

    def info(batch):
        w, o = ctypes.c_int32(), ctypes.c_int32()
        env.check(s.lib.gpmpc_get_launch_info(s._h, batch, ctypes.byref(w), ctypes.byref(o)))
        return w.value, o.value

    assert info(Bmax)[1] == 1
    tail = next((b for b in range(2, Bmax) if info(b) == (1, 2)), None)
    assert tail is not None, "no batch up to 1100 runs the tail boost"
    for batch, steps, what in ((Bmax, 2, "overlapped halves"), (tail, 2, f"tail boost at B = {tail}")):
        want = _side_stream_step(env, s, batch, x0, ts, steps, synchronise=True)
        got = _side_stream_step(env, s, batch, x0, ts, steps, synchronise=False)
        assert not np.isnan(want[0]).any() and not np.array_equal(want[0], np.zeros_like(want[0])), what
        for name, a, b in zip(("x", "u", "tight", "u0", "status"), got, want):
            assert SO.bits(a) == SO.bits(b), f"{what}: {name} differs from the synchronised run"
