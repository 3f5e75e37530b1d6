"""The constrained case table (tests/constrained_cases.py) on the two CPU references and the KKT
certificate (tests/kkt_ref.py): what makes the table trustworthy before a GPU sees it.

Per case, instance and step, at KKT tolerance 1e-9 (QP 1e-11): the numpy oracle (dense KKT IPM) and
the C++ restatement (Riccati IPM) both succeed in the same number of SQP iterations and agree to
1e-6 (1 + |.|); the declared kinds of active bound occur; every bound within 1e-6 carries a
multiplier >= 1e-6 (strict complementarity, which makes 1e-6 agreement in x a fair demand); and the
certificate -- which uses no solver's multipliers -- finds the oracle's solution stationary to
2 sqrt(n) tol, n = H (nx + nu) (an inf-norm stationarity <= tol is a 2-norm <= sqrt(n) tol).
"""

import numpy as np
import pytest

import constrained_cases as cc
import kkt_ref
from helpers import O, lqr, oracle_gps

KINDS = ("xl", "xu", "ul", "uu")


def cpp_run(case, tol=cc.TOL, qp_tol=cc.QP_TOL, steps=None):
    if not cc.cpu_ref_built():
        pytest.skip("oracle/lib/libcpuref.so not built (make -C oracle)")
    return cc.cpp_run(case.id, tol, qp_tol, 25, steps)


def active_kinds(case, spec, o):
    """{kind: (n,) bool} of the bounds within 1e-6 at the oracle's solution ``o``."""
    al, ah = kkt_ref.active_sets(o.x, o.u, *o.bounds)
    isx = kkt_ref.is_state(spec.nx, spec.nu, case.H)
    return {"xl": al & isx, "xu": ah & isx, "ul": al & ~isx, "uu": ah & ~isx}


def check_case(case, tol=cc.TOL, qp_tol=cc.QP_TOL):
    """Everything this module asserts per case; returns facts for the assertions over all cases."""
    spec, data, hyp = cc.case_spec(case)
    sd = spec.to_dict()
    dyn = O.Dynamics(sd, oracle_gps(data, hyp))
    traj = spec.reference_trajectory()
    nx, H = spec.nx, case.H
    n = H * (spec.nx + spec.nu)
    isx = kkt_ref.is_state(spec.nx, spec.nu, H)
    orun, crun = cc.oracle_run(case.id, tol, qp_tol), cpp_run(case, tol, qp_tol)
    seen = [set() for _ in case.instances]
    facts = dict(kinds=set(), tight_state=False, wrap=False)
    for s, (row, (cst, cit, cx, cu)) in enumerate(zip(orun, crun)):
        for b, (inst, o) in enumerate(zip(case.instances, row)):
            at = (case.id, inst.label, s)
            assert o.status == cst[b] == 0, (at, o.status, cst[b])
            assert o.sqp_iter == cit[b], (at, o.sqp_iter, cit[b])
            weak_step = s in inst.oracle_weak_steps
            if not weak_step:
                np.testing.assert_allclose(cx[b], o.x, rtol=0, atol=1e-6 * (1 + np.abs(o.x).max()), err_msg=str(at))
                np.testing.assert_allclose(cu[b], o.u, rtol=0, atol=1e-6 * (1 + np.abs(o.u).max()), err_msg=str(at))
            act = active_kinds(case, spec, o)
            for kind in KINDS:
                if act[kind].any():
                    seen[b].add(kind)
                    mult = (o.ll if kind[1] == "l" else o.lu)[act[kind]]
                    assert mult.min() >= 1e-6, (at, kind, mult.min())
            # a state bound that is active while its tightening is non-zero (d layout -> stage, state)
            t_state = np.abs(o.sc[:nx, 1:].T)                                    # (H, nx), stages 1..H
            idx = np.flatnonzero((act["xl"] | act["xu"])[isx])
            facts["tight_state"] |= bool(len(idx) and t_state.reshape(-1)[idx].max() > 1e-4)
            facts["wrap"] |= inst.phase0 + s + H >= traj.shape[1]
            win = O.reference_window(traj, inst.phase0 + s, H)
            cert = kkt_ref.certificate(sd, dyn, o.x, o.u, *o.bounds, win, x0=o.x0)
            if weak_step:
                # the declared exception is checked, not assumed: the oracle holds a multiplier >= 1e-6 on
                # a bound it left between 1e-6 and 1e-5 away, and misses the certificate for that reason
                # alone -- the restatement's solution of the same step takes the certificate instead, and
                # stays within 1e-5 (1 + |.|) of the oracle's
                w = kkt_ref.pack(o.x, o.u)
                slack = np.minimum(w - kkt_ref.pack(o.bounds[0], o.bounds[2]), kkt_ref.pack(o.bounds[1], o.bounds[3]) - w)
                weak = (slack > 1e-6) & (slack < 1e-5) & (np.maximum(o.ll, o.lu) >= 1e-6)
                assert weak.sum() == 1 and cert.stat > 2 * np.sqrt(n) * tol, (at, weak.sum(), cert.stat)
                cert = kkt_ref.certificate(sd, dyn, cx[b], cu[b], *o.bounds, win, x0=o.x0)
                assert np.abs(cx[b] - o.x).max() <= 1e-5 * (1 + np.abs(o.x).max()), at
                assert np.abs(cu[b] - o.u).max() <= 1e-5 * (1 + np.abs(o.u).max()), at
            assert cert.eq <= tol and cert.viol <= tol, (at, cert.eq, cert.viol)
            assert cert.stat <= 2 * np.sqrt(n) * tol, (at, cert.stat, 2 * np.sqrt(n) * tol)
    for inst, got in zip(case.instances, seen):
        assert inst.kinds <= got, (case.id, inst.label, sorted(inst.kinds), sorted(got))
        if not inst.kinds:
            assert not got, (case.id, inst.label, "the nominal instance met a bound", sorted(got))
        facts["kinds"] |= got
    return facts


@pytest.fixture(scope="module")
def facts():
    return {}


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.id)
def test_case_on_both_cpu_references(case, facts):
    assert case.N <= 60 and case.H <= 12 and case.B <= 8 and case.steps <= 4
    assert case.instances[-1].kinds == frozenset() and any(i.kinds for i in case.instances)
    facts[case.id] = check_case(case)


def test_table_covers_every_kind_tightening_and_wrap(facts):
    """Over all cases: the four kinds of active bound, a state bound active under a non-zero
    tightening, and a reference window that wraps (phase0 + step + H >= traj_len)."""
    all_facts = [facts[c.id] if c.id in facts else check_case(c) for c in cc.CASES]
    assert set().union(*(f["kinds"] for f in all_facts)) == set(KINDS)
    assert any(f["tight_state"] for f in all_facts)
    assert any(f["wrap"] for f in all_facts)


def test_certificate_reacts_to_small_perturbations():
    """The certificate is no rubber stamp: on the oracle's first solution of instance A, moving
    x[3, 0] by 1e-5 shows as an equality residual of 1e-5 and moving u[4] by 1e-4 raises the
    stationarity residual above 1e-7 (from 1.5e-9)."""
    case = cc.BY_ID["cartpole_u_vx"]
    spec, data, hyp = cc.case_spec(case)
    sd = spec.to_dict()
    dyn = O.Dynamics(sd, oracle_gps(data, hyp))
    o = cc.oracle_run(case.id)[0][0]
    win = O.reference_window(spec.reference_trajectory(), case.instances[0].phase0, case.H)
    base = kkt_ref.certificate(sd, dyn, o.x, o.u, *o.bounds, win, x0=o.x0)
    assert base.eq <= 1e-12 and base.stat <= 1e-8
    x = o.x.copy()
    x[3, 0] += 1e-5
    assert 0.9e-5 <= kkt_ref.certificate(sd, dyn, x, o.u, *o.bounds, win, x0=o.x0).eq <= 1.1e-5
    u = o.u.copy()
    u[4] += 1e-4
    assert kkt_ref.certificate(sd, dyn, o.x, u, *o.bounds, win, x0=o.x0).stat >= 1e-7


@pytest.mark.parametrize("qp_tol,want", [
    (1e-6, {"V": [(0, 8), (2, 25), (0, 4), (0, 4), (0, 4)], "V'": [(0, 7), (2, 25), (0, 4), (0, 4), (0, 4)]}),
    (1e-10, {"V": [(0, 8), (0, 4), (0, 3), (0, 4), (0, 4)], "V'": [(0, 8), (0, 4), (0, 4), (0, 4), (0, 4)]})])
def test_divergent_case_at_default_tolerance(qp_tol, want):
    """quad2d_vx at the default NLP tolerance 1e-6 over five steps, with the QP solved to the same (the
    default) and to 1e-10: (status, SQP iterations) of both CPU references as they were before the IPM
    floored its slacks -- the floor of 1e-12 is never reached here, and must not show.  (Measured on the
    parent's build and on this one; the issue quotes 9, 4, 3, 4, 4 for V, which no combination of the
    tolerances reproduced -- a QP tolerance of 1e-10 gives 8, 4, 3, 4, 4.)"""
    case = cc.BY_ID["quad2d_vx"]
    orun = cc.oracle_run(case.id, 1e-6, qp_tol, 25, 5)
    crun = cpp_run(case, 1e-6, qp_tol, steps=5)
    for b, inst in enumerate(case.instances[:2]):
        assert [(row[b].status, row[b].sqp_iter) for row in orun] == want[inst.label], inst.label
        assert [(int(c[0][b]), int(c[1][b])) for c in crun] == want[inst.label], inst.label
        assert max(np.abs(c[2][b] - row[b].x).max() for c, row in zip(crun, orun)) <= 1e-9
