"""The LM decision rules on the CPU: the reference state machine (tests/lm_ref.py) against a table of decisions
written out by hand, and ptzba.LMSolver's host loop against the reference -- on scripted scalar sequences and on the
real trajectories of tests/lm_cases.py (dense fp64 numpy handle).  No GPU, no native library."""
import math

import numpy as np
import pytest

import lm_cases as lc
import lm_ref


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("row", lc.TABLE, ids=repr)
def test_reference_gives_the_table(row):
    """Every field of every record is the literal the table holds (lambda and cost bit for bit), decided one at a
    time from the crafted scalars."""
    s = lm_ref.start(row.cost0, row.opts)
    assert (s.cost, s.initial_cost, s.lam, s.nu, s.nfev) == (row.cost0, row.cost0, row.opts.lambda0, 2.0, 1)
    for k, (step, want) in enumerate(row.steps):
        s = lm_ref.decide(s, lc.scalars8(step, s.cost), row.opts)
        got = {f: getattr(s, f) for f in want}
        assert all(_same(got[f], want[f]) for f in want), (row.name, k, got, want)
        assert s.initial_cost == row.cost0


def test_table_covers_every_exit():
    """The table reaches every status, both from an accepted and a rejected trial where the rules allow it."""
    seen = {(w["status"], w["accepted"]) for row in lc.TABLE for _, w in row.steps if w["done"]}
    assert {(lm_ref.FTOL, 1), (lm_ref.XTOL, 1), (lm_ref.GTOL, 1), (lm_ref.MAX_ITER, 1), (lm_ref.DAMPING, 0),
            (lm_ref.FAILED, 0)} <= seen


@pytest.mark.parametrize("row", lc.TABLE, ids=repr)
def test_reference_run_replays_the_table(row):
    """lm_ref.run over the scripted handle: the records of the table's steps, as long as the run lasts, and the
    damping of every build is the lambda of the record before it."""
    h = lc.ScriptedHandle(row.cost0, [s for s, _ in row.steps])
    recs = lm_ref.run(h, row.opts)
    assert recs[-1].done and not any(r.done for r in recs[:-1])
    for k, (r, (_, want)) in enumerate(zip(recs, row.steps)):
        got = {f: getattr(r, f) for f in want}
        assert all(_same(got[f], want[f]) for f in want), (row.name, k, got, want)
    assert h.lams == [row.opts.lambda0] + [r.lam for r in recs[:-1]]


def _host(handle, opts):
    import ptzba
    return ptzba.LMSolver(handle, device_loop=False, **opts.solver_kwargs()).run()


def _equal(res, recs, what):
    last = recs[-1]
    assert (res.status, res.iterations, res.njev, res.nfev) == (last.status, last.iterations, last.iterations,
                                                                 last.nfev), (what, res, last)
    assert res.lam == last.lam, (what, res.lam, last.lam)
    assert res.initial_cost == last.initial_cost
    assert abs(res.cost - last.cost) <= 1e-12 * abs(last.cost), (what, res.cost, last.cost)


@pytest.mark.parametrize("row", lc.TABLE, ids=repr)
def test_host_loop_equals_reference_scripted(row):
    """ptzba.LMSolver's host loop and the reference over the same scripted scalars (the tie rows included): status,
    iterations, nfev and lambda equal, the cost to 1e-12."""
    steps = [s for s, _ in row.steps]
    recs = lm_ref.run(lc.ScriptedHandle(row.cost0, steps), row.opts)
    h = lc.ScriptedHandle(row.cost0, steps)
    res = _host(h, row.opts)
    _equal(res, recs, row.name)
    assert h.lams == [row.opts.lambda0] + [r.lam for r in recs[:-1]]  # the same damping in every build


@pytest.mark.parametrize("name", list(lc.SCENARIOS))
def test_host_loop_equals_reference_real(name):
    """The same on the real trajectories, on the dense fp64 numpy handle: the reference reaches the exit the scenario
    is there for, its window keeps the margins the GPU comparison relies on, and the host loop ends as it does, in the
    same state."""
    opts = lc.scenario_opts(name)
    recs, (ptz, rays) = lc.reference(name)
    assert recs[-1].status == lc.EXPECTED_STATUS[name] and recs[-1].done
    lc.check_reference_margins(recs, opts)
    h = lc.numpy_handle()
    res = _host(h, opts)
    _equal(res, recs, name)
    p2, r2 = h.get_state()
    assert np.array_equal(p2, ptz) and np.array_equal(r2, rays)


def test_scenarios_reach_what_they_are_for():
    """The windows hold what their names say: rejections before the recovery, the tie at the very rejection that
    reaches max_retries, rejections before MAX_ITER, lambda on its floor."""
    rec = lc.reference("recover")[0]
    assert [r.accepted for r in rec] == [1] + [0] * 7 + [1] * 4
    tie, opts = lc.reference("tie")[0], lc.scenario_opts("tie")
    assert tie[-1].retries == opts.max_retries and tie[-1].lam > opts.max_lambda and tie[-1].status == lm_ref.DAMPING
    assert tie[-2].lam <= opts.max_lambda
    failed = lc.reference("failed")[0]
    assert failed[-1].retries == 3 and failed[-1].lam <= 1e16
    assert sum(1 - r.accepted for r in lc.reference("max_iter")[0]) >= 3
    floor = lc.reference("floor")[0]
    assert sum(r.lam == 1.0 and r.factor * r.old_lam < 1.0 for r in floor) >= 3
    assert any(r.factor is not None and r.factor > lc.THIRD and r.lam > lc.scenario_opts(n).min_lambda
               for n in lc.SCENARIOS for r in lc.reference(n)[0])  # an unsaturated factor is compared somewhere


def test_non_finite_start_raises():
    with pytest.raises(ValueError):
        lm_ref.run(lc.ScriptedHandle(float("nan"), []), lm_ref.Opts())
    assert lm_ref.run(lc.ScriptedHandle(1.0, []), lm_ref.Opts(max_iter=0)) == []
