"""The LM decision rules on the GPU against the reference state machine (tests/lm_ref.py), trial by trial.

A. Real trajectories.  The problem is synthetic.make_small_problem(12, 150, -8.0, 8.0, seed=1) (12 poses, 101
landmarks, 3,520 records), started from tests/lm_cases.far_start(): the initial poses, the free ones moved by 60 times
the fourth (11, 3) normal draw of default_rng(0) scaled by (0.3, 0.2, 30).  From there a Gauss-Newton run accepts once
(rho 0.946), rejects seven times in a row (rho <= -0.796, lambda 1e-9 ... 1.3e-1) and accepts four times (rho 0.957
... 1.185); the reference's next decision has rho -0.038, so that window ends at max_iter = 5.  Nine option sets
(lm_cases.SCENARIOS) lead through rejections and recovery, FAILED, DAMPING, the DAMPING / FAILED tie, MAX_ITER, FTOL,
XTOL, GTOL and the min_lambda floor.  Every decision record of the device-driven LM (lm_start / lm_init / lm_build /
lm_solve / lm_decide / lm_wait) is compared with the reference's run on the dense fp64 numpy handle, with the decision
fused into the trial-cost reduce (the default) and stand-alone (k_lm_decide, a handle whose exchange() was called):
discrete fields equal; cost to 1e-7 relative (the fp64 step gate of tests/test_gpu_k1_paths.py); lambda to 20 * 1e-7 *
cost / actual where its factor depends on rho, and exact to 1e-12 elsewhere -- its value where it does not depend on
the lambda before it (min_lambda floor, zero, 1e-9), its quotient by the lambda before it where the update is one
product by a constant (after a rejection, at the factor's 1/3 floor), the value then carrying the gate of the lambda
before it (lm_cases.lam_gates: a lambda divided by three keeps the relative deviation it had, so against the
reference's value it cannot be held tighter than the trial before it); the final state to 1e-6 of the largest
displacement from the start, per parameter kind.  The margins that keep rounding from flipping a
decision are asserted on the reference alone (lm_cases.check_reference_margins).  One more lm_build after the final
decision leaves the state as it is.  The four loops a caller can take (LMSolver with the device and the host loop,
solve, solve_resident) report the reference's status, iterations and nfev.  fp32: the discrete fields only, for the
windows without a converged tail.

B. Crafted scalars.  A handle that called exchange() leaves the 16-double scalar buffer (scal[0..8) | loc[0..8)) to its
caller between lm_start and lm_init and between lm_solve and lm_decide (include/ptzba.h: the all-reduce points).  Every
row of lm_cases.TABLE that needs no factorisation status is written there and decided by the stand-alone kernel: the
row's starting cost into scal[0] before lm_init (the cost the decision state starts from), then per step the trial cost
and the rays' max |g| into scal[1], scal[5], pred, |dx|^2 and |x|^2 split in halves between scal[2..4] and loc[0..2]
(the decision adds them), the poses' max |g| into loc[3], zero into loc[5].  The record must be the table's: discrete
fields and cost exactly, lambda to 1e-15 relative (1 - t*t*t may be contracted into an fma on the device).

Measured on an MI355X (the LMRULES lines; maxima over the nine scenarios, the same in both decision forms):
  cost, relative                                      3.89e-12  (recover; gate 1e-7)
  lambda where exact (values and quotients)           0.0       (bit for bit; gate 1e-12)
  lambda elsewhere, as a share of its gate            6.77e-7   (ftol / xtol / gtol: 1.5e-12 relative; gate 2.2e-6)
  final state, as a share of the largest displacement 2.89e-12  (max_iter; gate 1e-6)
fp32 and the crafted rows compare no continuous figure but the table's own (all exact on the device)."""
import numpy as np
import pytest

import lm_cases as lc
import lm_ref

pytestmark = pytest.mark.gpu

FORMS = ("fused", "standalone")
FP32_SCENARIOS = ("failed", "damping", "tie", "recover")


def _c_opts(o):
    import ptzba
    return ptzba.ptzba_lm_opts(o.ftol, o.xtol, o.gtol, o.lambda0, o.min_lambda, o.max_lambda, o.max_iter,
                               o.max_retries, 1 if o.gauss_newton else 0, 0.1, 0.25)


def _open(precision, form="fused", start=None):
    import ptzba
    p = lc.problem()
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=precision)
    h.set_state(lc.far_start() if start is None else start, p.init_rays)
    if form == "standalone":
        h.exchange()  # the caller may reduce the scalars itself from now on: no fused decision
    return h


def _records(h, opts):
    """The device-driven LM, trial by trial (ptzba.LMSolver._run_device's sequence): every decision record."""
    h.lm_start()
    h.lm_init(_c_opts(opts))
    h.lm_build()
    recs, limit = [], opts.max_iter * (opts.max_retries + 1)
    for k in range(limit):
        h.lm_solve()
        h.lm_decide(k)
        if k + 1 < limit:
            h.lm_build()
        recs.append(h.lm_wait(k))
        if recs[-1].done:
            break
    return recs


def _discrete(recs, ref, what):
    assert len(recs) == len(ref), (what, len(recs), len(ref))
    for k, (r, e) in enumerate(zip(recs, ref)):
        got = tuple(getattr(r, f) for f in lm_ref.DISCRETE_FIELDS)
        want = tuple(getattr(e, f) for f in lm_ref.DISCRETE_FIELDS)
        assert got == want, (what, k, dict(zip(lm_ref.DISCRETE_FIELDS, got)), dict(zip(lm_ref.DISCRETE_FIELDS, want)))


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0.0 else abs(a)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(lc.SCENARIOS))
def test_trajectory_fp64(gpu_available, name, form):
    opts = lc.scenario_opts(name)
    ref, (ptz_ref, rays_ref) = lc.reference(name)
    lc.check_reference_margins(ref, opts)
    assert ref[-1].status == lc.EXPECTED_STATUS[name]
    p, far = lc.problem(), lc.far_start()
    h = _open(0, form)
    recs = _records(h, opts)
    ptz, rays = h.get_state()
    h.lm_build()  # one more build after the final decision: harmless
    h.sync()
    ptz2, rays2 = h.get_state()
    h.close()
    # measured first, asserted after
    gates = lc.lam_gates(ref, opts)
    e_cost = max(_rel(r.cost, e.cost) for r, e in zip(recs, ref))
    n = min(len(recs), len(ref))
    e_lam = [_rel(recs[k].lam, ref[k].lam) for k in range(n)]
    # the update where it is one product by a constant: lambda / previous lambda against the reference's quotient
    e_quot = [_rel(recs[k].lam / recs[k - 1].lam, ref[k].lam / ref[k - 1].lam) if k > 0 and gates[k][1] else 0.0
              for k in range(n)]
    e_exact = max([e_lam[k] for k in range(n) if gates[k][0] == 1e-12] + e_quot, default=0.0)
    e_gated = max([e_lam[k] / gates[k][0] for k in range(n) if gates[k][0] != 1e-12], default=0.0)
    e_state = 0.0
    for got, want, x0 in ((ptz, ptz_ref, far), (rays, rays_ref, p.init_rays)):
        for c in range(want.shape[1]):
            disp = np.abs(want[:, c] - x0[:, c]).max()
            assert disp > 0
            e_state = max(e_state, np.abs(got[:, c] - want[:, c]).max() / disp)
    print(f"LMRULES {name} {form}: trials {len(recs)} cost rel {e_cost:.2e} lambda rel (exact products) {e_exact:.2e} "
          f"lambda / gate (elsewhere) {e_gated:.2e} state / displacement {e_state:.2e}")
    _discrete(recs, ref, (name, form))
    for k, (r, e, (g, _)) in enumerate(zip(recs, ref, gates)):
        assert r.initial_cost == recs[0].initial_cost and _rel(r.initial_cost, e.initial_cost) <= 1e-7
        assert _rel(r.cost, e.cost) <= 1e-7, (name, form, k, r.cost, e.cost)
        assert e_lam[k] <= g, (name, form, k, r.lam, e.lam, g)
        assert e_quot[k] <= 1e-12, (name, form, k, r.lam, recs[k - 1].lam, e.lam, ref[k - 1].lam)
    assert e_state <= 1e-6, e_state
    assert np.array_equal(ptz2, ptz) and np.array_equal(rays2, rays)


@pytest.mark.parametrize("name", list(lc.SCENARIOS))
def test_every_loop_reports_the_reference(gpu_available, name):
    """LMSolver with the device loop and with the host loop, BAHandle.solve and solve_resident: the reference's status,
    iterations and nfev (the cost to the step gate)."""
    import ptzba
    opts = lc.scenario_opts(name)
    last = lc.reference(name)[0][-1]
    p, far = lc.problem(), lc.far_start()
    kw = opts.solver_kwargs()
    h = _open(0)
    out = {}
    out["device"] = ptzba.LMSolver(h, device_loop=True, **kw).run()
    h.set_state(far, p.init_rays)
    out["host"] = ptzba.LMSolver(h, device_loop=False, **kw).run()
    out["solve"] = h.solve(far, p.init_rays, **kw)[2]
    h.set_state(far, p.init_rays)
    out["solve_resident"] = h.solve_resident(**kw)
    h.close()
    for loop, res in out.items():
        assert (res.status, res.iterations, res.nfev) == (last.status, last.iterations, last.nfev), (name, loop, res, last)
        assert _rel(res.cost, last.cost) <= 1e-7, (name, loop, res.cost, last.cost)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", FP32_SCENARIOS)
def test_trajectory_fp32_discrete(gpu_available, name, form):
    opts = lc.scenario_opts(name)
    ref = lc.reference(name)[0]
    lc.check_reference_margins(ref, opts)
    h = _open(1, form)
    recs = _records(h, opts)
    h.close()
    _discrete(recs, ref, (name, form, "fp32"))


# -------------------------------------------------------------------------------------------------
# B. crafted scalars into the stand-alone decision
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(gpu_available):
    import torch
    import bench
    h = _open(0, start=lc.problem().init_ptz)
    _, _, sc = h.exchange()
    arr = bench._DevArray(sc, 16)
    view = torch.as_tensor(arr, device="cuda:0")  # scal[0..8) | loc[0..8), aliased
    yield h, view, arr
    h.close()


def _write(view, values):
    import torch
    for slot, v in values.items():
        view[slot] = v
    torch.cuda.synchronize()


@pytest.mark.parametrize("row", [r for r in lc.TABLE if not r.needs_info], ids=repr)
def test_crafted_scalars_standalone(crafted, row):
    h, view, _ = crafted
    p = lc.problem()
    h.set_state(p.init_ptz, p.init_rays)
    h.lm_start()
    h.sync()
    _write(view, {0: row.cost0})  # the caller's all-reduce point between lm_start and lm_init
    h.lm_init(_c_opts(row.opts))
    h.lm_build()
    h.lm_solve()
    h.sync()
    bad = []
    for k, (s, want) in enumerate(row.steps):
        _write(view, {1: s["new"], 2: 0.5 * s["pred"], 3: 0.5 * s["dx2"], 4: 0.5 * s["x2"], 5: s["g_ray"],
                      8: 0.5 * s["pred"], 9: 0.5 * s["dx2"], 10: 0.5 * s["x2"], 11: s["g_pose"], 13: 0.0})
        h.lm_decide(k)
        r = h.lm_wait(k)  # every decided trial is waited for
        got = {f: getattr(r, f) for f in lm_ref.RECORD_FIELDS}
        for f in lm_ref.DISCRETE_FIELDS:
            if got[f] != want[f]:
                bad.append((k, f, got[f], want[f]))
        if got["cost"] != want["cost"] or got["initial_cost"] != row.cost0:
            bad.append((k, "cost", got["cost"], want["cost"], got["initial_cost"], row.cost0))
        if not (got["lam"] == want["lam"] or abs(got["lam"] - want["lam"]) <= 1e-15 * abs(want["lam"])):
            bad.append((k, "lam", got["lam"], want["lam"]))
    h.sync()
    ptz, rays = h.get_state()
    assert np.isfinite(ptz).all() and np.isfinite(rays).all()  # only the decision read the crafted numbers
    assert not bad, (row.name, bad)
