"""The reuse contract of the handles: after set_problem(B) succeeds on a handle that held a different
problem A, everything the handle computes is bit for bit what a new handle computes for B -- and still what the dense
fp64 references say.

Every transition test runs reuse_cases.dirty(h, A) (weights, a robust loss at f_scale 2.5 with curvature 0.1, pose
priors, ray priors, a marginal factor, a displacement, a device-driven run, both covariances, a marginal, a saved
state, an open trial), then set_problem(B), then reuse_cases.observe(h, B): the info queries, two host-driven steps
(scalars and states; the second reads the damping memory), the record-order residual, a device loop from a restored
snapshot, a host loop, covariance("all"), covariance_joint and marginal_prior.  It asserts np.array_equal on every item
against observe() on a new handle, and on the reused handle the first step against k1_cases.reference and the
covariance blocks against cov_ref at the gates of test_gpu_k1_paths.py / test_gpu_covariance.py: fp64 cost 1e-10, step
and predicted reduction 1e-7; fp32 cost 2e-6, step 2e-3, |delta|^2 4e-3; covariance blocks 1e-7 / 2e-3.  A case the
references do not state (a loss beyond Huber, two fixed frames, features set) is followed on the same handle by one
they do.  The stale data is what an ordinary preceding problem leaves; nothing is poisoned.

Also here: failed set_problem calls, the sticky caller-exchange mode, ptzba.solve's shared handle, EKFHandle's
buffers across shrinking updates, and the front end's work buffers from a large input to a small one."""
import dataclasses

import numpy as np
import pytest

import reuse_cases as rc
from reuse_cases import Case

pytestmark = pytest.mark.gpu

FULL = rc.FULL
C_TOL = {0: 1e-10, 1: 2e-6}
D_TOL = {0: 1e-7, 1: 2e-3}
D2_TOL = {0: 1e-7, 1: 4e-3}
COV_TOL = {0: 1e-7, 1: 2e-3}
_fresh = {}


def _new():
    import ptzba
    return ptzba.BAHandle(0)


def fresh(c):
    """observe(c) on a handle made for it: computed once per case and never modified."""
    if c not in _fresh:
        h = _new()
        rc.apply(h, c)
        _fresh[c] = rc.observe(h, c)
        h.close()
    return _fresh[c]


def _gates(tag, c, o):
    """The reused handle against the dense references (guards against reused and new being wrong alike)."""
    if c.has_reference:
        e = rc.first_step_errors(c, o)
        print(f"REUSE {tag} {c.name} precision={c.precision} loss={c.loss}: " + " ".join(f"{k}={v:.3e}" for k, v in e.items()))
        assert e["info"] == 0
        assert e["cost"] <= C_TOL[c.precision] and e["trial_cost"] <= C_TOL[c.precision], e
        assert e["step"] <= D_TOL[c.precision] and e["pred"] <= D_TOL[c.precision], e
        assert e["dx2"] <= D2_TOL[c.precision], e
    if c.loss in ("linear", "huber") and not c.features:
        ep, er = rc.covariance_errors(c, o)
        print(f"REUSE {tag} {c.name} precision={c.precision} n_fixed={c.n_fixed}: cov pose {ep:.3e} ray {er:.3e}")
        assert ep <= COV_TOL[c.precision] and er <= COV_TOL[c.precision], (ep, er)


def to(h, c, tag, applies=1):
    """set_problem(c) on the used handle, observe, compare with a new handle bit for bit and with the references."""
    for _ in range(applies):
        rc.apply(h, c)
    o = rc.observe(h, c)
    bad = rc.differing(o, fresh(c))
    assert not bad, (tag, c, bad)
    _gates(tag, c, o)
    return o


def _p(c, precision):
    return dataclasses.replace(c, precision=precision)


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("precision", [0, 1])
def test_shrink(gpu_available, precision):
    """P200 (weighted, Cauchy, every feature) -> P64 (plain, linear): the dense system buffer is replaced, every other
    buffer kept with the larger problem's data behind the smaller one's (test_reuse_cases.py); the factor's diagonal
    tiles, their inverses, the pose step and the status word keep their addresses."""
    a, b = (_p(c, precision) for c in rc.SIZE_PAIRS["shrink"])
    h = _new()
    rc.dirty(h, a)
    before = h.solver_buffers()
    assert h.solver_info()["backsolve"] == "blocked"
    o = to(h, b, "shrink")
    after = h.solver_buffers()
    h.close()
    assert all(after[k][0] == before[k][0] for k in before) and after["Ldiag"][1] < before["Ldiag"][1]
    assert o["solver_info"][5] == 0 and not o["displacement_info"][0] and o["pose_prior_info"][0] == 0


@pytest.mark.parametrize("precision", [0, 1])
def test_growth_within_slack(gpu_available, precision):
    """P140 -> P150: every buffer is kept, the records' and the state's grow into their quarter of slack."""
    a, b = (_p(c, precision) for c in rc.SIZE_PAIRS["growth_within_slack"])
    h = _new()
    rc.dirty(h, a)
    before = h.solver_buffers()
    to(h, b, "slack")
    after = h.solver_buffers()
    h.close()
    assert all(after[k] == before[k] for k in before)  # the same padded system dimension: the same buffers


@pytest.mark.parametrize("precision", [0, 1])
def test_growth_beyond_slack(gpu_available, precision):
    """P64 -> P200: nearly every buffer is replaced; the lookahead back-substitution gives way to the blocked one."""
    a, b = (_p(c, precision) for c in rc.SIZE_PAIRS["growth_beyond_slack"])
    h = _new()
    rc.dirty(h, a)
    assert h.solver_info()["backsolve"] == "lookahead"
    o = to(h, b, "growth")
    h.close()
    assert o["solver_info"][5] == 2


def test_back_substitution_form_there_and_back(gpu_available):
    """P200 -> P64 -> P200: blocked (persistent: its counters and epoch restart) -> lookahead -> blocked."""
    h = _new()
    rc.dirty(h, Case("P200w", **FULL))
    forms = [h.solver_info()["backsolve"]]
    for c in (Case("P64"), Case("P200"), Case("P64", precision=1), Case("P200", precision=1)):
        to(h, c, "backsolve")
        forms.append(h.solver_info()["backsolve"])
    h.close()
    assert forms == ["blocked", "lookahead", "blocked", "lookahead", "blocked"]


# ------------------------------------------------------------------------------------------------ same shape
def test_precision_flips(gpu_available):
    """P140 fp64 -> fp32 -> fp64: the record, table and slot buffers halve and double in place."""
    h = _new()
    rc.dirty(h, Case("P140w", **FULL))
    for precision in (1, 0, 1):
        to(h, Case("P140", precision=precision), "precision")
    h.close()


@pytest.mark.parametrize("precision", [0, 1])
def test_weighted_and_unweighted(gpu_available, precision):
    """The same records with and without weights (a stale rec_w), both ways, and merged pair-form records whose
    merged weights are multiplicities."""
    h = _new()
    rc.dirty(h, Case("P140w", precision=precision, **FULL))
    for name in ("P140", "P140w", "O140", "P140w", "P140"):
        to(h, Case(name, precision=precision), "weights")
    h.close()


@pytest.mark.parametrize("precision", [0, 1])
def test_record_stream_forms(gpu_available, precision):
    """Merged -> one record per segment -> unmerged and back; every form is really taken."""
    h = _new()
    rc.dirty(h, Case("M140", precision=precision, loss="cauchy", f_scale=2.5, features=True))
    seen = []
    for name in ("O140", "P140", "M140", "P140", "O140", "M140"):
        o = to(h, Case(name, precision=precision), "stream")
        seen.append((name, bool(o["k1_merge_info"][1]), bool(o["k1_merge_info"][2])))
    h.close()
    assert seen == [("O140", True, True), ("P140", False, False), ("M140", True, False), ("P140", False, False),
                    ("O140", True, True), ("M140", True, False)]


@pytest.mark.parametrize("precision", [0, 1])
def test_device_front_and_host_front(gpu_available, precision):
    """set_setup_front: the device front -> the host front -> the device front.  residual() and marginal_prior(drop_mask=)
    read the record permutation, which the device front writes itself and the host front uploads on first use; both
    are among the compared items.  The fronts also equal each other in everything they compute."""
    dev = Case("M140", precision=precision, front=0)
    host = Case("M140", precision=precision, front=2 ** 40)
    h = _new()
    rc.dirty(h, dataclasses.replace(dev, name="P140w", **FULL))
    for c in (host, dev, host, dataclasses.replace(dev, name="P150"), dataclasses.replace(host, name="P64")):
        o = to(h, c, "front")
        assert o["residual"].any() and o["marginal_prior"][5][0] > 0
    h.close()
    # (info()'s device_bytes counts the permutation from set_problem on under the device front, which writes it itself)
    assert rc.differing(fresh(dev), fresh(host)) == ["info"]
    assert np.flatnonzero(fresh(dev)["info"] != fresh(host)["info"]).tolist() == [7]


def test_fixed_frames_and_ordering(gpu_available):
    """n_fixed 1 -> 2 -> 1 and the natural order -> the nested orders (forced: one dissection level; default: two) and
    back, on the banded problem (padding rows and the reversed part come and go inside the kept system buffer)."""
    import ptzba
    h = _new()
    rc.dirty(h, Case("B140", ordering=ptzba.ORDER_NATURAL, loss="cauchy", f_scale=2.5, features=True))
    assert h.solver_info()["ordering"] == "natural"
    seen = []
    for c in (Case("B140", n_fixed=2, ordering=ptzba.ORDER_NESTED_FORCE), Case("B140", ordering=ptzba.ORDER_NATURAL),
              Case("B140"), Case("B140", n_fixed=2, ordering=ptzba.ORDER_NATURAL, precision=1),
              Case("B140", precision=1), Case("P140", precision=1)):
        o = to(h, c, "n_fixed / ordering")
        si = h.solver_info()
        seen.append((si["ordering"], si["nd_depth"], int(o["info"][4])))
        if c.n_fixed == 2:
            assert not o["covariance"][0][:2].any() and o["covariance"][0][2:].all()
    h.close()
    assert seen == [("nested", 1, 414), ("natural", 0, 417), ("nested", 2, 417), ("natural", 0, 414), ("nested", 2, 417),
                    ("natural", 0, 417)], seen


# ------------------------------------------------------------------------------------------------ features, loss
@pytest.mark.parametrize("precision", [0, 1])
def test_features_on_to_off(gpu_available, precision):
    """A has pose priors, ray priors, a marginal factor and a displacement; B has none and says so."""
    h = _new()
    rc.dirty(h, Case("P140", precision=precision, features=True))
    o = to(h, Case("P140", precision=precision), "features off")
    h.close()
    assert o["pose_prior_info"][0] == 0 and o["ray_prior_info"][0] == 0 and o["marginal_prior_info"][0] == 0
    assert not o["displacement_info"].any()
    assert o["marginal_prior"][5][2] == 0 and len(o["marginal_prior"][5]) == 3  # nothing absorbed


@pytest.mark.parametrize("precision", [0, 1])
def test_features_off_to_on(gpu_available, precision):
    """B sets all four features after a bare A (its first build is the first to take the separate prepare launch and
    the prior kernels on this handle); then the bare B, which the references state."""
    h = _new()
    rc.dirty(h, Case("P150", precision=precision))
    on = Case("P140", precision=precision, loss="huber", features=True)
    o = to(h, on, "features on")
    assert o["pose_prior_info"][0] == 2 and o["ray_prior_info"][:2].tolist() == [3, 2] and o["marginal_prior_info"][0] == 2
    assert o["displacement_info"][0] == 1 and np.array_equal(o["displacement_info"][1:], rc.DISPLACEMENT)
    assert o["pose_prior_info"][3] > 0 and o["ray_prior_info"][3] > 0 and o["marginal_prior"][5][2] == 1
    to(h, dataclasses.replace(on, features=False), "features on, then off")
    h.close()


@pytest.mark.parametrize("precision", [0, 1])
def test_loss_and_curvature(gpu_available, precision):
    """A: Cauchy, f_scale 2.5, curvature 0.1 (set by hand and by the device loop's switch); B: Huber with the defaults.
    The curvature does not carry over: B's first step is the IRLS step of the reference."""
    h = _new()
    rc.dirty(h, Case("P140w", precision=precision, **FULL))
    to(h, Case("P140", precision=precision, loss="huber"), "loss")
    to(h, Case("P140w", precision=precision, loss="huber", f_scale=2.5), "loss")
    to(h, Case("P140", precision=precision, loss="arctan", f_scale=2.5), "loss")
    to(h, Case("P140", precision=precision), "loss")
    h.close()


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("how", ["device", "host"])
def test_abandoned_runs(gpu_available, how, precision):
    """A run under A that never finished -- a device-driven one stopped after lm_solve with no lm_decide, a host-driven
    one stopped before accept -- then B with every feature (each setter is a between-solves call that refuses a pending
    trial), B's device loop and host loop, and the bare B."""
    a = Case("P150w", precision=precision, **FULL)
    h = _new()
    (rc.abandon_device_run if how == "device" else rc.abandon_host_run)(h, a)
    on = Case("P140", precision=precision, loss="huber", features=True)
    to(h, on, f"abandoned {how}")
    (rc.abandon_device_run if how == "device" else rc.abandon_host_run)(h, on)
    to(h, Case("P64", precision=precision), f"abandoned {how}")
    h.close()


def test_set_problem_twice(gpu_available):
    """set_problem(B) twice in a row, after a dirty A and on a new handle."""
    for precision in (0, 1):
        b = Case("P64", precision=precision, loss="huber")
        h = _new()
        rc.dirty(h, Case("P200w", precision=precision, **FULL))
        to(h, b, "twice", applies=2)
        h.close()
        h = _new()
        to(h, b, "twice, new handle", applies=2)
        h.close()


# ------------------------------------------------------------------------------------------------ failures
def test_failed_validation_leaves_the_problem_usable(gpu_available):
    """A set_problem that fails validation (a record with a frame out of range) on a handle holding A: A stays fully
    usable and computes what it computed before the call."""
    import ptzba
    a = Case("P140w", loss="huber", f_scale=2.5, features=True)
    h = _new()
    rc.apply(h, a)
    rc.observe(h, a)  # (the first residual uploads the permutation, which info()'s device_bytes counts from then on)
    before = rc.observe(h, a)
    u, v, ptz0, rays0, frame, landmark, xy, _ = rc.problem("P64")
    bad = frame.copy()
    bad[17] = len(ptz0)
    with pytest.raises(ptzba.PtzbaError, match="record 17: frame 64 out of range"):
        h.set_problem(len(ptz0), len(rays0), bad, landmark, xy, u, v)
    assert h.info()["n_pose"] == 140 and h.n_pose == 140
    assert not rc.differing(rc.observe(h, a), before)
    assert not [k for k in rc.differing(before, fresh(a)) if k != "info"]
    h.close()


def test_late_failure_leaves_no_problem(gpu_available):
    """A set_problem that fails after the handle's fields were overwritten (the dense solver's size limit: 6,400 poses
    with eight records, no device problem is built): every entry point that reads the problem refuses with "no problem
    set", and a following valid set_problem(B) equals a new handle."""
    import ptzba
    a = Case("P140w", **FULL)
    h = _new()
    rc.dirty(h, a)
    n = 6400
    fr = np.array([0, 1, 2, 3, 0, 1, 2, 3], np.int32)
    lm = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32)
    with pytest.raises(ptzba.PtzbaError, match="too large for the dense solver|factorisation plan"):
        h.set_problem(n, 2, fr, lm, np.full((8, 2), 100.0), 640.0, 360.0)
    ptz0, rays0 = a.p[2], a.p[3]
    x = np.concatenate([ptz0.reshape(-1), rays0.reshape(-1)])
    opts = ptzba.ptzba_lm_opts(1e-4, 1e-8, 0.0, 1e-12, 1e-12, 1e16, 3, 30, 0, 0.1, 0.25)
    calls = [h.info, h.k1_info, h.k1_merge_info, h.k2_info, h.k2_tile_info, h.build_info, h.schur_groups, h.solver_info,
             h.solver_buffers, lambda: h.residual(x), lambda: h.set_state(ptz0, rays0), h.get_state, h.save_state,
             h.restore_state, h.linearize, lambda: h.build_reduced(1e-2), h.solve_reduced, lambda: h.step(1e-2),
             h.read_scalars, lambda: h.accept(True), h.lm_start, lambda: h.lm_init(opts), h.lm_build, h.lm_solve,
             lambda: h.lm_decide(0), lambda: h.lm_wait(0), lambda: h.solve_resident(max_iter=3),
             lambda: h.solve(ptz0, rays0, max_iter=3), lambda: h.covariance("all"),
             lambda: h.covariance_joint([1, 2], [0]), lambda: h.set_pose_priors(rc.pose_factors(a.p)), h.clear_pose_priors,
             h.pose_prior_info, lambda: h.set_ray_priors(rc.ray_priors(a.p)), h.ray_prior_info,
             lambda: h.set_displacement(rc.DISPLACEMENT), h.displacement_info,
             lambda: h.marginal_prior(rc.leaving(a)[0], drop_mask=rc.leaving(a)[1]),
             lambda: h.set_marginal_prior(rc.marginal(a.p)), h.marginal_prior_info, h.exchange, h.exchange_packed,
             h.pack, h.unpack, h.dist_info, h.owned_frames]
    for call in calls:
        with pytest.raises(ptzba.PtzbaError, match="no problem set"):
            call()
    to(h, Case("P64", loss="huber"), "after a late failure")
    to(h, Case("P150", precision=1), "after a late failure")
    h.close()


def test_caller_exchange_mode_is_sticky(gpu_available):
    """exchange() under A switches the handle to the caller-exchange mode, which outlives set_problem (include/ptzba.h):
    B's steps and both LM loops still equal a new handle's bit for bit (the mode moves launches, not arithmetic), and
    priors and the displacement stay refused."""
    import ptzba
    h = _new()
    rc.apply(h, Case("P150w", loss="cauchy", f_scale=2.5))
    sys_ptr, count, scal_ptr = h.exchange()
    assert sys_ptr and scal_ptr and count == h.solver_info()["ld"] * (h.solver_info()["ld"] + 3)
    for b in (Case("P140", loss="huber"), Case("P64", precision=1, loss="huber")):
        rc.apply(h, b)
        o = rc.observe(h, b, between_solves=False)
        want = fresh(b)
        bad = rc.differing(o, {k: want[k] for k in o})
        assert not bad, (b, bad)
        assert "host_loop_state" in o and "covariance" not in o
        e = rc.first_step_errors(b, o)
        assert e["cost"] <= C_TOL[b.precision] and e["step"] <= D_TOL[b.precision], e
        with pytest.raises(ptzba.PtzbaError, match="single rank only"):
            h.set_pose_priors(rc.pose_factors(b.p))
        with pytest.raises(ptzba.PtzbaError, match="single rank only"):
            h.set_displacement(rc.DISPLACEMENT)
        with pytest.raises(ptzba.PtzbaError, match="single rank only"):
            h.set_ray_priors(rc.ray_priors(b.p))
    h.close()


# ------------------------------------------------------------------------------------------------ ptzba.solve
def _keyframe_calls():
    """Six keyframe-like solve() calls: growing problems, a precision and loss flip, a shrink; the options alternate."""
    import ptzba
    P = rc.problem
    p140 = P("P140")
    o = np.lexsort((p140[4], p140[5]))  # by landmark, then frame: the default drop mask pairs neighbouring records
    o = o[:len(o) // 2 * 2]
    sorted140 = p140[:4] + (p140[4][o], p140[5][o], p140[6][o], None)
    return [("P64", P("P64"), dict(pose_priors=rc.pose_factors(P("P64")))),
            ("P140", P("P140w"), dict(ray_priors=rc.ray_priors(P("P140w")), loss="cauchy", f_scale=2.5)),
            ("P150", P("P150"), dict(displacement=rc.DISPLACEMENT, loss="huber")),
            ("P200", P("P200"), dict(covariance=dict(landmarks="all", joint=([199, 1, 100], [0, 7, 3, 40])),
                                     marginal_prior=rc.marginal(P("P200")))),
            ("P140 fp32", sorted140, dict(precision=ptzba.FP32, loss="huber", marginalize=[1, 2],
                                          pose_priors=rc.pose_factors(p140))),
            ("P64", P("P64w"), dict(covariance=dict(landmarks=[5, 0, 5], scale="residual")))]


def _solve(p, keep, **kw):
    import ptzba
    u, v, ptz0, rays0, frame, landmark, xy, weight = p
    return ptzba.solve(len(ptz0), len(rays0), frame, landmark, xy, u, v, ptz0, rays0, weight=weight, keep_handle=keep,
                       max_iter=4, ftol=1e-15, xtol=1e-15, **kw)


def _flat(out):
    """Every array and every LMResult field of a solve() result (wall-clock fields left out)."""
    res = out[2]
    items = [out[0], out[1], np.array([res.status, res.cost, res.initial_cost, res.njev, res.nfev, res.iterations,
                                       res.lam, res.trials], np.float64)]
    for extra in out[3:]:
        if isinstance(extra, dict):  # marginalize=
            m, st = extra["marginal"], extra["stats"]
            items += [m.frames, m.lin, m.info, m.grad, np.array([m.offset, st["min_pivot"], st["dropped_records"],
                                                                 st["dropped_landmarks"], st["marginal_absorbed"]]),
                      np.array(st["absorbed"], np.int64)]
        else:  # covariance=
            pose_cov, ray_cov, info = extra
            items += [pose_cov, ray_cov, np.array([info["scale"], info["min_pivot"], info["n_free"]])]
            if "joint" in info:
                items.append(info["joint"])
    return items


def test_solve_shared_handle_equals_private_handles(gpu_available):
    """ptzba.solve(keep_handle=True) over a keyframe-like sequence equals keep_handle=False call by call, in every
    returned array and LMResult field; a call that raises in the middle drops the shared handle, and the call after it
    equals the private-handle result too."""
    import ptzba
    calls = _keyframe_calls()
    want = [_flat(_solve(p, False, **kw)) for _, p, kw in calls]
    ptzba.release_solve_handles()
    try:
        for k, (tag, p, kw) in enumerate(calls):
            got = _flat(_solve(p, True, **kw))
            assert len(got) == len(want[k])
            bad = [i for i, (x, y) in enumerate(zip(got, want[k])) if not np.array_equal(x, y)]
            assert not bad, (k, tag, bad)
            if k == 2:
                shared = ptzba._solve_handles[0]
                broken = p[:4] + (np.where(np.arange(len(p[4])) == 5, len(p[2]), p[4]).astype(np.int32),) + p[5:]
                with pytest.raises(ptzba.PtzbaError, match="record 5: frame 150 out of range"):
                    _solve(broken, True)
                assert 0 not in ptzba._solve_handles and shared.h is None
        assert ptzba._solve_handles[0].n_pose == 64
    finally:
        ptzba.release_solve_handles()
    assert not ptzba._solve_handles
    assert want[0][2][0] == 0 and want[0][2][5] == 4  # the runs really iterate


# ------------------------------------------------------------------------------------------------ EKFHandle
def test_ekf_handle_across_shrinking_updates(gpu_available):
    """One EKFHandle through updates of 240, 40, 1, 0 and 200 matches with remove_rays / add_rays between them: the
    innovation matrix and the signed factor shrink from 480 rows to 2 inside buffers kept by reserve().  Every update
    equals oracle.ekf_update on the state read before it (test_ekf_update_matches_oracle's tolerances) and, bit for
    bit, a new handle set to that state and given the same update."""
    import ptzba
    from oracle import ptz_oracle as orc
    from test_gpu_ekf import _random_state
    s0, _, _ = _random_state(300, 31, frac_obs=1.0)
    u, v, H, W = s0["u"], s0["v"], 1080, 1920
    rng = np.random.default_rng(32)
    h = ptzba.EKFHandle(0)
    h.set_state(s0["rays"], s0["state_cov"])
    ptz = np.array([s0["pan"], s0["tilt"], s0["f"]])
    for k, (n_match, edit) in enumerate([(240, None), (40, ("remove", 30)), (1, ("add", 15)), (0, None),
                                         (200, ("remove", 5))]):
        if edit and edit[0] == "remove":
            h.remove_rays(rng.choice(h.n_ray, edit[1], replace=False))
        elif edit:
            pts = np.stack([rng.uniform(100, W - 100, edit[1]), rng.uniform(100, H - 100, edit[1])], 1)
            h.add_rays(orc.back_project_to_rays(u, v, ptz[2], ptz[0], ptz[1], pts), 0.001)
        rays, cov = h.get_state()
        _, vis = orc.project_rays_visible(u, v, ptz[2], ptz[0], ptz[1], rays, H, W)
        vis = np.asarray(vis).astype(np.int64)
        assert len(vis) >= n_match
        idx = np.sort(rng.choice(vis, n_match, replace=False))
        obs = (orc.project_rays(u, v, ptz[2] + 2.0, ptz[0] + 0.02, ptz[1] - 0.01, rays[idx]) +
               rng.normal(0, 0.3, (n_match, 2))).reshape(-1, 2)
        got = h.update(u, v, ptz, obs, idx, H, W, 0.1)
        rays1, cov1 = h.get_state()
        g = ptzba.EKFHandle(0)
        g.set_state(rays, cov)
        new = g.update(u, v, ptz, obs, idx, H, W, 0.1)
        rays2, cov2 = g.get_state()
        g.close()
        assert got[2] == new[2] == n_match, (k, got[2], new[2])
        assert np.array_equal(got[0], new[0]) and np.array_equal(got[1], new[1]), k
        assert np.array_equal(rays1, rays2) and np.array_equal(cov1, cov2), k
        if n_match:
            s = dict(u=u, v=v, pan=ptz[0], tilt=ptz[1], f=ptz[2], displacement=None, rays=rays.copy(), state_cov=cov.copy())
            ref = orc.ekf_update(s, obs, idx, H, W)
            assert abs(got[0][0] - ref["pan"]) < 1e-9 and abs(got[0][1] - ref["tilt"]) < 1e-9
            assert abs(got[0][2] - ref["f"]) < 1e-6
            np.testing.assert_allclose(got[1], ref["velocity"], rtol=0, atol=1e-6)
            np.testing.assert_allclose(rays1, ref["rays"], rtol=0, atol=1e-9)
            np.testing.assert_allclose(cov1, ref["state_cov"], rtol=1e-7, atol=1e-13)
            assert np.array_equal(cov1 != cov, ref["state_cov"] != cov)
        else:  # no match: the state is left alone (test_ekf_update_no_match_leaves_state)
            assert np.all(got[1] == 0) and np.array_equal(got[0], ptz)
            assert np.array_equal(rays1, rays) and np.array_equal(cov1, cov)
        ptz = got[0]
    assert h.n_ray == 300 - 30 + 15 - 5
    h.close()


# ------------------------------------------------------------------------------------------------ front end
def test_front_end_work_buffers_from_large_to_small(gpu_available):
    """sift, orb, corner_min_eig, lk_track and match_knn2 keep per-device work buffers that only grow: each runs on a
    large input and then on a small one, whose result meets the assertions of the oracle tests
    (test_gpu_frontend.py)."""
    import frontend_data
    import ptzba
    from oracle import ptz_oracle as orc
    from test_gpu_frontend import _lk_compare, _lk_points, _sift_match
    big, bigJ, _ = frontend_data.textured_pair(seed=7, width=640, height=360, d_pan=1.5, d_tilt=-0.5, f=900.0, df=12.0)
    # sift
    assert len(ptzba.sift(big, 0)[0]) > 500
    I, _, _ = frontend_data.textured_pair(seed=2, width=192, height=144, d_pan=0.5, f=400.0)
    kg, rg, dg = ptzba.sift(I, 0)
    ko, ro, do = orc.sift_detect_compute(I, 0)
    assert len(kg) == len(ko) > 50
    pr = _sift_match(kg, ko)
    assert len(pr) == len(ko)
    assert np.array_equal(kg[pr[:, 0], :3], ko[pr[:, 1], :3]) and np.array_equal(rg[pr[:, 0]], ro[pr[:, 1]])
    da = np.abs(kg[pr[:, 0], 3] - ko[pr[:, 1], 3])
    assert np.minimum(da, 360 - da).max() < 1e-3
    dd = np.abs(dg[pr[:, 0]] - do[pr[:, 1]])
    assert dd.max() <= 1 and np.mean(dd.max(1) == 0) >= 0.99 and np.all(np.diff(rg) <= 0)
    # orb
    assert len(ptzba.orb(big, 1500, "orb")[0]) > 500
    I, _, _ = frontend_data.textured_pair(seed=22, width=257, height=181, d_pan=0.5, f=400.0)
    kg, dg = ptzba.orb(I, 300, "orb")
    ko, do = orc.orb_detect_compute(I, 300, "orb")
    assert len(kg) == len(ko) > 50 and np.array_equal(kg[:, [0, 1, 2, 4, 5]], ko[:, [0, 1, 2, 4, 5]])
    da = np.abs(kg[:, 3].astype(np.float64) - ko[:, 3])
    assert np.minimum(da, 360 - da).max() < 1e-3 and np.array_equal(dg, do)
    # corner_min_eig
    wide, _, _ = frontend_data.textured_pair(seed=13, width=1280, height=720)
    assert ptzba.corner_min_eig(wide)[1].sum() > 0
    I, _, _ = frontend_data.textured_pair(seed=12, width=257, height=131)
    eig, loc = ptzba.corner_min_eig(I)
    reig, rloc = orc.corner_min_eig(I)
    np.testing.assert_array_equal(eig, reig)
    np.testing.assert_array_equal(loc, rloc)
    assert loc.sum() > 0 and not loc[0].any() and not loc[:, -1].any()
    # lk_track
    assert ptzba.lk_track(big, bigJ, _lk_points(3, 2000, 640, 360), levels=5)[1].mean() > 0.5
    I, J, _ = frontend_data.textured_pair(seed=2, width=257, height=199, flat_box=(0, 0, 40, 40))
    p = _lk_points(2, 300, 257, 199)
    p[:3] = [[15.0, 15.0], [20.0, 22.0], [256.0, 198.0]]
    nxt, st, err = _lk_compare(I, J, p, win=21, levels=3)
    assert st[:2].sum() == 0 and (st == 1).mean() > 0.9
    # match_knn2
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (1500, 128)).astype(np.float32)
    b = rng.integers(0, 256, (1400, 128)).astype(np.float32)
    assert ptzba.match_knn2(a, b)[0].min() >= 0
    for n1, n2 in ((130, 2), (1, 70), (37, 70)):
        idx, dist = ptzba.match_knn2(a[:n1], b[:n2])
        ridx, rdist = orc.knn2(a[:n1], b[:n2])
        assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist.astype(np.float32)), (n1, n2)
