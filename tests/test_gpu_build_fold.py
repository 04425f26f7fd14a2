"""The build prologue folded into K2 and the trial kernel (device-driven single-GPU fp32 solves: K2's product waves zero
the pattern tiles, b | g_pose | dU and info, its list build and k_trial form the landmark damping themselves through
lm_damp; csrc/schur_kernels.hip, csrc/ba_kernels.hip, build_impl in csrc/api.hip) against the k_build_prologue launch it
replaces, which PTZBA_K2_PROLOGUE=1 forces: the same fp64 expressions on the same inputs, so the state, the result tuple
and every decision record are equal bit for bit.

BAHandle.build_info() counts the builds enqueued on either path, so each case also asserts which path it really took:
the default takes the folded one, the forced setting and the paths the fold leaves alone (a pose prior,
PTZBA_NO_FUSED_PREP, the host-step API, covariance and marginal_prior's own builds) the prologue launch."""
import numpy as np
import pytest

import k2_cases as k2c
from prior_ref import SIGMA

pytestmark = pytest.mark.gpu

SETTINGS = ("1", None)  # PTZBA_K2_PROLOGUE: the prologue launch (the reference), the default
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _config2():
    def make():
        import synthetic
        p = synthetic.make_problem("config2", seed=0)
        return p.u, p.v, p.init_ptz, p.init_rays, p.frame, p.landmark, p.xy, None
    return _memo("config2", make)


N_ODD = 70
LM_NONE, LM_FIXED = 5, 9  # a landmark without records, a landmark only the fixed frame 0 sees


def _odd():
    """70 poses, ~400 landmarks of 3-10 consecutive frames; landmark LM_NONE has no record at all (its segment carries
    zero records), landmark LM_FIXED two records in frame 0 only."""
    def make():
        rng = np.random.default_rng(101)
        segs = []
        for lm in range(400):
            if lm == LM_NONE:
                segs.append((lm, 3, 0))
            elif lm == LM_FIXED:
                segs.append((lm, 0, 2))
            else:
                k = int(rng.integers(3, 11))
                s = min(lm % N_ODD, N_ODD - k) if lm < 2 * N_ODD else int(rng.integers(0, N_ODD - k + 1))
                segs += [(lm, f, int(rng.integers(1, 3))) for f in range(s, s + k)]
        return k2c.build(N_ODD, segs, 102)
    return _memo("odd", make)


def _one_item():
    """20 poses, 8 landmarks seen by every frame: one F1 block, one chunk, one list -- a single work item that zeroes
    every pattern tile."""
    return _memo("one", lambda: k2c.build(20, [(lm, f, 1) for lm in range(8) for f in range(20)], 103))


def _open(p, loss, setting, monkeypatch, env=(), win=None):
    import ptzba
    for name in ("PTZBA_NO_FUSED_PREP", "PTZBA_K2_PROLOGUE"):
        monkeypatch.delenv(name, raising=False)
    if setting is not None:
        monkeypatch.setenv("PTZBA_K2_PROLOGUE", setting)
    for name in env:
        monkeypatch.setenv(name, "1")
    u, v, ptz0, rays0, frame, landmark, xy, weight = p
    h = ptzba.BAHandle(0)
    kw = {} if win is None else dict(frame_win_hi=win)
    h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, weight=weight, precision=ptzba.FP32,
                  loss=ptzba.LOSS_HUBER if loss == "huber" else ptzba.LOSS_LINEAR, **kw)
    h.set_state(ptz0, rays0)
    return h


def _res(r):
    return (r.cost, r.initial_cost, r.njev, r.nfev, r.status, r.trials)


def _path(h, setting, folded=True):
    """The builds of this handle so far went down the path the case is there for."""
    bi = h.build_info()
    assert bi["forced_prologue"] == (setting == "1"), bi
    if setting is None and folded:
        assert bi["folded_builds"] >= 1 and bi["prologue_builds"] == 0, bi
    else:
        assert bi["folded_builds"] == 0 and bi["prologue_builds"] >= 1, bi


def _same(out):
    (ptz, rays), res = out[0]
    assert np.isfinite(ptz).all() and np.isfinite(rays).all()
    for (p2, r2), res2 in out[1:]:
        assert res2 == res, (res2, res)
        assert np.array_equal(p2, ptz) and np.array_equal(r2, rays)


@pytest.mark.parametrize("loss", ["huber", "linear"])
def test_config2_solve_bitwise_equal(gpu_available, loss, monkeypatch):
    p, out = _config2(), []
    for setting in SETTINGS:
        h = _open(p, loss, setting, monkeypatch)
        r = h.solve_resident(ftol=1e-14, xtol=1e-16, max_iter=3)
        _path(h, setting)
        out.append((h.get_state(), _res(r)))
        h.close()
    assert out[0][1][2] == 3 and not np.array_equal(out[0][0][0], p[2])  # three accepted steps: the state moved
    _same(out)


def _records(h, lambda0, max_iter):
    """The device-driven LM, trial by trial (ptzba.LMSolver._run_device's sequence): every decision record."""
    import ptzba
    h.lm_start()
    h.lm_init(ptzba.ptzba_lm_opts(1e-14, 1e-16, 0.0, lambda0, 1e-12, 1e16, max_iter, 30, 0, 0.1, 0.25))
    h.lm_build()
    recs, limit = [], max_iter * 31
    for k in range(limit):
        h.lm_solve()
        h.lm_decide(k)
        if k + 1 < limit:
            h.lm_build()
        r = h.lm_wait(k)
        recs.append((r.cost, r.lam, r.iterations, r.nfev, r.trials, r.retries, r.status, r.done, r.accepted))
        if r.done:
            break
    return recs


def test_rejected_trial_rebuild_bitwise_equal(gpu_available, monkeypatch):
    """A start 40 x further from the optimum than the case's own, with Gauss-Newton damping: the first steps overshoot
    and are rejected, so the build runs again on the same linearisation with a larger lambda (the damping re-formed from
    unchanged rows and an unchanged D_ray).  The records prove the rejections."""
    u, v, ptz0, rays0, frame, landmark, xy, w = _odd()
    rng = np.random.default_rng(104)
    far = ptz0 + rng.normal(0, 1.0, ptz0.shape) * np.array([0.6, 0.4, 200.0])
    far[0] = ptz0[0]
    p, out = (u, v, far, rays0, frame, landmark, xy, w), []
    for setting in SETTINGS:
        h = _open(p, "huber", setting, monkeypatch)
        recs = _records(h, 1e-12, 4)
        _path(h, setting)
        out.append((h.get_state(), recs))
        h.close()
    recs = out[0][1]
    print(f"BUILDFOLD retries per record {[r[5] for r in recs]} accepted {[r[8] for r in recs]}")
    assert max(r[5] for r in recs) >= 1 and any(r[8] for r in recs), recs
    _same(out)


def test_landmarks_without_a_step_bitwise_equal(gpu_available, monkeypatch):
    """A landmark without records keeps a zero step and its ray; a landmark only the fixed frame sees is in no K2 list
    but has a block of its own, which k_trial damps."""
    p, out = _odd(), []
    frame, landmark = p[4], p[5]
    assert not (landmark == LM_NONE).any() and set(frame[landmark == LM_FIXED]) == {0}
    for setting in SETTINGS:
        h = _open(p, "huber", setting, monkeypatch)
        assert h.info()["n_active_landmarks"] == len(p[3]) - 1
        r = h.solve_resident(ftol=1e-14, xtol=1e-16, max_iter=3)
        _path(h, setting)
        out.append((h.get_state(), _res(r)))
        h.close()
    rays = out[1][0][1]
    assert np.array_equal(rays[LM_NONE], p[3][LM_NONE]) and not np.array_equal(rays[LM_FIXED], p[3][LM_FIXED])
    _same(out)


def test_ray_priors_bitwise_equal(gpu_available, monkeypatch):
    """Ray priors on all landmarks with records: lm_out holds their share before either path reads it."""
    p, out = _odd(), []
    rng = np.random.default_rng(105)
    pri = [(lm, p[3][lm] + rng.normal(0, 0.01, 2), np.diag([4e3, 6e3]) + 5e2) for lm in range(len(p[3])) if lm != LM_NONE]
    for setting in SETTINGS:
        h = _open(p, "huber", setting, monkeypatch)
        h.set_ray_priors(pri)
        assert h.ray_prior_info()[1] == len(pri)
        r = h.solve_resident(ftol=1e-14, xtol=1e-16, max_iter=3)
        _path(h, setting)
        out.append((h.get_state(), _res(r)))
        h.close()
    _same(out)


@pytest.mark.parametrize("how", ["pose_prior", "no_fused_prep"])
def test_unfused_builds_keep_the_prologue(gpu_available, how, monkeypatch):
    """A pose prior and PTZBA_NO_FUSED_PREP=1 switch the fused prepare off: both settings launch the prologue."""
    p, out = _odd(), []
    W = np.diag(1.0 / SIGMA ** 2)
    rng = np.random.default_rng(106)
    factors = [([f], p[2][f] + rng.uniform(-3, 3, 3) * SIGMA, W) for f in range(1, N_ODD, 4)]
    for setting in SETTINGS:
        h = _open(p, "huber", setting, monkeypatch, env=("PTZBA_NO_FUSED_PREP",) if how == "no_fused_prep" else ())
        if how == "pose_prior":
            h.set_pose_priors(factors)
        r = h.solve_resident(ftol=1e-14, xtol=1e-16, max_iter=3)
        _path(h, setting, folded=False)
        out.append((h.get_state(), _res(r)))
        h.close()
    _same(out)


def test_second_solve_after_other_builds_bitwise_equal(gpu_available, monkeypatch):
    """Between two resident solves a covariance call, a marginal_prior call and a host-step build at lambda 1e-3 leave
    their own S, vectors, lm_aux and D_ray behind (all through the prologue launch): the second solve's first folded
    build zeroes for itself and reads none of it."""
    p, out = _odd(), []
    for setting in SETTINGS:
        h = _open(p, "huber", setting, monkeypatch)
        r1 = h.solve_resident(ftol=1e-14, xtol=1e-16, max_iter=2)
        _path(h, setting)
        n0 = h.build_info()["prologue_builds"]
        cov, _, ci = h.covariance()
        m, _ = h.marginal_prior([1])
        h.linearize()
        h.build_reduced(1e-3)
        assert h.build_info()["prologue_builds"] >= n0 + 3
        r2 = h.solve_resident(ftol=1e-14, xtol=1e-16, max_iter=2)
        out.append((h.get_state(), (_res(r1), _res(r2), ci["min_pivot"], cov.tobytes(), m.info.tobytes())))
        h.close()
    assert out[0][1][1][2] >= 1
    _same(out)


@pytest.mark.parametrize("name", ["one_item", "tiny"])
def test_more_tiles_than_items_bitwise_equal(gpu_available, name, monkeypatch):
    p = _one_item() if name == "one_item" else k2c.problem("tiny")
    out = []
    for setting in SETTINGS:
        h = _open(p, "huber", setting, monkeypatch)
        items, tiles = h.k2_info()["items"], h.solver_info()["pattern_tiles"]
        assert tiles > items and (name != "one_item" or items == 1), (items, tiles)
        h.save_state()
        rs = [h.solve_resident(restore=True, ftol=1e-14, xtol=1e-16, max_iter=3) for _ in range(2)]
        _path(h, setting)
        out.append((h.get_state(), tuple(_res(r) for r in rs)))
        h.close()
    assert out[0][1][0] == out[0][1][1]
    _same(out)
