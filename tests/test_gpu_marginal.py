"""GPU tests of the keyframe marginalisation (ptzba_marginal_prior / ptzba_set_marginal_prior: BAHandle.marginal_prior,
set_marginal_prior, ptzba.solve's and the drop-in's `marginal_prior=` / `marginalize=`, Map(marginalize=True)).

Reference: tests/marg_ref.py (pinned by test_marginal_cpu.py).  The cases -- config 1 E = [0], [3], [0, 1] and config 2
E = [0], [24, 25], the latter in the natural and the forced nested order -- are the smallest that cover a fixed E, a
free E, a mixed E, frames whose rows straddle a 32-row tile, the reversed part of a nested order and a K spread over
every tile.  Tolerances are the project's own: STEP_TOL of test_single_gauss_newton_step_is_exact, TOL of
test_gpu_covariance.py, the initial-cost tolerance of test_gpu_ba.py (fp64 1e-10, fp32 2e-6)."""
import functools

import numpy as np
import pytest

import cov_ref
import marg_ref
import prior_ref
from test_gpu_covariance import TOL

pytestmark = pytest.mark.gpu

STEP_TOL = {0: 1e-7, 1: 2e-3}  # test_gpu_ba.test_single_gauss_newton_step_is_exact's own
COST_TOL = {0: 1e-10, 1: 2e-6}  # test_gpu_ba.test_initial_cost_is_finite_and_matches_oracle's own
LOSS = {0: "linear", 1: "huber"}


@functools.lru_cache(maxsize=None)
def _ref(cfg, E, loss=0):
    p = prior_ref.problem(cfg)
    m = marg_ref.marginal(p, p.init_ptz, p.init_rays, E, loss=LOSS[loss], f_scale=1.0)[0]
    for a in (m.frames, m.lin, m.info, m.grad):
        a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _ref_identity(cfg, E):
    p = prior_ref.problem(cfg)
    out = marg_ref.step_identity(p, E, _ref(cfg, E))
    out[3].setflags(write=False)
    return out


def _handle(p, precision=0, ordering=0, loss=0, win=None, state=True):
    import ptzba
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=precision, ordering=ordering,
                  loss=loss, f_scale=1.0, frame_win_hi=win)
    if state:
        h.set_state(p.init_ptz, p.init_rays)
    return h


def marg_err(got, ref):
    """(Lambda error by cov_ref.block_err's correlation scaling, eta error max |d eta_i| / sqrt(Lambda_ii) relative to
    max |eta_i| / sqrt(Lambda_ii))."""
    d = np.sqrt(np.diag(ref.info))
    e_info = float(np.max(np.abs(got.info - ref.info) / np.outer(d, d)))
    e_grad = float(np.max(np.abs(got.grad - ref.grad) / d) / np.max(np.abs(ref.grad) / d))
    return e_info, e_grad


def _assert_marginal(got, ref, precision, what):
    assert got.frames.tolist() == ref.frames.tolist(), what
    np.testing.assert_array_equal(got.lin, ref.lin)
    e_info, e_grad = marg_err(got, ref)
    e_off = abs(got.offset - ref.offset) / ref.offset
    print(f"{what} precision {precision}: Lambda {e_info:.3e}, eta {e_grad:.3e} (tol {STEP_TOL[precision]:.0e}), "
          f"offset {e_off:.3e} (tol {COST_TOL[precision]:.0e})")
    assert np.array_equal(got.info, got.info.T)
    assert e_info < STEP_TOL[precision], e_info
    assert e_grad < STEP_TOL[precision], e_grad
    assert e_off <= COST_TOL[precision], e_off


CASES_1 = [("config1", (0,), 0, 0), ("config1", (3,), 0, 0), ("config1", (0, 1), 0, 0), ("config2", (0,), 0, 0),
           ("config2", (24, 25), 0, 0), ("config2", (0,), 2, 0), ("config2", (24, 25), 2, 0), ("config2", (0,), 0, 1)]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cfg,E,ordering,loss", CASES_1)
@pytest.mark.parametrize("precision", [0, 1])
def test_marginal_matches_reference(gpu_available, precision, cfg, E, ordering, loss):
    """Frames exact; Lambda, eta and the offset against marg_ref at the project's tolerances."""
    p = prior_ref.problem(cfg)
    ref = _ref(cfg, E, loss)
    h = _handle(p, precision, ordering, loss)
    if ordering == 2:
        assert h.solver_info()["ordering"] == "nested"
    got, stats = h.marginal_prior(list(E))
    h.close()
    import ptzba
    mask = ptzba.drop_mask(p.frame, E)
    assert stats["dropped_records"] == int(mask.sum())
    assert stats["dropped_landmarks"] == len(np.unique(p.landmark[mask != 0]))
    assert stats["absorbed"] == [] and not stats["marginal_absorbed"]
    free_E = [f for f in E if f >= 1]
    assert (stats["min_pivot"] > 0) == bool(free_E)
    _assert_marginal(got, ref, precision, f"{cfg} E={list(E)} ordering {ordering} loss {LOSS[loss]}")


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("cfg,E,precision", [(c, e, 0) for c, e in marg_ref.CASES] +
                         [("config1", (0,), 1), ("config1", (0, 1), 1), ("config2", (0,), 1)])
def test_step_identity_on_the_device(gpu_available, cfg, E, precision):
    """The marginal of p's handle, set on a handle of Q2 (p without D): one undamped step equals the reference step
    of the clone problem Q1 on the kept poses and the rays that still have records; the step without the marginal is
    at least 10 tolerances away.  A free frame of E keeps no record in Q2 and gets a unary prior, so it decouples."""
    import ptzba
    p = prior_ref.problem(cfg)
    _, moved, scale, ref, keepf, seen = _ref_identity(cfg, E)
    tol = STEP_TOL[precision]
    assert moved >= 10 * tol, moved
    h = _handle(p, precision)
    m, _ = h.marginal_prior(list(E))
    h.close()
    q2 = marg_ref.kept_problem(p, ptzba.drop_mask(p.frame, E))
    unary = [([f], p.init_ptz[f], np.diag(1.0 / prior_ref.SIGMA ** 2)) for f in E if f >= 1]
    win = ptzba.prior_window(p.n_pose, q2.frame, q2.landmark, unary + [m])
    h = _handle(q2, precision, win=win, state=False)
    if unary:
        h.set_pose_priors(unary)
    h.set_state(p.init_ptz, p.init_rays)
    h.set_marginal_prior(m)
    assert h.marginal_prior_info()[:2] == (len(m.frames), 3 * len(m.frames))
    h.linearize()
    h.build_reduced(0.0)
    h.solve_reduced()
    assert h.read_scalars()[5] == 0
    h.accept(True)
    ptz1, rays1 = h.get_state()
    h.close()
    dx = np.concatenate([(ptz1 - p.init_ptz)[keepf].reshape(-1), (rays1 - p.init_rays)[seen].reshape(-1)])
    err = np.abs(dx - ref).max() / scale
    print(f"{cfg} E={list(E)} precision {precision}: step identity {err:.3e} (tol {tol:.0e}); without the marginal "
          f"{moved:.3e}")
    assert err < tol, err


# ------------------------------------------------------------------------------------------------ 3
def test_absorbs_pose_prior_factors(gpu_available):
    """Config 1, E = [3]: a pair factor (3, 5), a unary on 7 (stays) and a unary on 3 -- factors 0 and 2 are absorbed
    whole, frame 5 is in K anyway, and the result equals marg_ref's."""
    import ptzba
    p = prior_ref.problem("config1")
    rng = np.random.default_rng(3)
    factors = [(np.array(fr, np.int32), (p.init_ptz[fr] + rng.uniform(-3, 3, (len(fr), 3)) * prior_ref.SIGMA).reshape(-1),
                prior_ref._spd(rng, fr)) for fr in ([3, 5], [7], [3])]
    ref, absorbed = marg_ref.marginal(p, p.init_ptz, p.init_rays, (3,), factors=factors)
    assert absorbed == [0, 2]
    plain = _ref("config1", (3,))
    assert marg_err(plain, ref)[0] > 1e-3  # the factors matter
    for precision in (0, 1):
        h = _handle(p, precision, win=ptzba.prior_window(p.n_pose, p.frame, p.landmark, factors), state=False)
        h.set_pose_priors(factors)
        h.set_state(p.init_ptz, p.init_rays)
        got, stats = h.marginal_prior([3])
        assert h.pose_prior_info()[0] == 3  # the handle keeps its factors
        h.close()
        assert stats["absorbed"] == [0, 2] and not stats["marginal_absorbed"]
        _assert_marginal(got, ref, precision, "config1 E=[3] with factors")


def test_absorbs_the_stored_marginal(gpu_available):
    """Sequential marginalisation: the marginal of E = [0] set on the handle of the remaining problem, then E = [1]:
    the stored marginal is absorbed, as marg_ref does it.  The joint E = [0, 1] is another function (a landmark seen by
    both leaving frames gets two clones)."""
    import ptzba
    p = prior_ref.problem("config1")
    h = _handle(p)
    m0, _ = h.marginal_prior([0])
    h.close()
    q2 = marg_ref.kept_problem(p, ptzba.drop_mask(p.frame, [0]))
    ref, absorbed = marg_ref.marginal(q2, p.init_ptz, p.init_rays, (1,), marg=m0)
    assert absorbed == ["m"] and 1 in m0.frames
    joint = _ref("config1", (0, 1))
    assert joint.frames.tolist() != ref.frames.tolist() or marg_err(joint, ref)[0] > 1e-6
    for precision in (0, 1):
        h = _handle(q2, precision, win=ptzba.prior_window(p.n_pose, q2.frame, q2.landmark, [m0]))
        h.set_marginal_prior(m0)
        got, stats = h.marginal_prior([1])
        assert h.marginal_prior_info()[0] == len(m0.frames)  # still set: replacing it is the caller's step
        h.close()
        assert stats["marginal_absorbed"] and stats["absorbed"] == []
        _assert_marginal(got, ref, precision, "config1 E=[0] then E=[1]")


# ------------------------------------------------------------------------------------------------ 4
def test_converged_solve_with_a_marginal(gpu_available):
    """Config 1, fp64, Q2 of E = [0] with its marginal: the device loop and the host loop take identical iterates,
    both stop at marg_ref.solve's optimum (1e-6 deg / 1e-4 px), and the reported cost is the records' cost + q(x)."""
    import ptzba
    p = prior_ref.problem("config1")
    m = _ref("config1", (0,))
    q2 = marg_ref.kept_problem(p, ptzba.drop_mask(p.frame, [0]))
    ptz_ref, rays_ref, c_ref = marg_ref.solve(q2, p.init_ptz, p.init_rays, marg=m)
    win = ptzba.prior_window(p.n_pose, q2.frame, q2.landmark, [m])
    seen = np.unique(q2.landmark)
    out = []
    for device_loop in (False, True):
        h = _handle(q2, win=win)
        h.set_marginal_prior(m)
        res = ptzba.LMSolver(h, ftol=1e-14, xtol=1e-14, max_iter=100, device_loop=device_loop).run()
        ptz, rays = h.get_state()
        q = h.marginal_prior_info()[3]
        h.linearize()
        c_with = h.read_scalars()[0]
        h.clear_marginal_prior()
        assert h.marginal_prior_info() == (0, 0, 0.0, 0.0)
        h.linearize()
        c_without = h.read_scalars()[0]
        h.close()
        assert abs(q - m.value(ptz)) <= 1e-12 * abs(q)
        assert abs(c_with - (c_without + m.value(ptz))) <= 1e-12 * c_with
        assert abs(res.cost - c_with) <= 1e-12 * c_with
        out.append((res, ptz, rays))
    (rh, ph, yh), (rd, pd, yd) = out
    print(rh, rd)
    assert rd.njev == rh.njev and rd.status == rh.status and rd.nfev == rh.nfev, (rh, rd)
    assert abs(rd.cost - rh.cost) <= 1e-12 * rh.cost
    np.testing.assert_allclose(pd, ph, rtol=0, atol=1e-10)
    np.testing.assert_allclose(yd, yh, rtol=0, atol=1e-10)
    for res, ptz, rays in out:
        np.testing.assert_allclose(ptz[:, :2], ptz_ref[:, :2], rtol=0, atol=1e-6)
        np.testing.assert_allclose(ptz[:, 2], ptz_ref[:, 2], rtol=0, atol=1e-4)
        np.testing.assert_allclose(rays[seen], rays_ref[seen], rtol=0, atol=1e-6)
        assert abs(res.cost - c_ref) <= 1e-9 * c_ref


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("precision", [0, 1])
def test_covariance_includes_the_marginal(gpu_available, precision):
    """Config 1 with the marginal of E = [3] set on the full problem's handle (pure algebra: the test does not care
    that this counts D twice): the covariance blocks are those of inv(H + Lambda), at test_gpu_covariance's TOL."""
    import ptzba
    p = prior_ref.problem("config1")
    m = _ref("config1", (3,))
    H = cov_ref.normal_matrix(p, p.init_ptz, p.init_rays)
    idx = marg_ref._rows3(m.frames)
    H0 = H.copy()
    H[np.ix_(idx, idx)] += m.info
    pose_ref, ray_ref = cov_ref._cut(np.linalg.inv(H), p.n_pose, p.n_landmark, 1)
    pose_plain = cov_ref._cut(np.linalg.inv(H0), p.n_pose, p.n_landmark, 1)[0]
    assert cov_ref.block_err(pose_plain, pose_ref) > 10 * TOL[precision]
    h = _handle(p, precision, win=ptzba.prior_window(p.n_pose, p.frame, p.landmark, [m]))
    h.set_marginal_prior(m)
    pose, ray, _ = h.covariance(landmarks="all")
    h.close()
    e_pose, e_ray = cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref)
    print(f"precision {precision}: pose blocks {e_pose:.3e}, ray blocks {e_ray:.3e} (tol {TOL[precision]:.0e})")
    assert e_pose < TOL[precision] and e_ray < TOL[precision]


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("precision,loss", [(0, 0), (1, 1)])
def test_leaves_no_trace(gpu_available, precision, loss):
    """After marginal_prior the state is unchanged and a solve is bitwise the solve without the call; set then clear,
    then solve: bitwise equal; two calls give bitwise equal Lambda and eta."""
    import ptzba
    p = prior_ref.problem("config1")
    m_set = _ref("config1", (3,))
    win = ptzba.prior_window(p.n_pose, p.frame, p.landmark, [m_set])

    def run(prepare):
        h = _handle(p, precision, loss=loss, win=win)
        extra = prepare(h)
        res = ptzba.LMSolver(h, max_iter=8).run()
        ptz, rays = h.get_state()
        h.close()
        return res, ptz, rays, extra

    def call_twice(h):
        a, _ = h.marginal_prior([3])
        ptz, rays = h.get_state()
        np.testing.assert_array_equal(ptz, p.init_ptz)
        np.testing.assert_array_equal(rays, p.init_rays)
        b, _ = h.marginal_prior([3])
        assert np.array_equal(a.info, b.info) and np.array_equal(a.grad, b.grad) and a.offset == b.offset
        return a

    def set_clear(h):
        h.set_marginal_prior(m_set)
        h.clear_marginal_prior()

    base = run(lambda h: None)
    for prepare in (call_twice, set_clear):
        got = run(prepare)
        assert got[0].cost == base[0].cost and got[0].nfev == base[0].nfev and got[0].njev == base[0].njev
        np.testing.assert_array_equal(got[1], base[1])
        np.testing.assert_array_equal(got[2], base[2])
    # ... and after a solve, at the solution, twice the same again
    h = _handle(p, precision, loss=loss)
    ptzba.LMSolver(h, max_iter=8).run()
    a, _ = h.marginal_prior([0, 1])
    b, _ = h.marginal_prior([0, 1])
    h.close()
    assert np.array_equal(a.info, b.info) and np.array_equal(a.grad, b.grad) and a.offset == b.offset


# ------------------------------------------------------------------------------------------------ 7
def test_marginal_prior_refusals(gpu_available):
    """Every refusal has its message and leaves the handle as it was: the same call afterwards gives the same bits."""
    import ptzba
    import synthetic
    p = prior_ref.problem("config2")
    h = _handle(p)
    before, _ = h.marginal_prior([24, 25])
    mask = ptzba.drop_mask(p.frame, [0])

    def refused(match, *a, **kw):
        with pytest.raises(ptzba.PtzbaError, match=match):
            h.marginal_prior(*a, **kw)

    refused("9 free leaving frames", list(range(1, 10)))
    refused("mask has", [0], mask[:-2])
    refused("out of range", [50])
    refused("out of range", [-1])
    refused("named twice", [3, 3])
    refused("nothing to marginalise", [0], np.zeros_like(mask))
    refused("unknown struct_size", [0], _struct_size=8)
    # frame 3 leaves, but none of its records is dropped and no factor names it
    refused("leaving frame 3 is not determined", [0, 3], mask & (1 - ptzba.drop_mask(p.frame, [3])))
    h.linearize()
    h.build_reduced(1e-3)
    h.solve_reduced()
    refused("trial is pending", [0])
    h.accept(False)
    ptz, rays = h.get_state()
    np.testing.assert_array_equal(ptz, p.init_ptz)
    np.testing.assert_array_equal(rays, p.init_rays)
    after, _ = h.marginal_prior([24, 25])
    h.close()
    assert np.array_equal(after.info, before.info) and np.array_equal(after.grad, before.grad)
    # |K| > 64: 80 keyframes, every record dropped
    big = synthetic.make_small_problem(80, 800, 30.0, 70.0, seed=0)
    assert len(np.unique(big.frame)) > 66
    h = _handle(big)
    with pytest.raises(ptzba.PtzbaError, match="at most 64"):
        h.marginal_prior([0], np.ones(len(big.frame), np.uint8))
    h.close()


def test_set_marginal_prior_refusals(gpu_available):
    import ptzba
    p = prior_ref.problem("config2")
    h = _handle(p)  # the records' own coupling window
    good = _ref("config2", (0,))
    win_ok = ptzba.prior_window(p.n_pose, p.frame, p.landmark, [good])
    ok = ptzba.Marginal([1, 2], p.init_ptz[[1, 2]], np.eye(6), np.zeros(6), 0.0)

    def variant(**kw):
        m = ptzba.Marginal(ok.frames, ok.lin, ok.info, ok.grad, ok.offset)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def refused(match, m, **kw):
        with pytest.raises(ptzba.PtzbaError, match=match):
            h.set_marginal_prior(m, _raw=True, **kw)
        assert h.marginal_prior_info()[0] == 2

    h.set_marginal_prior(ok)
    refused("not a free frame", variant(frames=np.array([0, 2], np.int32)))
    refused("not a free frame", variant(frames=np.array([1, 50], np.int32)))
    refused("named twice", variant(frames=np.array([2, 2], np.int32)))
    bad = ok.info.copy()
    bad[0, 1] = np.nan
    refused("non-finite", variant(info=bad))
    refused("non-finite", variant(grad=np.full(6, np.inf)))
    bad = ok.info.copy()
    bad[0, 1] = 1e-6
    refused("not symmetric", variant(info=bad))
    bad = ok.info.copy()
    bad[2, 2] = -1.0
    refused("negative diagonal", variant(info=bad))
    refused("coupling window", ptzba.Marginal([1, 45], p.init_ptz[[1, 45]], np.eye(6), np.zeros(6), 0.0))
    refused("unknown struct_size", ok, _struct_size=16)
    with pytest.raises(ValueError, match="positive semi-definite"):
        h.set_marginal_prior(variant(info=np.diag([1.0, 1, 1, 1, 1, -1e-3])))
    if not np.array_equal(win_ok, ptzba.frame_coupling_window(p.n_pose, p.frame, p.landmark)):
        refused("coupling window", good)
    # asymmetry within 1e-12 max|Lambda| is symmetrised
    tiny = ok.info.copy()
    tiny[0, 1] = 1e-13
    h.set_marginal_prior(variant(info=tiny), _raw=True)
    # with a marginal set, an exchange cannot be attached; a handle with a hook takes no marginal and computes none
    with pytest.raises(ptzba.PtzbaError, match="marginal prior"):
        h.set_exchange_hook(lambda kind, ptr, count, stream: None)
    h.set_marginal_prior(None)
    assert h.marginal_prior_info() == (0, 0, 0.0, 0.0)
    h.set_exchange_hook(lambda kind, ptr, count, stream: None)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        h.set_marginal_prior(ok)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        h.marginal_prior([0])
    h.set_exchange_hook(None)
    h.set_marginal_prior(ok)
    assert h.marginal_prior_info()[0] == 2
    h.close()
    p1 = prior_ref.problem("config1")
    g = ptzba.BAHandle(0)
    g.set_problem(p1.n_pose, p1.n_landmark, p1.frame, p1.landmark, p1.xy, p1.u, p1.v, dist_world=2, dist_rank=0,
                  frame_win_hi=ptzba.frame_coupling_window(p1.n_pose, p1.frame, p1.landmark))
    g.set_state(p1.init_ptz, p1.init_rays)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        g.marginal_prior([0])
    g.close()


# ------------------------------------------------------------------------------------------------ 8
CENTER, ROT = np.array([0.0, -10.0, 5.0]), np.eye(3)


class _SyntheticCalls:
    """SyntheticFrontEnd installed as the front-end hooks, and ptzba.solve's arguments recorded per call."""

    def __init__(self, scene):
        self.scene = scene
        self.solves = []

    def __enter__(self):
        import image_process
        import ptzba
        import synthetic
        self.saved = image_process.detect_compute_sift, image_process.match_sift_features, ptzba.solve
        synthetic.SyntheticFrontEnd(self.scene).install()
        real = ptzba.solve

        def solve(*a, **kw):
            self.solves.append((a, kw))
            return real(*a, **kw)
        ptzba.solve = solve
        return self

    def __exit__(self, *exc):
        import image_process
        import ptzba
        image_process.detect_compute_sift, image_process.match_sift_features, ptzba.solve = self.saved


def _poses(kfs):
    return np.array([[k.pan, k.tilt, k.f] for k in kfs])


def test_dropin_against_the_handle_level(gpu_available):
    """bundle_adjustment(marginalize=[first image]) returns the marginal BAHandle.marginal_prior gives on the same
    records at the same solution, keyed by image index; bundle_adjustment(marginal_prior=that) over the images that
    stay takes the handle-level solve's poses -- both bitwise.  A key outside the call raises ValueError."""
    import random
    import bundle_adjustment as ba
    import ptzba
    import synthetic
    sc = synthetic.make_scene(6, 150, 54, 63, seed=1)
    lm_kw = dict(ftol=1e-10, xtol=1e-12, max_iter=50)
    with _SyntheticCalls(sc) as calls:
        random.seed(1)
        plain = ba.bundle_adjustment(list(range(6)), list(range(100, 106)), "sift", sc.init_ptz.copy(), CENTER, ROT, sc.u,
                                     sc.v, "", **lm_kw)
        random.seed(1)
        lm, kfs, mo = ba.bundle_adjustment(list(range(6)), list(range(100, 106)), "sift", sc.init_ptz.copy(), CENTER, ROT,
                                           sc.u, sc.v, "", marginalize=[100], **lm_kw)
        assert len(plain) == 2
        np.testing.assert_array_equal(_poses(plain[1]), _poses(kfs))  # the keyword leaves the solve alone
        np.testing.assert_array_equal(plain[0], lm)
        m = mo["marginal"]
        assert mo["stats"]["dropped_records"] > 0 and len(m.frames) >= 2 and m.frames.min() > 100
        # the same at the handle level
        (N, n_lm, frame, lmk, xy, u, v, ptz0, rays0), _ = calls.solves[-1]
        h = ptzba.BAHandle(0)
        h.set_problem(N, n_lm, frame, lmk, xy, u, v)
        h.set_state(ptz0, rays0)
        ptzba.LMSolver(h, **lm_kw).run()
        ptz_h, _ = h.get_state()
        m_h, _ = h.marginal_prior([0])
        h.close()
        np.testing.assert_array_equal(ptz_h[1:], _poses(kfs)[1:])
        assert (m_h.frames + 100).tolist() == m.frames.tolist()
        assert np.array_equal(m_h.info, m.info) and np.array_equal(m_h.grad, m.grad) and m_h.offset == m.offset
        np.testing.assert_array_equal(m_h.lin, m.lin)
        # the next window: images 101..105 from the adjusted poses, with and without the marginal
        ptz1 = _poses(kfs)[1:]
        with pytest.raises(ValueError, match="not among image_indices"):
            ba.bundle_adjustment(list(range(2, 6)), list(range(102, 106)), "sift", ptz1[1:].copy(), CENTER, ROT, sc.u,
                                 sc.v, "", marginal_prior=m, **lm_kw)
        outs = []
        for kw in ({}, dict(marginal_prior=m)):
            random.seed(2)
            outs.append(ba.bundle_adjustment(list(range(1, 6)), list(range(101, 106)), "sift", ptz1.copy(), CENTER, ROT,
                                             sc.u, sc.v, "", **kw, **lm_kw))
        assert np.abs(_poses(outs[0][1]) - _poses(outs[1][1])).max() > 1e-6  # the marginal pulls
        (N, n_lm, frame, lmk, xy, u, v, ptz0, rays0), _ = calls.solves[-1]
        m_loc = m.reindex({101 + i: i for i in range(5)})
        h = ptzba.BAHandle(0)
        h.set_problem(N, n_lm, frame, lmk, xy, u, v, frame_win_hi=ptzba.prior_window(N, frame, lmk, [m_loc]))
        h.set_state(ptz0, rays0)
        h.set_marginal_prior(m_loc)  # (frame 0 conditioned at the state)
        ptzba.LMSolver(h, **lm_kw).run()
        ptz_h, rays_h = h.get_state()
        h.close()
        np.testing.assert_array_equal(ptz_h[1:], _poses(outs[1][1])[1:])
        np.testing.assert_array_equal(rays_h, outs[1][0])


def test_map_marginalize_equals_hand_replay(gpu_available):
    """Map("sift", max_ba_frame=4, marginalize=True) over 7 synthetic keyframes against the sequence of
    bundle_adjustment calls replayed by hand (merge the leaving keyframe's marginal once it has left, condition on
    every keyframe outside the window at its kept pose): every pose and ray bitwise.  The marginal changes the map."""
    import random
    import bundle_adjustment as ba
    import ptzba
    import scene_map
    import synthetic
    from correspondence import CorrespondenceCache
    from key_frame import KeyFrame
    sc = synthetic.make_scene(7, 160, 52, 64, seed=2)
    W = 4

    def kf(k):
        return KeyFrame(k, 300 + k, CENTER, ROT, sc.u, sc.v, *sc.init_ptz[k])

    def run_map(marginalize):
        random.seed(3)
        m = scene_map.Map("sift", max_ba_frame=W, marginalize=marginalize)
        m.add_first_keyframe(kf(0))
        steps = []
        for k in range(1, 7):
            m.add_keyframe_with_ba(kf(k), "")
            steps.append((_poses(m.keyframe_list), m.global_ray.copy()))
        return m, steps

    with _SyntheticCalls(sc) as calls:
        m_on, on = run_map(True)
        n_marg = sum(1 for _, kw in calls.solves if kw.get("marginal_prior") is not None)
        n_ask = sum(1 for _, kw in calls.solves if kw.get("marginalize") is not None)
        assert n_ask == 4 and n_marg == 3, (n_ask, n_marg)  # full windows at keyframes 3..6; a prior from 4 on
        _, off = run_map(False)
        assert m_on.marginal_carry.stored is not None and m_on.marginal_carry.stored.frames.min() >= 303
        assert max(np.abs(a[0] - b[0]).max() for a, b in zip(on, off)) > 1e-6
        for a, b in zip(on[:3], off[:3]):  # ... from the first call with a prior on
            np.testing.assert_array_equal(a[0], b[0])
        # the hand replay
        random.seed(3)
        cache = CorrespondenceCache()
        kfl = [kf(0)]
        cache.prepare(kfl[0].img_index, kfl[0].img, "sift")
        stored, pending, poses = None, None, {}
        for k in range(1, 7):
            ref = kfl[0]
            kfl.append(kf(k))
            kept = []
            if len(kfl) > W:
                kept, kfl = kfl[:-W], kfl[-W:]
                cache.retain([q.img_index for q in kfl])
            idx = [q.img_index for q in kfl]
            for q in kept + kfl[:-1]:
                poses[q.img_index] = (q.pan, q.tilt, q.f)
            if pending is not None and pending[0] not in idx:
                stored = ptzba.merge_marginals(stored, pending[1])
            pending = None
            if stored is not None:
                gone = [int(f) for f in stored.frames if int(f) not in idx]
                if gone:
                    stored = stored.condition(gone, np.array([poses[f] for f in gone]))
            kw = dict(marginal_prior=stored)
            if len(kfl) == W:
                kw["marginalize"] = [idx[0]]
            out = ba.bundle_adjustment([q.img for q in kfl], idx, "sift", _poses(kfl), ref.center, ref.base_rotation,
                                       ref.u, ref.v, "", False, correspondences=cache, **kw)
            kfl = kept + [q for q in out[1] if q.has_features()]
            for q in out[1]:
                poses[q.img_index] = (q.pan, q.tilt, q.f)
            if len(idx) == W:
                pending = (idx[0], out[-1]["marginal"])
            np.testing.assert_array_equal(_poses(kfl), on[k - 1][0])
            np.testing.assert_array_equal(out[0], on[k - 1][1])
