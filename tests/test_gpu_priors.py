"""GPU tests of the Gaussian pose priors (ptzba_set_pose_priors: BAHandle.set_pose_priors, ptzba.solve's and the
drop-in's `pose_priors=`).

Reference (tests/prior_ref.py, pinned to scipy by test_priors_cpu.py): the oracle's residual and analytic Jacobian plus
the dense prior terms P = sum info_k, P e.  One factor set per problem (prior_ref.factor_set): a unary prior on the
first free frame and on the last frame, an adjacent pair and a dense G = 3 factor (listed out of order) that share a
frame, and at config 2 the pairs (11, 12) / (15, 16), whose system rows straddle a 32-row tile boundary in the natural
(rows 30-32) / forced nested order (rows 94-96), the pair (47, 48), which the nested order reverses (transposed block),
and the pair (1, 45), outside the records' coupling window (the window is raised for it by prior_window).  sigma =
0.02 deg / 2 px, means up to 10 sigma off the initial poses."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

import prior_ref
from test_gpu_covariance import TOL

pytestmark = pytest.mark.gpu

C2_PAIRS, C2_FAR = prior_ref.CONFIG2_PAIRS, prior_ref.CONFIG2_FAR
STEP_TOL = {0: 1e-7, 1: 2e-3}  # test_gpu_ba.test_single_gauss_newton_step_is_exact's own


@functools.lru_cache(maxsize=None)
def _case(cfg):
    import ptzba
    p = prior_ref.problem(cfg)
    c2 = cfg == "config2"
    factors = prior_ref.factor_set(p, C2_PAIRS if c2 else (), C2_FAR if c2 else None)
    win = ptzba.prior_window(p.n_pose, p.frame, p.landmark, factors)
    win.setflags(write=False)
    return p, factors, win


def _handle(cfg, precision=0, ordering=0, loss=0, f_scale=1.0, priors=True):
    import ptzba
    p, factors, win = _case(cfg)
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=precision, ordering=ordering,
                  loss=loss, f_scale=f_scale, frame_win_hi=win)
    if priors:
        h.set_pose_priors(factors)
    h.set_state(p.init_ptz, p.init_rays)
    return h


def _n_blocks(factors):
    return len({(min(a, b), max(a, b)) for fr, _, _ in factors for a in fr.tolist() for b in fr.tolist()})


@functools.lru_cache(maxsize=None)
def _ref_steps(cfg):
    """(dx with priors, dx without) of one undamped Gauss-Newton step at the initial state."""
    p, factors, _ = _case(cfg)
    dx1 = prior_ref.gn_step(p, p.init_ptz, p.init_rays, factors)[0]
    dx0 = prior_ref.gn_step(p, p.init_ptz, p.init_rays, [])[0]
    dx1.setflags(write=False)
    dx0.setflags(write=False)
    return dx1, dx0


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cfg,ordering", [("config1", 0), ("config2", 0), ("config2", 2)])
@pytest.mark.parametrize("precision", [0, 1])
def test_gauss_newton_step_with_priors_is_exact(gpu_available, precision, cfg, ordering):
    """One undamped step == the dense solve of (H + P) dx = -(g + P e), to test_single_gauss_newton_step_is_exact's
    tolerance; the reference step without the priors is at least 10 tolerances away, so a build that dropped them
    (or any one kind of block: the far pair, the transposed one, a straddling frame) could not pass."""
    p, factors, _ = _case(cfg)
    dx, dx_plain = _ref_steps(cfg)
    tol = STEP_TOL[precision]
    moved = np.abs(dx - dx_plain).max() / np.abs(dx).max()
    assert moved >= 10 * tol, moved
    h = _handle(cfg, precision, ordering)
    if ordering == 2:
        assert h.solver_info()["ordering"] == "nested"
    h.linearize()
    h.build_reduced(0.0)
    h.solve_reduced()
    s = h.read_scalars()
    assert s[5] == 0
    h.accept(True)
    ptz1, rays1 = h.get_state()
    h.close()
    dx_gpu = np.concatenate([(ptz1 - p.init_ptz)[1:].reshape(-1), (rays1 - p.init_rays).reshape(-1)])
    err = np.abs(dx_gpu - dx).max() / np.abs(dx).max()
    print(f"{cfg} ordering {ordering} precision {precision}: step error {err:.3e} (tol {tol:.0e}); priors move the "
          f"step by {moved:.3e}")
    assert err < tol, err


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("cfg", ["config1", "config2"])
def test_prior_cost(gpu_available, cfg):
    """pose_prior_info: the counts, and the prior cost == numpy's 1/2 e^T info e (1e-12 relative); the cost
    linearize() reports with the priors minus the one after clearing them is that cost (1e-9 of the total, fp64)."""
    p, factors, _ = _case(cfg)
    h = _handle(cfg)
    n_f, n_row, n_blk, c = h.pose_prior_info()
    ref = prior_ref.prior_cost(factors, p.init_ptz)
    assert (n_f, n_row, n_blk) == (len(factors), sum(3 * len(f[0]) for f in factors), _n_blocks(factors))
    print(f"{cfg}: prior cost {c!r} vs {ref!r}")
    assert ref > 0 and abs(c - ref) <= 1e-12 * ref
    h.linearize()
    with_p = h.read_scalars()[0]
    h.clear_pose_priors()
    assert h.pose_prior_info() == (0, 0, 0, 0.0)
    h.linearize()
    without = h.read_scalars()[0]
    h.close()
    assert abs((with_p - without) - ref) <= 1e-9 * with_p, (with_p, without, ref)
    assert abs(without - prior_ref.cost(p, p.init_ptz, p.init_rays, [])) <= 1e-9 * without


def test_prior_cost_many_factors(gpu_available):
    """A unary prior on every free frame of config 2 plus a relative-pose prior (info = [[W, -W], [-W, W]], rank 3
    of 6) on every consecutive pair: 97 factors, 435 prior rows, so the cost is summed over more than one workgroup.
    Cost vs numpy (1e-12), bitwise repeatable, and the undamped step still exact (1e-7)."""
    import ptzba
    p = prior_ref.problem("config2")
    rng = np.random.default_rng(5)
    W = np.diag(1.0 / prior_ref.SIGMA ** 2)
    R = np.block([[W, -W], [-W, W]])
    factors = [([f], p.init_ptz[f] + rng.uniform(-3, 3, 3) * prior_ref.SIGMA, W) for f in range(1, p.n_pose)]
    factors += [([f, f + 1], (p.init_ptz[[f, f + 1]] + rng.uniform(-3, 3, (2, 3)) * prior_ref.SIGMA).reshape(-1), R)
                for f in range(1, p.n_pose - 1)]
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v)  # (consecutive frames are coupled)
    h.set_pose_priors(factors)
    h.set_state(p.init_ptz, p.init_rays)
    info = h.pose_prior_info()
    ref = prior_ref.prior_cost(factors, p.init_ptz)
    assert info[:3] == (97, 435, 49 + 48) and abs(info[3] - ref) <= 1e-12 * ref, (info, ref)
    assert h.pose_prior_info() == info
    h.linearize()
    c0 = h.read_scalars()[0]
    h.build_reduced(0.0)
    h.solve_reduced()
    s = h.read_scalars()
    assert s[5] == 0
    h.accept(True)
    ptz1, rays1 = h.get_state()
    h.close()
    assert abs(c0 - prior_ref.cost(p, p.init_ptz, p.init_rays, factors)) <= 1e-9 * c0
    assert abs(s[1] - prior_ref.cost(p, ptz1, rays1, factors)) <= 1e-9 * s[1]  # the trial cost includes the prior
    dx = prior_ref.gn_step(p, p.init_ptz, p.init_rays, factors)[0]
    dx_gpu = np.concatenate([(ptz1 - p.init_ptz)[1:].reshape(-1), (rays1 - p.init_rays).reshape(-1)])
    err = np.abs(dx_gpu - dx).max() / np.abs(dx).max()
    print(f"97 factors: prior cost {info[3]!r} vs {ref!r}; step error {err:.3e}")
    assert err < 1e-7, err


# ------------------------------------------------------------------------------------------------ 3
def test_converged_solve_device_and_host_loops(gpu_available):
    """Config 1, fp64, linear: the device loop and the host loop take identical iterates (the assertions of
    test_device_loop_equals_host_loop) and both stop at prior_ref's optimum (1e-6 deg / 1e-4 px); the reported cost
    includes the prior."""
    import ptzba
    p, factors, _ = _case("config1")
    ptz_ref, rays_ref, c_ref = prior_ref.solve(p, p.init_ptz, p.init_rays, factors)
    out = []
    for device_loop in (False, True):
        h = _handle("config1")
        res = ptzba.LMSolver(h, ftol=1e-14, xtol=1e-14, max_iter=100, device_loop=device_loop).run()
        ptz, rays = h.get_state()
        out.append((res, ptz, rays))
        h.close()
    (rh, ph, yh), (rd, pd, yd) = out
    print(rh, rd)
    assert rd.njev == rh.njev and rd.status == rh.status and rd.nfev == rh.nfev, (rh, rd)
    assert abs(rd.cost - rh.cost) <= 1e-12 * rh.cost
    np.testing.assert_allclose(pd, ph, rtol=0, atol=1e-10)
    np.testing.assert_allclose(yd, yh, rtol=0, atol=1e-10)
    for res, ptz, rays in out:
        np.testing.assert_allclose(ptz[:, :2], ptz_ref[:, :2], rtol=0, atol=1e-6)
        np.testing.assert_allclose(ptz[:, 2], ptz_ref[:, 2], rtol=0, atol=1e-4)
        np.testing.assert_allclose(rays, rays_ref, rtol=0, atol=1e-6)
        assert abs(res.cost - c_ref) <= 1e-9 * c_ref
        assert abs(res.initial_cost - prior_ref.cost(p, p.init_ptz, p.init_rays, factors)) <= 1e-9 * res.initial_cost


def test_converged_solve_config2_fp32_huber(gpu_available):
    """Config 2, fp32, Huber, through ptzba.solve(pose_priors=...): the solve stops at prior_ref's stationary point
    of the Huber objective with priors (pose RMSE <= 1e-4, the project's gate).  That point is recorded
    (tests/golden/priors_config2_huber.npz, prior_ref.config2_huber_point) and its stationarity re-checked here; it is
    not the optimum without priors (tests/golden/config2_optimum.npz)."""
    import ptzba
    import synthetic
    p, factors, _ = _case("config2")
    xt = golden("config2_optimum.npz")["x_tight_huber"]
    ptz_plain = np.concatenate([p.init_ptz[0], xt[:3 * (p.n_pose - 1)]]).reshape(-1, 3)
    golden(prior_ref.CONFIG2_HUBER)
    ptz_ref, _, c_ref = prior_ref.config2_huber_point(os.path.join(GOLDEN, prior_ref.CONFIG2_HUBER))
    assert np.any(synthetic.pose_rmse(ptz_ref, ptz_plain) > 1e-3)
    ptz, rays, res = ptzba.solve(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, p.init_ptz, p.init_rays,
                                 precision=ptzba.FP32, loss=ptzba.LOSS_HUBER, f_scale=1.0, ftol=1e-12, xtol=1e-12,
                                 max_iter=100, pose_priors=factors, keep_handle=False)
    rmse = synthetic.pose_rmse(ptz, ptz_ref)
    print(f"config2 fp32 huber with priors: {res}; pose RMSE {rmse}; cost {res.cost!r} vs {c_ref!r}")
    assert np.all(rmse <= 1e-4), rmse
    assert abs(res.cost - c_ref) <= 1e-5 * c_ref


# ------------------------------------------------------------------------------------------------ 4
def test_unobserved_frame(gpu_available):
    """Config 1 without frame 6's records: singular without a prior (covariance() fails as before), well posed with a
    unary prior on frame 6 -- the solve converges with frame 6 at the prior mean (1e-9) and covariance() returns
    info^-1 for it (1e-7, correlation-scaled)."""
    import ptzba
    import cov_ref
    p = prior_ref.problem("config1")
    keep = p.frame != 6
    rng = np.random.default_rng(3)
    A = rng.standard_normal((3, 3))
    s = 1.0 / prior_ref.SIGMA
    info = (A @ A.T / 3 + np.eye(3)) * np.outer(s, s)
    info = 0.5 * (info + info.T)
    mu = p.init_ptz[6] + np.array([0.05, -0.03, 4.0])
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame[keep], p.landmark[keep], p.xy[keep], p.u, p.v)
    h.set_pose_priors([([6], mu, info)])
    h.set_state(p.init_ptz, p.init_rays)
    res = ptzba.LMSolver(h, ftol=1e-14, xtol=1e-14, max_iter=100).run()
    ptz, _ = h.get_state()
    print(res, ptz[6] - mu)
    assert res.status > 0, res
    assert np.abs(ptz[6] - mu).max() <= 1e-9
    pose, _, cinfo = h.covariance()
    err = cov_ref.block_err(pose[6:7], np.linalg.inv(info)[None])
    print(f"frame 6 block vs info^-1: {err:.3e}; {cinfo}")
    assert err <= 1e-7
    assert cinfo["n_free"] == 3 * (p.n_pose - 1) + 2 * p.n_landmark
    h.clear_pose_priors()
    with pytest.raises(ptzba.PtzbaError, match="not positive definite"):
        h.covariance()
    h.close()


# ------------------------------------------------------------------------------------------------ 5
@functools.lru_cache(maxsize=None)
def _ref_cov(cfg):
    import cov_ref
    p, factors, _ = _case(cfg)
    H = prior_ref.normal_matrix(p, p.init_ptz, p.init_rays, factors)
    pose, ray = cov_ref._cut(np.linalg.inv(H), p.n_pose, p.n_landmark, 1)
    pose.setflags(write=False)
    ray.setflags(write=False)
    return pose, ray


@pytest.mark.parametrize("cfg,ordering,precision", [("config1", 0, 0), ("config1", 0, 1), ("config2", 2, 0)])
def test_covariance_blocks_match_inverse_with_priors(gpu_available, cfg, ordering, precision):
    """covariance() == the blocks of inv(H + P) (test_gpu_covariance's metric and TOL), and not those of inv(H)."""
    import cov_ref
    p, factors, _ = _case(cfg)
    pose_ref, ray_ref = _ref_cov(cfg)
    h = _handle(cfg, precision, ordering)
    idx = np.arange(p.n_landmark) if cfg == "config1" else np.arange(0, p.n_landmark, 32)
    pose, ray, info = h.covariance(idx)
    # scale "residual": (sum r^2 + sum e^T info e) / (2 R + prior rows - n_free)
    _, _, info_s = h.covariance(None, scale="residual")
    h.close()
    ep, er = cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref[idx])
    print(f"{cfg} ordering {ordering} precision {precision}: pose {ep:.3e} ray {er:.3e} (tol {TOL[precision]:.0e})")
    assert ep <= TOL[precision] and er <= TOL[precision], (ep, er)
    plain = cov_ref.synthetic_reference(cfg)[1]
    assert cov_ref.block_err(pose_ref, plain) > 100 * TOL[precision]  # the priors show in the reference
    n_free = 3 * (p.n_pose - 1) + 2 * p.n_landmark
    rows = sum(3 * len(f[0]) for f in factors)
    s2 = 2.0 * prior_ref.cost(p, p.init_ptz, p.init_rays, factors) / (2 * len(p.frame) + rows - n_free)
    assert abs(info_s["scale"] - s2) <= (1e-9 if precision == 0 else 1e-4) * s2, (info_s, s2)


# ------------------------------------------------------------------------------------------------ 6
def test_no_trace(gpu_available):
    """Priors set and cleared leave no trace: the solve is bitwise that of a handle that never had any (state, cost,
    iterations); set_problem clears them; two solves with the same priors are bitwise equal."""
    import ptzba
    p, factors, win = _case("config2")

    def run(h):
        h.set_state(p.init_ptz, p.init_rays)
        res = ptzba.LMSolver(h, ftol=1e-10, xtol=1e-12, max_iter=30).run()
        ptz, rays = h.get_state()
        return ptz.tobytes(), rays.tobytes(), res.cost, res.njev, res.nfev, res.status

    fresh = _handle("config2", precision=1, loss=1, priors=False)
    a = run(fresh)
    fresh.close()
    h = _handle("config2", precision=1, loss=1)
    with_1 = run(h)
    with_2 = run(h)
    assert with_1 == with_2
    assert with_1[0] != a[0]
    h.clear_pose_priors()
    b = run(h)
    assert b == a
    h.set_pose_priors(factors)
    assert h.pose_prior_info()[0] == len(factors)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=1, loss=1, frame_win_hi=win)
    assert h.pose_prior_info() == (0, 0, 0, 0.0)
    c = run(h)
    h.close()
    assert c == a


# ------------------------------------------------------------------------------------------------ 7
def _native_set(h, groups, means, infos, struct_size=None):
    """ptzba_set_pose_priors straight through ctypes (no Python-side validation); returns (rc, message)."""
    import ptzba
    begin = np.zeros(len(groups) + 1, np.int32)
    begin[1:] = np.cumsum([len(g) for g in groups])
    frames = np.ascontiguousarray(np.concatenate([np.asarray(g, np.int32) for g in groups]) if groups else [], np.int32)
    mean = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float64).reshape(-1) for m in means]))
    info = np.ascontiguousarray(np.concatenate([np.asarray(i, np.float64).reshape(-1) for i in infos]))
    pr = ptzba.ptzba_pose_priors(ctypes.sizeof(ptzba.ptzba_pose_priors) if struct_size is None else struct_size,
                                 len(groups), begin.ctypes.data, frames.ctypes.data, mean.ctypes.data, info.ctypes.data)
    rc = ptzba.lib().ptzba_set_pose_priors(h.h, ctypes.byref(pr))
    return rc, ptzba.lib().ptzba_last_error().decode()


def test_refusals(gpu_available):
    """Every refusal of ptzba_set_pose_priors, each with its message and the handle's priors left as they were."""
    import ptzba
    p, factors, win = _case("config2")
    h = ptzba.BAHandle(0)
    # the records' own window: (1, 45) is outside it
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, n_fixed=2)
    h.set_state(p.init_ptz, p.init_rays)
    near = [f for f in factors if tuple(f[0]) != C2_FAR and 1 not in f[0]]  # (frame 1 is fixed on this handle)
    h.set_pose_priors(near)
    before = h.pose_prior_info()
    assert before[0] == len(near)
    eye, z3 = np.eye(3), np.zeros(3)
    asym = eye.copy()
    asym[0, 1] = 1e-9
    cases = [
        ("not a free frame", [[1]], [z3], [eye]),  # < n_fixed
        ("not a free frame", [[0]], [z3], [eye]),
        ("not a free frame", [[p.n_pose]], [z3], [eye]),
        ("not a free frame", [[-1]], [z3], [eye]),
        ("twice", [[5, 5]], [np.zeros(6)], [np.eye(6)]),
        ("1..8 allowed", [list(range(2, 11))], [np.zeros(27)], [np.eye(27)]),
        ("1..8 allowed", [[3], []], [z3], [eye]),
        ("non-finite mean", [[5]], [np.array([0.0, np.inf, 0.0])], [eye]),
        ("non-finite information", [[5]], [z3], [np.diag([1.0, np.nan, 1.0])]),
        ("negative diagonal", [[5]], [z3], [np.diag([1.0, -1e-3, 1.0])]),
        ("not symmetric", [[5]], [z3], [asym]),
        ("frames 2 and 45", [[2, 45]], [np.zeros(6)], [np.eye(6)]),
        ("frames 2 and 45", [[45, 2]], [np.zeros(6)], [np.eye(6)]),
    ]
    for needle, groups, means, infos in cases:
        rc, msg = _native_set(h, groups, means, infos)
        assert rc != 0 and needle in msg, (needle, rc, msg)
        assert h.pose_prior_info() == before, needle
    rc, msg = _native_set(h, [[2, 45]], [np.zeros(6)], [np.eye(6)])
    assert "frame_win_hi" in msg
    rc, msg = _native_set(h, [[5]], [z3], [eye], struct_size=24)
    assert rc != 0 and "struct_size" in msg and h.pose_prior_info() == before
    # the Python layer passes the library's refusal on
    with pytest.raises(ptzba.PtzbaError, match="frame_win_hi"):
        h.set_pose_priors([([2, 45], np.zeros(6), np.eye(6))])
    assert h.pose_prior_info() == before
    # asymmetry within 1e-12 max|info| is symmetrised, not refused
    tiny = eye.copy()
    tiny[0, 1] = 5e-13
    rc, msg = _native_set(h, [[5]], [p.init_ptz[5] + 1.0], [tiny])
    assert rc == 0, msg
    assert h.pose_prior_info()[:3] == (1, 3, 1) and abs(h.pose_prior_info()[3] - 1.5 - 0.5 * 5e-13) < 1e-12
    # with priors set, an exchange cannot be attached
    with pytest.raises(ptzba.PtzbaError, match="pose priors"):
        h.set_exchange_hook(lambda kind, ptr, count, stream: None)
    rc = ptzba.lib().ptzba_attach_comm(h.h, ctypes.c_void_p(1))  # (refused before the pointer is looked at)
    assert rc != 0 and "pose priors" in ptzba.lib().ptzba_last_error().decode()
    # a handle with a hook, and a sharded handle, take no priors
    h.clear_pose_priors()
    h.set_exchange_hook(lambda kind, ptr, count, stream: None)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        h.set_pose_priors(near)
    h.set_exchange_hook(None)
    h.set_pose_priors(near)
    assert h.pose_prior_info() == before
    h.close()
    p1 = prior_ref.problem("config1")
    g = ptzba.BAHandle(0)
    w1 = ptzba.frame_coupling_window(p1.n_pose, p1.frame, p1.landmark)
    g.set_problem(p1.n_pose, p1.n_landmark, p1.frame, p1.landmark, p1.xy, p1.u, p1.v, frame_win_hi=w1, dist_world=2,
                  dist_rank=0)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        g.set_pose_priors(_case("config1")[1])
    g.close()
    # (1, 45) with the raised window is accepted
    k = _handle("config2")
    assert k.pose_prior_info()[0] == len(factors)
    k.close()


# ------------------------------------------------------------------------------------------------ 8
def test_dropin_prior_on_the_unmatched_image(gpu_available):
    """ba_4x60 has an image without any match.  bundle_adjustment(pose_priors=...) with a unary prior on it returns
    that keyframe at the prior mean (1e-9); the observed keyframes agree with the call without priors (1e-6 deg /
    1e-4 px), whose outputs the keyword leaves alone."""
    import random
    import image_process
    import bundle_adjustment as ba
    from test_gpu_ba import _install_fixture_frontend, _problem_from_golden
    d = golden("ba_4x60.npz")
    n, _, frame, _, _, u, v = _problem_from_golden(d)
    lonely = [f for f in range(n) if f not in set(frame.tolist())]
    assert len(lonely) == 1 and lonely[0] >= 1
    f = lonely[0]
    mu = d["init_ptz"][f] + np.array([0.2, -0.1, 15.0])
    info = np.diag(1.0 / prior_ref.SIGMA ** 2)
    outs = []
    for kw in ({}, dict(pose_priors=[([100 + f], mu, info)])):
        saved, _ = _install_fixture_frontend(d)
        try:
            random.seed(int(d["seed"]))
            outs.append(ba.bundle_adjustment(list(range(n)), list(range(100, 100 + n)), "sift", d["init_ptz"].copy(),
                                             np.array([0.0, -10.0, 5.0]), np.eye(3), u, v, "", ftol=1e-14, xtol=1e-14,
                                             max_iter=200, **kw))
        finally:
            image_process.detect_compute_sift, image_process.match_sift_features = saved
    (lm0, kf0), (lm1, kf1) = outs
    ptz0 = np.array([[k.pan, k.tilt, k.f] for k in kf0])
    ptz1 = np.array([[k.pan, k.tilt, k.f] for k in kf1])
    print("unmatched image", f, "with prior", ptz1[f], "mean", mu, "without", ptz0[f])
    assert np.abs(ptz1[f] - mu).max() <= 1e-9
    seen = [i for i in range(n) if i != f]
    np.testing.assert_allclose(ptz1[seen, :2], ptz0[seen, :2], rtol=0, atol=1e-6)
    np.testing.assert_allclose(ptz1[seen, 2], ptz0[seen, 2], rtol=0, atol=1e-4)
    np.testing.assert_allclose(lm1, lm0, rtol=0, atol=1e-6)
