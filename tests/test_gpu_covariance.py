"""GPU tests of the BA posterior covariance (ptzba_covariance: BAHandle.covariance, LMSolver.covariance and the
drop-in's `covariance=` keyword).

Reference (tests/cov_ref.py): the oracle's analytic Jacobian at the state, rows scaled by sqrt(rho') for Huber,
np.linalg.inv(J^T J) whole; the pose and ray blocks are cut out of it.  Metric: correlation-scaled block error,
max |S_gpu - S_ref| / sqrt(S_ref,ii S_ref,jj).  Tolerances: the project's own for the same linearise -> Schur ->
Cholesky chain (test_gpu_ba.test_single_gauss_newton_step_is_exact): 1e-7 fp64, 2e-3 fp32.  The reference's two routes
agree to 1e-13 (config 1) and 2e-12 (config 2) in this metric (test_covariance_cpu.py)."""
import ctypes

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

TOL = {0: 1e-7, 1: 2e-3}


def _handle(p, precision=0, ordering=0, loss=0, f_scale=1.0, n_fixed=1, state=None):
    import ptzba
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=precision, ordering=ordering,
                  loss=loss, f_scale=f_scale, n_fixed=n_fixed)
    ptz, rays = state if state is not None else (p.init_ptz, p.init_rays)
    h.set_state(ptz, rays)
    return h


def _frames_per_landmark(p):
    seen = np.zeros((p.n_landmark, p.n_pose), bool)
    seen[p.landmark, p.frame] = True
    return seen.sum(1)


def _config2_landmarks(p):
    """50 landmarks: index 0, index M - 1, the one seen by the most frames, one seen by the fewest, 46 drawn."""
    cnt = _frames_per_landmark(p)
    pick = [0, p.n_landmark - 1, int(np.argmax(cnt)), int(np.argmin(cnt))]
    rest = np.random.default_rng(0).choice(p.n_landmark, 46, replace=False)
    idx = np.concatenate([pick, rest]).astype(np.int32)
    assert len(idx) == 50 and cnt[idx].max() == cnt.max() and cnt[idx].min() == cnt.min()
    return idx


@pytest.mark.parametrize("cfg,ordering", [("config1", 0), ("config2", 0), ("config2", 2)])
@pytest.mark.parametrize("precision", [0, 1])
def test_blocks_match_dense_inverse(gpu_available, precision, cfg, ordering):
    """Pose and ray blocks == the blocks of the dense inverse.  config 1: one tile with the augmented row inside it,
    every landmark (130 -> nine right-hand-side blocks, the last ragged).  config 2: five tiles; ordering 2 forces the
    nested order (padding rows, reversed part); every pose plus 50 landmarks."""
    import cov_ref
    p, pose_ref, ray_ref = cov_ref.synthetic_reference(cfg)
    h = _handle(p, precision, ordering)
    if ordering == 2:
        assert h.solver_info()["ordering"] == "nested"
    if cfg == "config1":
        si = h.solver_info()
        assert si["n_aug"] == 27 and si["ld"] == 32  # the augmented row shares the data rows' tile
        pose, ray, info = h.covariance("all")
        idx = np.arange(p.n_landmark)
        assert len(idx) == 130
    else:
        idx = _config2_landmarks(p)
        pose, ray, info = h.covariance(idx)
    h.close()
    ep, er = cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref[idx])
    print(f"{cfg} ordering {ordering} precision {precision}: pose {ep:.3e} ray {er:.3e} (tol {TOL[precision]:.0e}); "
          f"{info}")
    assert info["scale"] == 1.0 and info["min_pivot"] > 0 and info["n_free"] == 3 * (p.n_pose - 1) + 2 * p.n_landmark
    assert ep <= TOL[precision] and er <= TOL[precision], (ep, er)


def test_two_fixed_frames(gpu_available):
    """n_fixed = 2 at config 1: frames 0 and 1 come back all zero, the rest match the dense inverse with both
    reference poses removed."""
    import cov_ref
    p, pose_ref, ray_ref = cov_ref.synthetic_reference("config1", n_fixed=2)
    h = _handle(p, n_fixed=2)
    pose, ray, info = h.covariance("all")
    h.close()
    assert not pose[:2].any() and pose[2:].all()
    ep, er = cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref)
    print(f"n_fixed 2: pose {ep:.3e} ray {er:.3e}")
    assert info["n_free"] == 3 * (p.n_pose - 2) + 2 * p.n_landmark
    assert ep <= 1e-7 and er <= 1e-7, (ep, er)


def test_huber_weights_and_curvature_setting(gpu_available):
    """Huber (config 2, fp64): the blocks match the sqrt(rho')-weighted reference to 1e-7 -- IRLS weights whatever
    curvature was set -- and set_huber_curvature's effect on a later linearize() is what it is without the call."""
    import ptzba
    import cov_ref
    from oracle import ptz_oracle as orc
    fs = 1.0
    p, pose_ref, ray_ref = cov_ref.synthetic_reference("config2", "huber", fs)
    r = orc.compute_residual_records(np.concatenate([p.init_ptz.reshape(-1), p.init_rays.reshape(-1)]), p.n_pose, p.u,
                                     p.v, p.frame.astype(np.int64), p.landmark.astype(np.int64), p.xy)
    beyond = np.abs(r) > fs
    print(f"huber f_scale {fs}: {beyond.sum()} of {len(r)} residuals beyond the unit")
    assert beyond.any() and not beyond.all()
    idx = _config2_landmarks(p)
    h = _handle(p, loss=ptzba.LOSS_HUBER, f_scale=fs)
    pose, ray, _ = h.covariance(idx)
    e0 = max(cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref[idx]))
    h.set_huber_curvature(0.1)
    pose1, ray1, _ = h.covariance(idx)
    e1 = max(cov_ref.block_err(pose1, pose_ref), cov_ref.block_err(ray1, ray_ref[idx]))
    print(f"huber: {e0:.3e}; after set_huber_curvature(0.1): {e1:.3e}")
    assert e0 <= 1e-7 and e1 <= 1e-7, (e0, e1)
    assert pose1.tobytes() == pose.tobytes() and ray1.tobytes() == ray.tobytes()
    # the 0.1 setting still governs the next linearisation: the same damped step as on a handle that never asked
    h.linearize()
    h.step(1e-3)
    s = h.read_scalars()
    h.close()
    g = _handle(p, loss=ptzba.LOSS_HUBER, f_scale=fs)
    g.set_huber_curvature(0.1)
    g.linearize()
    g.step(1e-3)
    t = g.read_scalars()
    g.close()
    assert s.tobytes() == t.tobytes(), (s, t)
    k = _handle(p, loss=ptzba.LOSS_HUBER, f_scale=fs)  # (and 0.1 is not what IRLS gives: the comparison can fail)
    k.linearize()
    k.step(1e-3)
    assert k.read_scalars()[1] != t[1]
    k.close()


def test_residual_scale_at_optimum(gpu_available):
    """LMSolver solves config 1 in fp64; covariance(scale="residual") == s^2 H^-1 of the oracle at the returned state,
    s^2 = sum r^2 / (2 R - n_free)."""
    import ptzba
    import synthetic
    import cov_ref
    from oracle import ptz_oracle as orc
    p = synthetic.make_problem("config1", seed=0)
    h = _handle(p)
    solver = ptzba.LMSolver(h, ftol=1e-10, xtol=1e-12)
    res = solver.run()
    pose, ray, info = solver.covariance("all", scale="residual")
    ptz, rays = h.get_state()
    h.close()
    assert res.status > 0, res
    r = orc.compute_residual_records(np.concatenate([ptz.reshape(-1), rays.reshape(-1)]), p.n_pose, p.u, p.v,
                                     p.frame.astype(np.int64), p.landmark.astype(np.int64), p.xy)
    n_free = 3 * (p.n_pose - 1) + 2 * p.n_landmark
    s2 = float(np.sum(r * r)) / (len(r) - n_free)
    assert len(r) == 2 * len(p.frame)
    pose_ref, ray_ref = cov_ref.dense_blocks(p, ptz, rays)
    ep, er = cov_ref.block_err(pose, s2 * pose_ref), cov_ref.block_err(ray, s2 * ray_ref)
    print(f"optimum: s2 {s2:.6e} (gpu {info['scale']:.6e}); pose {ep:.3e} ray {er:.3e}")
    assert abs(info["scale"] - s2) <= 1e-9 * s2
    assert info["n_free"] == n_free
    assert ep <= 1e-7 and er <= 1e-7, (ep, er)


def test_structure_and_determinism(gpu_available):
    """Every block symmetric bit for bit with positive eigenvalues; two calls return identical bytes; poses without
    rays and rays without poses work; duplicate indices return duplicate blocks; a given scale multiplies."""
    import cov_ref
    p, pose_ref, ray_ref = cov_ref.synthetic_reference("config2")
    h = _handle(p, precision=1, ordering=2)
    pose, ray, _ = h.covariance("all")
    pose2, ray2, _ = h.covariance("all")
    assert pose.tobytes() == pose2.tobytes() and ray.tobytes() == ray2.tobytes()
    assert np.array_equal(pose, pose.transpose(0, 2, 1)) and np.array_equal(ray, ray.transpose(0, 2, 1))
    assert not pose[0].any()
    assert np.all(np.linalg.eigvalsh(pose[1:]) > 0) and np.all(np.linalg.eigvalsh(ray) > 0)
    only_pose, none_ray, _ = h.covariance(None)
    assert none_ray is None and only_pose.tobytes() == pose.tobytes()
    idx = np.array([7, 3, 7, p.n_landmark - 1, 3], np.int32)
    no_pose, some, _ = h.covariance(idx, poses=False)
    assert no_pose is None and some.shape == (5, 2, 2)
    assert some.tobytes() == ray[idx].tobytes()
    scaled_pose, scaled_ray, info = h.covariance(idx, scale=2.0)
    assert info["scale"] == 2.0
    assert np.array_equal(scaled_pose, 2.0 * pose) and np.array_equal(scaled_ray, 2.0 * ray[idx])
    empty = h.covariance(np.zeros(0, np.int32))[1]
    assert empty.shape == (0, 2, 2)
    h.close()


def test_no_side_effect_on_a_following_solve(gpu_available):
    """config 2, fp32 + Huber: a device-loop solve from x0, and one with covariance("all") between set_state and the
    solve, give the same state, njev and status bit for bit."""
    import ptzba
    import synthetic
    p = synthetic.make_problem("config2", seed=0)
    out = []
    for with_cov in (False, True):
        h = _handle(p, precision=1, loss=ptzba.LOSS_HUBER)
        if with_cov:
            h.covariance("all")
        res = ptzba.LMSolver(h, ftol=1e-4, xtol=1e-8).run()
        ptz, rays = h.get_state()
        h.close()
        out.append((ptz.tobytes(), rays.tobytes(), res.njev, res.status, res.cost))
    assert out[0][2] > 1
    assert out[0] == out[1], (out[0][2:], out[1][2:])


def test_errors_leave_the_handle_usable(gpu_available):
    """Out-of-range landmark index, unknown struct_size and an unobserved free frame each raise with a message naming
    the condition; the handle then still computes a covariance on a good problem."""
    import ptzba
    import synthetic
    import cov_ref
    p, pose_ref, _ = cov_ref.synthetic_reference("config1")
    h = _handle(p)
    with pytest.raises(ptzba.PtzbaError, match="out of range"):
        h.covariance(np.array([0, p.n_landmark], np.int32))
    with pytest.raises(ptzba.PtzbaError, match="out of range"):
        h.covariance(np.array([-1], np.int32))
    with pytest.raises(ptzba.PtzbaError, match="struct_size"):
        h.covariance(None, _struct_size=ctypes.sizeof(ptzba.ptzba_cov_opts) + 8)
    with pytest.raises(ptzba.PtzbaError, match="bad options"):
        h.covariance(None, scale=-1.0)
    assert cov_ref.block_err(h.covariance(None)[0], pose_ref) <= 1e-7
    # one free frame without records: S is singular, the factorisation reports it, no numbers come back
    keep = p.frame != 5
    h.set_problem(p.n_pose, p.n_landmark, p.frame[keep], p.landmark[keep], p.xy[keep], p.u, p.v)
    h.set_state(p.init_ptz, p.init_rays)
    with pytest.raises(ptzba.PtzbaError, match="not positive definite"):
        h.covariance("all")
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v)
    h.set_state(p.init_ptz, p.init_rays)
    assert cov_ref.block_err(h.covariance(None)[0], pose_ref) <= 1e-7
    h.close()
    e = ptzba.BAHandle(0)
    with pytest.raises(ptzba.PtzbaError, match="no problem set"):
        e.covariance(None)
    e.close()


def test_dropin_keyword(gpu_available):
    """bundle_adjustment() on the ba_6x120 golden: with the keyword off it returns what it returns today (the
    assertions of test_gpu_ba.test_dropin_bundle_adjustment_matches_reference); with it on, the same keyframes and
    landmarks plus covariances equal to BAHandle.covariance at that solution (1e-7 in the block metric: the drop-in's
    handle holds the same records in the match graph's order, so the sums differ in rounding only)."""
    import random
    import image_process
    import bundle_adjustment as ba
    import ptzba
    import cov_ref
    from test_gpu_ba import _install_fixture_frontend, _problem_from_golden
    d = golden("ba_6x120.npz")
    n = int(d["n_pose"])
    runs = []
    for on in (False, True):
        saved, kp_store = _install_fixture_frontend(d)
        try:
            random.seed(int(d["seed"]))
            kw = dict(covariance=True) if on else {}
            out = ba.bundle_adjustment(list(range(n)), list(range(100, 100 + n)), "sift", d["init_ptz"].copy(),
                                       np.array([0.0, -10.0, 5.0]), np.eye(3), float(d["u"]), float(d["v"]), "",
                                       ftol=1e-14, xtol=1e-14, max_iter=200, **kw)
        finally:
            image_process.detect_compute_sift, image_process.match_sift_features = saved
        assert len(out) == (3 if on else 2)
        landmarks, keyframes = out[:2]
        assert landmarks.shape == (int(d["n_landmark"]), 2)
        off = d["kf_off"]
        for i, kf in enumerate(keyframes):
            np.testing.assert_array_equal(kf.landmark_index.astype(np.int64), d["kf_lmk"][off[i]:off[i + 1]])
            pos = {id(o): k for k, o in enumerate(kp_store[i])}
            np.testing.assert_array_equal([pos[id(o)] for o in kf.feature_pts], d["kf_local"][off[i]:off[i + 1]])
            assert kf.img_index == 100 + i
        assert int(ba.LAST_RESULT["n_residual"]) == int(d["n_residual"])
        np.testing.assert_allclose(ba.LAST_RESULT["x0"], d["x0"], rtol=0, atol=1e-9)
        xt = d["x_tight"]
        ptz = np.array([[k.pan, k.tilt, k.f] for k in keyframes])
        ptz_t = np.concatenate([d["ref_pose"], xt[:3 * (n - 1)]]).reshape(-1, 3)
        np.testing.assert_allclose(ptz[:, :2], ptz_t[:, :2], rtol=0, atol=1e-6)
        np.testing.assert_allclose(ptz[:, 2], ptz_t[:, 2], rtol=0, atol=1e-4)
        np.testing.assert_allclose(landmarks.reshape(-1), xt[3 * (n - 1):], rtol=0, atol=1e-6)
        runs.append((ptz, landmarks, out[2] if on else None))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    ptz, landmarks, cov = runs[1]
    assert cov["pose_cov"].shape == (n, 3, 3) and cov["ray_cov"].shape == (len(landmarks), 2, 2)
    n_pose, n_lm, frame, landmark, xy, u, v = _problem_from_golden(d)
    h = ptzba.BAHandle(0)
    h.set_problem(n_pose, n_lm, frame, landmark, xy, u, v)
    h.set_state(ptz, landmarks)
    pose_ref, ray_ref, _ = h.covariance("all")
    h.close()
    assert not cov["pose_cov"][0].any() and cov["pose_cov"][1:].any()
    ep, er = cov_ref.block_err(cov["pose_cov"], pose_ref), cov_ref.block_err(cov["ray_cov"], ray_ref)
    print(f"drop-in vs BAHandle.covariance: pose {ep:.3e} ray {er:.3e}")
    assert ep <= 1e-7 and er <= 1e-7, (ep, er)
