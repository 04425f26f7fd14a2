"""CPU tests of the Gaussian pose priors: the reference itself (tests/prior_ref.py against scipy), the factorisation
plan for a coupling window raised by prior_window, and the Python-side validation.  No GPU."""
import numpy as np
import pytest

import chol_plan_exec as cpe
import prior_ref
import ptzba

CONFIG2_PAIRS, CONFIG2_FAR = prior_ref.CONFIG2_PAIRS, prior_ref.CONFIG2_FAR


def test_reference_optimum_equals_scipy_on_whitened_rows():
    """prior_ref's Gauss-Newton optimum at config 1 (linear loss) == scipy least_squares on the oracle residual
    stacked with the whitened prior rows L^T e (info = L L^T), whose 1/2 |.|^2 is the prior cost.  1e-8 relative to
    each parameter's magnitude (>= 1)."""
    from scipy.optimize import least_squares
    from oracle import ptz_oracle as orc
    p = prior_ref.problem("config1")
    factors = prior_ref.factor_set(p)
    ptz, rays, c = prior_ref.solve(p, p.init_ptz, p.init_rays, factors)
    fr, lm = p.frame.astype(np.int64), p.landmark.astype(np.int64)
    chol = [np.linalg.cholesky(info) for _, _, info in factors]
    idx = [(3 * np.asarray(f, np.int64)[:, None] + np.arange(3)[None, :]).reshape(-1) - 3 for f, _, _ in factors]

    def fun(x):
        r = orc.compute_residual_records(np.concatenate([p.init_ptz[0], x]), p.n_pose, p.u, p.v, fr, lm, p.xy)
        rows = [L.T @ (x[i] - m) for L, i, (_, m, _) in zip(chol, idx, factors)]
        return np.concatenate([r.reshape(-1)] + rows)

    def jac(x):
        J = orc.ba_jacobian(x, p.n_pose, p.n_landmark, p.u, p.v, p.init_ptz[0], fr, lm).toarray()
        rows = []
        for L, i in zip(chol, idx):
            A = np.zeros((len(i), len(x)))
            A[:, i] = L.T
            rows.append(A)
        return np.concatenate([J] + rows)

    x0 = np.concatenate([p.init_ptz[1:].reshape(-1), p.init_rays.reshape(-1)])
    ref = least_squares(fun, x0, jac=jac, method="trf", tr_solver="exact", x_scale="jac", ftol=1e-15, xtol=1e-15,
                        gtol=1e-15)
    x = np.concatenate([ptz[1:].reshape(-1), rays.reshape(-1)])
    err = np.max(np.abs(x - ref.x) / np.maximum(1.0, np.abs(ref.x)))
    print(f"prior_ref vs scipy: {err:.3e}; cost {c:.12e} vs {ref.cost:.12e}; prior share "
          f"{prior_ref.prior_cost(factors, ptz):.6e}")
    assert err <= 1e-8, err
    assert abs(c - ref.cost) <= 1e-10 * ref.cost
    # the priors matter at this optimum: without them it lies elsewhere
    ptz0, _, _ = prior_ref.solve(p, p.init_ptz, p.init_rays, [])
    assert np.abs(ptz0 - ptz).max() > 1e-3


@pytest.mark.parametrize("cfg,ordering", [("config1", 0), ("config2", 0), ("config2", 2)])
def test_plan_for_prior_window_covers_the_factor_pairs(cfg, ordering):
    """The plan exported for prior_window's window factors a matrix whose coupling is exactly the records' window
    plus the factor pairs: replayed on the CPU (as test_plan_replay.py does) it gives numpy's Cholesky factor.  At
    config 2 the pair (1, 45) lies outside the records' window, so the window has to be raised for it
    (the library refuses the factor otherwise: test_gpu_priors.py)."""
    p = prior_ref.problem(cfg)
    c2 = cfg == "config2"
    factors = prior_ref.factor_set(p, CONFIG2_PAIRS if c2 else (), CONFIG2_FAR if c2 else None)
    win0 = ptzba.frame_coupling_window(p.n_pose, p.frame, p.landmark)
    win = ptzba.prior_window(p.n_pose, p.frame, p.landmark, factors)
    assert np.all(win >= win0)
    if c2:
        assert win0[0] == 26 and win0[1] == 32 and win0[19] == 49 and win0[45] == 49  # banded: (1, 45) is outside
        assert win[1] == 45 and win0[1] < 45
    else:
        assert np.all(win0 == p.n_pose - 1) and np.array_equal(win, win0)  # fully coupled
    pos, tasks, off, n_aug, _ = ptzba.plan_export(win, 1, ordering)
    ld = (n_aug + 1 + 31) // 32 * 32
    pairs = {(f1, f2) for f1 in range(1, p.n_pose) for f2 in range(f1, int(win0[f1]) + 1)}
    for frames, _, _ in factors:
        pairs |= {(min(a, b), max(a, b)) for a in frames.tolist() for b in frames.tolist()}
    rng = np.random.default_rng(0)
    S = np.zeros((ld, ld))
    for f1, f2 in sorted(pairs):
        blk = rng.standard_normal((3, 3))
        p1, p2 = pos[f1], pos[f2]
        if f1 == f2:
            blk = 0.5 * (blk + blk.T)
        S[p2:p2 + 3, p1:p1 + 3] += blk
        if f1 != f2:
            S[p1:p1 + 3, p2:p2 + 3] += blk.T
    rows = np.zeros(ld, bool)
    for f in range(1, p.n_pose):
        rows[pos[f]:pos[f] + 3] = True
    S[np.arange(ld), np.arange(ld)] = np.where(rows, np.abs(S).sum(1) + 1.0, 1.0)
    b = rng.standard_normal(n_aug) * rows[:n_aug]
    S[n_aug, :n_aug] = b
    S[:n_aug, n_aug] = b
    S[n_aug, n_aug] = np.abs(b).sum() * 1e3 + 1.0
    Lf, _ = cpe.replay(S, tasks, off)
    Lref = np.linalg.cholesky(S)
    assert np.abs(Lf - Lref).max() <= 1e-12 * np.abs(Lref).max()
    if c2:
        assert np.abs(S[pos[45]:pos[45] + 3, pos[1]:pos[1] + 3]).min() > 0  # the far pair's block is there


def test_recorded_config2_huber_point_is_stationary():
    """tests/golden/priors_config2_huber.npz (the reference of test_gpu_priors' config-2 Huber solve) is a stationary
    point of the Huber objective with the config-2 factor set as prior_ref builds it today."""
    import os
    from conftest import GOLDEN, golden
    golden(prior_ref.CONFIG2_HUBER)
    ptz, rays, c = prior_ref.config2_huber_point(os.path.join(GOLDEN, prior_ref.CONFIG2_HUBER))
    assert ptz.shape == (50, 3) and rays.shape == (1609, 2) and c > 0


def test_python_validation_errors():
    eye = np.eye(3)
    ok = ([2], [0.0, 0.0, 3000.0], eye)
    assert len(ptzba.check_pose_priors([ok], 5)) == 1
    bad = {
        "mean size": ([2], [0.0, 0.0], eye),
        "info shape": ([2], [0.0, 0.0, 1.0], np.eye(4)),
        "info shape for two frames": ([2, 3], np.zeros(6), eye),
        "repeated frame": ([2, 2], np.zeros(6), np.eye(6)),
        "no frame": ([], [], np.zeros((0, 0))),
        "nine frames": (list(range(1, 10)), np.zeros(27), np.eye(27)),
        "frame out of range": ([5], np.zeros(3), eye),
        "negative frame": ([-1], np.zeros(3), eye),
        "non-integer frames": ([1.5], np.zeros(3), eye),
        "non-finite mean": ([2], [0.0, np.nan, 1.0], eye),
        "non-finite info": ([2], np.zeros(3), np.diag([1.0, np.inf, 1.0])),
        "asymmetric": ([2], np.zeros(3), eye + np.array([[0, 1e-3, 0], [0, 0, 0], [0, 0, 0]])),
        "indefinite": ([2], np.zeros(3), np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]])),
        "negative definite": ([2], np.zeros(3), -eye),
    }
    for what, fac in bad.items():
        with pytest.raises(ValueError):
            ptzba.check_pose_priors([ok, fac], 5)
            pytest.fail(what)
    with pytest.raises(ValueError):
        ptzba.check_pose_priors([5], 5)  # not a (frames, mean, info) triple
    # semi-definite is allowed (a prior on pan only), and asymmetry within 1e-12 max|info|
    ptzba.check_pose_priors([([2], np.zeros(3), np.diag([4.0, 0.0, 0.0]))], 5)
    ptzba.check_pose_priors([([2], np.zeros(3), eye + np.array([[0, 1e-13, 0], [0, 0, 0], [0, 0, 0]]))], 5)
    # prior_window: every pair of a factor is covered, the records' window kept elsewhere
    fr = np.array([0, 1, 1, 2, 2, 3, 3, 4], np.int32)
    lm = np.array([0, 0, 1, 1, 2, 2, 3, 3], np.int32)
    w = ptzba.prior_window(5, fr, lm, [([4, 1, 2], np.zeros(9), np.eye(9))])
    assert w.tolist() == [1, 4, 4, 4, 4]


def test_bundle_adjustment_refuses_a_prior_on_the_gauge_image():
    """The drop-in's pose_priors are keyed by image index; the first image is the gauge.  Raised before any image
    is touched."""
    import bundle_adjustment as ba
    ptzs = np.array([[0.0, 0.0, 3000.0], [1.0, 0.0, 3000.0]])
    args = ([None, None], [7, 9], "sift", ptzs, np.zeros(3), np.eye(3), 640.0, 360.0, "")
    with pytest.raises(ValueError, match="gauge"):
        ba.bundle_adjustment(*args, pose_priors=[([7], ptzs[0], np.eye(3))])
    with pytest.raises(ValueError, match="image index"):
        ba.bundle_adjustment(*args, pose_priors=[([8], ptzs[1], np.eye(3))])
    with pytest.raises(ValueError):
        ba.bundle_adjustment(*args, pose_priors=[([9], ptzs[1], -np.eye(3))])


def test_map_and_slam_pass_the_keyframe_prior(monkeypatch):
    """Map.add_keyframe_with_ba(pose_prior=cov) hands bundle_adjustment one unary factor on the new keyframe's image
    index, mean its current pose, info = cov^-1; without the keyword the call is as before.  PtzSlam.keyframe_prior
    passes state_cov[:3, :3]."""
    import scene_map
    from key_frame import KeyFrame
    from ptz_slam import PtzSlam
    calls = []

    def fake_ba(images, image_indices, *args, **kw):
        calls.append((list(image_indices), kw))
        return np.zeros((0, 2)), []

    monkeypatch.setattr(scene_map, "bundle_adjustment", fake_ba)
    kf = [KeyFrame(None, 10 + i, np.zeros(3), np.eye(3), 640.0, 360.0, 1.0 * i, -2.0, 3000.0 + i) for i in range(3)]
    m = scene_map.Map("sift", cache_correspondences=False)
    m.add_first_keyframe(kf[0])
    m.keyframe_list.append(kf[1])
    m.add_keyframe_with_ba(kf[2], "")
    assert "pose_priors" not in calls[-1][1]
    cov = np.array([[4e-4, 1e-5, 0.0], [1e-5, 9e-4, 0.0], [0.0, 0.0, 25.0]])
    m.keyframe_list = [kf[0], kf[1]]
    m.add_keyframe_with_ba(kf[2], "", pose_prior=cov)
    idx, kw = calls[-1]
    (frames, mean, info), = kw["pose_priors"]
    assert idx == [10, 11, 12] and list(frames) == [12]
    np.testing.assert_array_equal(mean, [2.0, -2.0, 3002.0])
    np.testing.assert_allclose(info @ cov, np.eye(3), atol=1e-12)
    assert np.array_equal(info, info.T)
    for bad in (np.eye(2), -np.eye(3), np.diag([1.0, 0.0, 1.0]), np.full((3, 3), np.nan)):
        m.keyframe_list = [kf[0], kf[1]]
        with pytest.raises(ValueError):
            m.add_keyframe_with_ba(kf[2], "", pose_prior=bad)

    class Cam:
        camera_center, base_rotation, principal_point = np.zeros(3), np.eye(3), (640.0, 360.0)
        pan, tilt, focal_length = 2.0, -2.0, 3002.0

    slam = PtzSlam()
    assert slam.keyframe_prior is False
    slam.keyframe_map = m
    m.keyframe_list = [kf[0], kf[1]]
    slam.state_cov = np.block([[cov, np.zeros((3, 2))], [np.zeros((2, 3)), np.eye(2)]])
    slam.add_keyframe(None, Cam(), 12)
    assert "pose_priors" not in calls[-1][1]
    slam.keyframe_prior = True
    m.keyframe_list = [kf[0], kf[1]]
    slam.add_keyframe(None, Cam(), 12)
    np.testing.assert_allclose(calls[-1][1]["pose_priors"][0][2] @ cov, np.eye(3), atol=1e-12)
