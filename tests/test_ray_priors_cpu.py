"""CPU tests of the Gaussian ray priors: the reference itself (tests/ray_prior_ref.py against scipy), the Python-side
validation and helpers, and the drop-in's keying of a prior by (image index, keypoint index).  No GPU."""
import os

import numpy as np
import pytest

import ptzba
import ray_prior_ref


def test_reference_optimum_equals_scipy_on_whitened_rows():
    """ray_prior_ref's Gauss-Newton optimum at config 1 (linear loss) with the standard set S == scipy least_squares on
    the oracle residual stacked with the whitened prior rows L^T e (info = L L^T).  1e-8 relative to each parameter's
    magnitude (>= 1): test_priors_cpu's tolerance for the same check."""
    from scipy.optimize import least_squares
    from oracle import ptz_oracle as orc
    p = ray_prior_ref.problem("config1")
    S = list(ray_prior_ref.standard("config1"))
    ptz, rays, c = ray_prior_ref.solve(p, p.init_ptz, p.init_rays, S)
    fr, lm = p.frame.astype(np.int64), p.landmark.astype(np.int64)
    k = 3 * (p.n_pose - 1)
    chol = [np.linalg.cholesky(info) for _, _, info in S]
    idx = [k + 2 * l + np.arange(2) for l, _, _ in S]

    def fun(x):
        r = orc.compute_residual_records(np.concatenate([p.init_ptz[0], x]), p.n_pose, p.u, p.v, fr, lm, p.xy)
        rows = [L.T @ (x[i] - m) for L, i, (_, m, _) in zip(chol, idx, S)]
        return np.concatenate([r.reshape(-1)] + rows)

    def jac(x):
        J = orc.ba_jacobian(x, p.n_pose, p.n_landmark, p.u, p.v, p.init_ptz[0], fr, lm).toarray()
        A = np.zeros((2 * len(S), len(x)))
        for n, (L, i) in enumerate(zip(chol, idx)):
            A[2 * n:2 * n + 2, i] = L.T
        return np.concatenate([J, A])

    x0 = np.concatenate([p.init_ptz[1:].reshape(-1), p.init_rays.reshape(-1)])
    ref = least_squares(fun, x0, jac=jac, method="trf", tr_solver="exact", x_scale="jac", ftol=1e-15, xtol=1e-15,
                        gtol=1e-15)
    x = np.concatenate([ptz[1:].reshape(-1), rays.reshape(-1)])
    err = np.max(np.abs(x - ref.x) / np.maximum(1.0, np.abs(ref.x)))
    print(f"ray_prior_ref vs scipy: {err:.3e}; cost {c:.12e} vs {ref.cost:.12e}; prior share "
          f"{ray_prior_ref.ray_prior_cost(S, rays):.6e}")
    assert err <= 1e-8, err
    assert abs(c - ref.cost) <= 1e-10 * ref.cost
    # the priors matter at this optimum: without them it lies elsewhere
    _, rays0, _ = ray_prior_ref.solve(p, p.init_ptz, p.init_rays, [])
    assert np.abs(rays0 - rays).max() > 1e-3


def test_standard_set_shape():
    """S names every third observed landmark once and the first five of them twice, the duplicates not adjacent."""
    for cfg in ("config1", "config2"):
        p = ray_prior_ref.problem(cfg)
        S = ray_prior_ref.standard(cfg)
        lms = ray_prior_ref.observed(p)[::3]
        assert [s[0] for s in S] == lms.tolist() + lms[:5].tolist()
        assert not np.array_equal(S[0][1], S[len(lms)][1])
        lm, mean, info = ptzba.check_ray_priors(S, p.n_landmark)
        assert lm.dtype == np.int32 and mean.shape == (len(S), 2) and info.shape == (len(S), 3)
        ev = [np.linalg.eigvalsh(s[2]) for s in S]
        np.testing.assert_allclose(np.array(ev), np.tile([1 / 0.06 ** 2, 1 / 0.02 ** 2], (len(S), 1)), rtol=1e-9)


def test_recorded_config2_huber_point_is_stationary():
    """tests/golden/ray_priors_config2_huber.npz (the reference of test_gpu_ray_priors' config-2 Huber solve) is a
    stationary point of the Huber objective with S as ray_prior_ref builds it today."""
    from conftest import GOLDEN, golden
    golden(ray_prior_ref.CONFIG2_HUBER)
    ptz, rays, c = ray_prior_ref.config2_huber_point(os.path.join(GOLDEN, ray_prior_ref.CONFIG2_HUBER))
    assert ptz.shape == (50, 3) and rays.shape == (1609, 2) and c > 0


def test_python_validation_errors():
    eye = np.eye(2)
    ok = (2, [10.0, -5.0], eye)
    lm, mean, info = ptzba.check_ray_priors([ok, ok], 5)
    assert lm.tolist() == [2, 2] and mean.tolist() == [[10.0, -5.0]] * 2 and info.tolist() == [[1.0, 0.0, 1.0]] * 2
    bad = {
        "mean size": (2, [0.0, 0.0, 1.0], eye),
        "info shape": (2, [0.0, 0.0], np.eye(3)),
        "flat info": (2, [0.0, 0.0], [1.0, 0.0, 1.0]),
        "landmark out of range": (5, [0.0, 0.0], eye),
        "negative landmark": (-1, [0.0, 0.0], eye),
        "non-integer landmark": (1.5, [0.0, 0.0], eye),
        "landmark list": ([1, 2], [0.0, 0.0], eye),
        "non-finite mean": (2, [0.0, np.nan], eye),
        "non-finite info": (2, [0.0, 0.0], np.diag([1.0, np.inf])),
        "asymmetric": (2, [0.0, 0.0], np.array([[1.0, 1e-3], [0.0, 1.0]])),
        "indefinite": (2, [0.0, 0.0], np.array([[1.0, 2.0], [2.0, 1.0]])),
        "negative definite": (2, [0.0, 0.0], -eye),
    }
    for what, pr in bad.items():
        with pytest.raises(ValueError):
            ptzba.check_ray_priors([ok, pr], 5)
            pytest.fail(what)
    with pytest.raises(ValueError):
        ptzba.check_ray_priors([5], 5)  # not a (landmark, mean, info) triple
    # semi-definite is allowed (a prior on theta only); asymmetry within 1e-12 max|info| is symmetrised
    ptzba.check_ray_priors([(2, [0.0, 0.0], np.diag([4.0, 0.0]))], 5)
    _, _, info = ptzba.check_ray_priors([(2, [0.0, 0.0], np.array([[1.0, 4e-13], [0.0, 1.0]]))], 5)
    assert info.tolist() == [[1.0, 2e-13, 1.0]]
    assert ptzba.check_ray_priors([])[0].shape == (0,)
    assert ptzba.check_ray_priors([(10 ** 6, [0.0, 0.0], eye)])[0].tolist() == [10 ** 6]  # no bound given


def test_ray_priors_from_covariance_round_trip():
    rng = np.random.default_rng(1)
    n = 6
    A = rng.standard_normal((n, 2, 2))
    cov = A @ A.transpose(0, 2, 1) * 1e-3 + 1e-4 * np.eye(2)
    cov[2] = 0.0  # a landmark without records: covariance() leaves a zero block
    cov[4] = np.diag([1e-3, 1e-9])
    rays = rng.uniform(-30, 30, (n, 2))
    lms = np.array([7, 3, 9, 11, 5, 2])
    out = ptzba.ray_priors_from_covariance(lms, rays, cov)
    assert [o[0] for o in out] == [7, 3, 11, 5, 2]  # the zero block is skipped
    for l, mean, info in out:
        i = lms.tolist().index(l)
        np.testing.assert_array_equal(mean, rays[i])
        np.testing.assert_allclose(np.linalg.inv(info), cov[i], rtol=1e-9, atol=0)
    ptzba.check_ray_priors(out, 12)
    out4 = ptzba.ray_priors_from_covariance(lms, rays, cov, inflate=4.0)
    for (_, _, a), (_, _, b) in zip(out, out4):
        np.testing.assert_allclose(4.0 * b, a, rtol=1e-12)
    out_e = ptzba.ray_priors_from_covariance(lms, rays, cov, min_eig=1e-8)
    assert [o[0] for o in out_e] == [7, 3, 11, 2]  # the block with an eigenvalue 1e-9 is skipped
    with pytest.raises(ValueError):
        ptzba.ray_priors_from_covariance(lms[:3], rays, cov)
    assert "twice" in ptzba.ray_priors_from_covariance.__doc__ and "twice" in ptzba.ray_priors_from_result.__doc__


def test_bundle_adjustment_key_errors_before_image_work():
    """The drop-in's ray priors are keyed by (image index, keypoint index); a bad key or value raises before any image
    is touched (the images here are None)."""
    import bundle_adjustment as ba
    ptzs = np.array([[0.0, 0.0, 3000.0], [1.0, 0.0, 3000.0]])
    args = ([None, None], [7, 9], "sift", ptzs, np.zeros(3), np.eye(3), 640.0, 360.0, "")
    eye = np.eye(2)
    with pytest.raises(ValueError, match="image index"):
        ba.bundle_adjustment(*args, ray_priors=[(8, 0, [0.0, 0.0], eye)])
    with pytest.raises(ValueError, match="keypoint index"):
        ba.bundle_adjustment(*args, ray_priors=[(7, -1, [0.0, 0.0], eye)])
    with pytest.raises(ValueError, match="keypoint index"):
        ba.bundle_adjustment(*args, ray_priors=[(7, 0.5, [0.0, 0.0], eye)])
    with pytest.raises(ValueError, match="expected"):
        ba.bundle_adjustment(*args, ray_priors=[(7, 0, [0.0, 0.0])])
    with pytest.raises(ValueError, match="positive semi-definite"):
        ba.bundle_adjustment(*args, ray_priors=[(9, 0, [0.0, 0.0], -eye)])
    with pytest.raises(ValueError, match="non-finite"):
        ba.bundle_adjustment(*args, ray_priors=[(9, 0, [0.0, np.nan], eye)])


def _toy_graph():
    """Three images, 6 / 7 / 5 keypoints, matches (0, 1) and (1, 2): landmarks seen by two or three images."""
    import correspondence
    rng = np.random.default_rng(0)
    counts = [6, 7, 5]
    xy = [rng.uniform(0, 1280, (n, 2)) for n in counts]
    des = [np.zeros((n, 4), np.float32) for n in counts]
    k1 = [0, 2, 5, 1, 3, 6]  # pair (0, 1): keypoints 0, 2, 5 of image 0; pair (1, 2): keypoints 1, 3, 6 of image 1
    k2 = [1, 4, 2, 0, 4, 3]  # ... matched with 1, 4, 2 of image 1 and 0, 4, 3 of image 2
    return correspondence.MatchGraph([a.copy() for a in xy], des, xy, [0, 1], [1, 2], [0, 3, 6], k1, k2)


def test_keypoint_index_and_ray_priors_from_result(monkeypatch):
    """KeyFrame.keypoint_index is parallel to landmark_index (empty for a keyframe built by hand);
    ray_priors_from_result gives one key per landmark, through the first keyframe holding it, and bundle_adjustment
    resolves each key back to that landmark; a keypoint without a match is skipped and reported."""
    import bundle_adjustment as ba
    import correspondence
    from key_frame import KeyFrame
    g = _toy_graph()
    M = g.n_landmark
    assert M == 5  # image 1's keypoint 1 is in both pairs: 6 matches, 5 landmarks
    calls = []

    def fake_solve(n_pose, n_landmark, frame, landmark, xy, u, v, init_ptz, init_rays, **kw):
        calls.append(kw)
        rays = np.stack([np.arange(n_landmark) * 1.0, np.arange(n_landmark) * -2.0], 1)
        cov = (np.zeros((n_pose, 3, 3)), np.arange(1, n_landmark + 1)[:, None, None] * 1e-4 * np.eye(2), {})
        return (np.array(init_ptz), rays, None) + ((cov,) if kw.get("covariance") else ())

    monkeypatch.setattr(correspondence, "build_graph", lambda *a, **k: _toy_graph())
    monkeypatch.setattr(ba.ptzba, "solve", fake_solve)
    monkeypatch.setattr(ba.ptzba, "image_to_ray", lambda u, v, f, pan, tilt, x, y, device=0: (x * 0.0, y * 0.0))
    ptzs = np.array([[0.0, 0.0, 3000.0], [1.0, 0.0, 3000.0], [2.0, 0.0, 3000.0]])
    args = ([None] * 3, [10, 11, 12], "sift", ptzs, np.zeros(3), np.eye(3), 640.0, 360.0, "")
    lms, kfs, cov = ba.bundle_adjustment(*args, covariance=True)
    assert calls[-1].get("ray_priors") is None and "ray_priors_used" not in ba.LAST_RESULT
    for f, kf in enumerate(kfs):
        li, ki = np.asarray(kf.landmark_index), np.asarray(kf.keypoint_index)
        assert len(li) == len(ki) > 0
        for l, k in zip(li.tolist(), ki.tolist()):  # the pair is a match of the graph
            hit = ((g.m_i == f) & (g.k1 == k) & (g.lm == l)) | ((g.m_j == f) & (g.k2 == k) & (g.lm == l))
            assert hit.any()
        np.testing.assert_array_equal(np.asarray(kf.feature_pts), np.asarray(g.keypoints[f])[ki])
    assert len(KeyFrame(None, 0, np.zeros(3), np.eye(3), 1.0, 1.0, 0.0, 0.0, 1.0).keypoint_index) == 0
    keyed = ptzba.ray_priors_from_result(kfs, lms, cov["ray_cov"], inflate=2.0)
    assert len(keyed) == M
    first = {}
    for kf in kfs:
        for l, k in zip(np.asarray(kf.landmark_index).tolist(), np.asarray(kf.keypoint_index).tolist()):
            first.setdefault(l, (kf.img_index, k))
    assert [(a, b) for a, b, _, _ in keyed] == [first[l] for l in range(M)]
    out = ba.bundle_adjustment(*args, ray_priors=keyed + [(12, 1, [0.0, 0.0], np.eye(2))])
    assert len(out) == 2
    rp = calls[-1]["ray_priors"]
    assert [r[0] for r in rp] == list(range(M))  # every key resolves back to its landmark
    for l, mean, info in rp:
        np.testing.assert_array_equal(mean, lms[l])
        np.testing.assert_allclose(np.linalg.inv(info), 2.0 * cov["ray_cov"][l], rtol=1e-12)
    assert ba.LAST_RESULT["ray_priors_used"] == M and ba.LAST_RESULT["ray_priors_skipped"] == [(12, 1)]
    # two keys of one landmark are two priors on it
    a, b = (10, 0), (11, 1)  # the match (0, 1): keypoint 0 of image 10 with keypoint 1 of image 11
    ba.bundle_adjustment(*args, ray_priors=[(a[0], a[1], [0.0, 0.0], np.eye(2)), (b[0], b[1], [1.0, 1.0], np.eye(2))])
    rp = calls[-1]["ray_priors"]
    assert len(rp) == 2 and rp[0][0] == rp[1][0]
