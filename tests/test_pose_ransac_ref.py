"""CPU checks of the pose-RANSAC yardstick (tests/pose_ransac_ref.py, the fp64 NumPy restatement the GPU tests
compare `ptz_pose_ransac` with): its minimal solver recovers the pose from noise-free pairs, and its full RANSAC
reproduces the figures recorded for case 1 of test_gpu_pose_ransac.py (scene seed 11, 96 correspondences, half of
them wrong, noise 0.5 px, 256 samples, RANSAC seed 7, threshold 3 px): the winner holds all 48 true inliers and no
reprojection error of any candidate lies within 4.8e-3 px of the threshold."""
import numpy as np
import pytest

import pose_ransac_ref as pr
from oracle import ptz_oracle as orc

U, V = 640.0, 360.0


def test_minimal_solver_recovers_noise_free_pose():
    rng = np.random.default_rng(0)
    done = 0
    while done < 200:
        gt = np.array([rng.uniform(40, 75), rng.uniform(-14, -4), rng.uniform(1800, 4300)])
        pix = rng.uniform(0.0, [1280.0, 720.0], (2, 2))
        if np.hypot(*(pix[0] - pix[1])) <= 200.0:
            continue
        done += 1
        th, ph = orc.from_image_to_ray(U, V, gt[2], gt[0], gt[1], pix[:, 0], pix[:, 1])
        p0, p1 = pr.ray_dirs(np.stack([th, ph], 1))
        a = pix - [U, V]
        cands = pr.minimal_solver((p0[0], p1[0]), (p0[1], p1[1]), a[0], a[1])
        assert 1 <= len(cands) <= 4
        assert [s for s, _ in cands] == sorted(s for s, _ in cands)
        err = min(np.max(np.abs((pr.cand_to_ptz(c) - gt) / [1.0, 1.0, 1000.0])) for _, c in cands)
        assert err < 1e-9, (gt, pix, err)  # degrees, and f / 1000


def test_degenerate_samples_give_no_candidate():
    assert pr.minimal_solver((0.1, 0.2), (0.1, 0.2), (10.0, 5.0), (10.0, 5.0)) == []  # the same ray twice
    # pixels 100 and 200 px out on the same side of the principal point are seen at most atan(1 / (2 sqrt 2)) =
    # 19.5 degrees apart, whatever f: rays 30 degrees apart have no solution
    assert pr.minimal_solver((0.0, 0.0), (np.tan(np.pi / 6), 0.0), (100.0, 0.0), (200.0, 0.0)) == []
    i, j = pr.sample(7, 3, 1)  # one correspondence: the second draw cannot differ
    assert i == j == 0


def test_full_ransac_case_1_figures():
    gt, rays, pts, truth = pr.make_scene(11, 96, 0.5, 0.5)
    assert truth.sum() == 48
    R = pr.pose_ransac_ref(U, V, rays, pts, 3.0, 256, 7)
    h, slot, c, ptz, count = R["cands"][R["best"]]
    assert count == 48 == max(k[4] for k in R["cands"])
    assert h == min(k[0] for k in R["cands"] if k[4] == 48)
    assert np.array_equal(pr.inlier_mask(ptz, rays, pts, U, V, 3.0), truth)
    assert 4.8e-3 < R["margin"] < 4.9e-3
    assert abs(ptz[0] - gt[0]) < 0.05 and abs(ptz[1] - gt[1]) < 0.05 and abs(ptz[2] - gt[2]) < 10.0
    # the sampling convention is the homography sampler's stream
    assert pr.sample(7, 0, 96) == (orc._ransac_draw(7, 0, 0, 0, 96), orc._ransac_sample(7, 0, 96)[1])


def test_random_forest_map_drops_its_nn_database_on_add_keyframe():
    """RandomForestMap.relocalize builds its descriptor -> ray database lazily; a new keyframe (and the BA it
    triggers, which moves the poses) invalidates it."""
    import key_frame
    import scene_map

    class Db:
        closed = 0

        def close(self):
            self.closed += 1

    rf = scene_map.RandomForestMap()
    rf.bundle_adjustment_processing = lambda: None
    db = rf._nn_map = Db()
    rf.add_keyframe(key_frame.KeyFrame(None, 0, np.zeros(3), np.eye(3), U, V, 50.0, -8.0, 2500.0))
    assert rf._nn_map is None and db.closed == 1
    rf.add_keyframe(key_frame.KeyFrame(None, 1, np.zeros(3), np.eye(3), U, V, 55.0, -8.0, 2500.0))
    assert rf._nn_map is None and len(rf.keyframe_list) == 2


def test_too_few_correspondences_is_an_error():
    """n_corr < 2 is an error return of the C entry point, before any device is touched."""
    import ptzba
    with pytest.raises(ptzba.PtzbaError, match="at least 2"):
        ptzba.pose_ransac(U, V, np.zeros((1, 2)), np.zeros((1, 2)))
    with pytest.raises(ValueError):
        ptzba.pose_ransac(U, V, np.zeros((3, 2)), np.zeros((2, 2)))
