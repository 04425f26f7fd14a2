"""GPU nearest-neighbour ray map (nearest_neighbor.NNBasedMap) and the relocalisation built on it:
`find_nearest` against the oracle's exact kNN, `relocalize_robust` (find_nearest + ptz_pose_ransac) end to end on a
synthetic ray scene with wrong matches, the contrast with the reference-style `relocalize`, and
`RandomForestMap.relocalize`, which stands in for the reference's forest.

Scene: 700 rays (pan 20..90, tilt -17..-1 degrees), each with its own integer-valued 128-d descriptor; 4 keyframes at
pan 40 / 50 / 60 / 70 see the rays that project into 1280 x 720.  The query frame sits at pan 55 (5 degrees from the
nearest keyframes); its points carry 0.3 px noise and 30 % of its descriptors are replaced by descriptors of other
database rays, so they match wrong rays."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U, V = 640.0, 360.0
KF_POSES = np.array([[40.0, -9.0, 2500.0], [50.0, -8.0, 2600.0], [60.0, -9.5, 2400.0], [70.0, -8.5, 2500.0]])
Q_POSE = np.array([55.0, -8.7, 2700.0])


def _visible(pose, rays):
    from oracle import ptz_oracle as orc
    pts = orc.project_rays(U, V, pose[2], pose[0], pose[1], rays)
    keep = np.flatnonzero((pts[:, 0] > 0) & (pts[:, 0] < 1280) & (pts[:, 1] > 0) & (pts[:, 1] < 720))
    return keep, pts[keep]


@functools.lru_cache(maxsize=None)
def _scene():
    rng = np.random.default_rng(21)
    rays = np.stack([rng.uniform(20, 90, 700), rng.uniform(-17, -1, 700)], 1)
    des = rng.integers(0, 256, (700, 128)).astype(np.float32)
    frames = []
    for pose in KF_POSES:
        idx, pts = _visible(pose, rays)
        frames.append((pose, idx, pts))
    in_map = np.unique(np.concatenate([f[1] for f in frames]))
    idx, pts = _visible(Q_POSE, rays)
    seen = np.isin(idx, in_map)
    idx, pts = idx[seen], pts[seen]
    q_pts = pts + rng.normal(0.0, 0.3, pts.shape)
    q_des = des[idx].copy()
    wrong = rng.choice(len(idx), int(round(0.3 * len(idx))), replace=False)
    for k in wrong:  # the descriptor of another ray of the map
        q_des[k] = des[rng.choice(in_map[in_map != idx[k]])]
    return rays, des, frames, q_pts, q_des, len(idx) - len(wrong)


def _keyframes():
    import key_frame
    rays, des, frames, _, _, _ = _scene()
    out = []
    for k, (pose, idx, pts) in enumerate(frames):
        kf = key_frame.KeyFrame(None, k, np.zeros(3), np.eye(3), U, V, pose[0], pose[1], pose[2])
        kf.feature_pts = pts.copy()
        kf.feature_des = des[idx].copy()
        out.append(kf)
    return out


def _query(pose, pts, des):
    import key_frame
    kf = key_frame.KeyFrame(None, -1, np.zeros(3), np.eye(3), U, V, pose[0], pose[1], pose[2])
    kf.feature_pts = np.array(pts)
    kf.feature_des = np.array(des)
    return kf


def _near(p, q):
    return abs(p[0] - q[0]) < 0.01 and abs(p[1] - q[1]) < 0.01 and abs(p[2] - q[2]) < 2.0


def test_find_nearest_equals_exact_knn(gpu_available):
    import key_frame
    import nearest_neighbor
    from oracle import ptz_oracle as orc
    rng = np.random.default_rng(5)
    m = nearest_neighbor.NNBasedMap()
    try:
        for k in range(4):
            kf = key_frame.KeyFrame(None, k, np.zeros(3), np.eye(3), U, V, 50.0 + k, -8.0, 2500.0)
            kf.feature_pts = np.stack([rng.uniform(0, 1280, 50), rng.uniform(0, 720, 50)], 1)
            kf.feature_des = rng.integers(0, 256, (50, 128)).astype(np.float32)
            m.add_keyframe_without_ba(kf)
        assert m.global_des.shape == (200, 128) and m.global_ray.shape == (200, 2)
        m.build_kdtree()
        rows = rng.choice(200, 40, replace=False)
        q = np.concatenate([m.global_des[rows] + rng.integers(-2, 3, (40, 128)),
                            rng.integers(0, 256, (20, 128))]).astype(np.float32)
        q = q[rng.permutation(60)]
        idx, dist = orc.knn2(q, m.global_des)
        d2 = dist[:, 0] ** 2
        assert np.all(np.abs(d2 - 2000.0) > 1.0)
        keep = np.flatnonzero(d2 < 2000.0)
        assert len(keep) == 40
        kp_index, ray_index = m.find_nearest(q)
        assert kp_index == keep.tolist()
        assert ray_index == idx[keep, 0].tolist()
        # rays were back-projected at the keyframe's pose
        kf0 = m.keyframe_list[0]
        np.testing.assert_allclose(m.global_ray[:50], orc.back_project_to_rays(U, V, kf0.f, kf0.pan, kf0.tilt,
                                                                                kf0.feature_pts), atol=1e-9)
    finally:
        m.close()


def test_relocalize_robust_end_to_end(gpu_available):
    import nearest_neighbor
    rays, des, frames, q_pts, q_des, n_good = _scene()
    assert n_good >= 30
    m = nearest_neighbor.NNBasedMap()
    try:
        m.add_keyframes(_keyframes())
        # the pose of the query keyframe is not read: hand over a useless one
        ptz, n_inliers, found = m.relocalize_robust(_query([0.0, 0.0, 1000.0], q_pts, q_des), threshold=3.0,
                                                    n_hyp=1024, seed=0)
        print("robust", ptz, n_inliers, found, "truth", Q_POSE, "good matches", n_good)
        assert found and n_inliers >= n_good - 2
        assert _near(ptz, Q_POSE), (ptz, Q_POSE)
        # the reference's relocalize: least squares over every match from a pose 3 degrees off
        ls = m.relocalize(_query(Q_POSE + [3.0, 0.0, 0.0], q_pts, q_des))
        print("least squares", ls)
        assert not _near(ls, Q_POSE), (ls, Q_POSE)
        # without wrong matches the same call does find the pose
        good = m.relocalize(_query(Q_POSE + [3.0, 0.0, 0.0], q_pts, _clean_des()))
        assert _near(good, Q_POSE), (good, Q_POSE)
    finally:
        m.close()


def _clean_des():
    rays, des, frames, q_pts, q_des, _ = _scene()
    in_map = np.unique(np.concatenate([f[1] for f in frames]))
    idx, _ = _visible(Q_POSE, rays)
    return des[idx[np.isin(idx, in_map)]]


def test_random_forest_map_relocalize(gpu_available):
    import scene_map
    rays, des, frames, q_pts, q_des, n_good = _scene()
    rf = scene_map.RandomForestMap()
    rf.keyframe_list = _keyframes()
    lost = [10.0, -5.0, 1500.0]
    pose = rf.relocalize(_query(lost, q_pts, q_des), lost)
    assert _near(pose, Q_POSE), (pose, Q_POSE)
    # nothing matches: the pose passed in comes back
    rng = np.random.default_rng(9)
    junk = rng.integers(0, 256, q_des.shape).astype(np.float32)
    back = rf.relocalize(_query(lost, q_pts, junk), lost)
    assert np.array_equal(back, lost)
    rf._drop_nn_map()
