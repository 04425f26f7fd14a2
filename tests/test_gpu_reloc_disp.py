"""GPU relocalisation under the displaced camera K (R p + d(f)): `ptz_pose_ransac_disp`,
`ptz_refine_poses_disp` and `ptz_back_project_rays_exact` against tests/reloc_disp_ref.py (fp64 NumPy) and scipy on
disp_ref.project's residual, and the maps built on them.  Displacement disp_ref.LAMBDA, u, v = 640, 360, RANSAC seed 7,
threshold 3 px.

The four scenes (scene seed, N, outlier fraction, noise px, samples) are test_gpu_pose_ransac.py's shapes seen through
the displaced camera (reloc_disp_ref.make_scene_disp): neither N nor the sample count a multiple of 64 or 256, 70 %
outliers, and more correspondences than one 1024-entry LDS tile of the scoring kernel.  The condition on the inputs,
asserted on the reference alone, is test_reloc_disp_cpu.py's: no candidate has a reprojection error within 1e-6 px of
the threshold (the nearest is 1.3e-2, 9.1e-3, 1.9e-4 and 9.6e-3 px)."""
import ctypes
import functools

import numpy as np
import pytest

import disp_ref
import pose_ransac_ref as pr
import reloc_disp_ref as rd
from disp_ref import LAMBDA

pytestmark = pytest.mark.gpu

U, V, SEED, THR = 640.0, 360.0, 7, 3.0
CASES = {1: (11, 96, 0.5, 0.5, 256), 2: (12, 67, 0.4, 0.5, 70), 5: (15, 300, 0.7, 0.5, 512),
         7: (16, 1100, 0.5, 0.5, 64)}


def _close(p, q, ang=1e-6, fpx=1e-4):
    assert abs(p[0] - q[0]) < ang and abs(p[1] - q[1]) < ang and abs(p[2] - q[2]) < fpx, (p, q)


@functools.lru_cache(maxsize=None)
def _case(scene_seed, n, outlier_frac, noise, n_hyp):
    """The scene, the reference's scored candidates and scipy's optimum on the true inliers."""
    gt, rays, pts, truth = rd.make_scene_disp(scene_seed, n, outlier_frac, noise)
    ref = rd.pose_ransac_ref_disp(U, V, rays, pts, LAMBDA, THR, n_hyp, SEED)
    opt = rd.scipy_optimum(gt, rays[truth], pts[truth], U, V, LAMBDA).x
    for a in (gt, rays, pts, truth, opt):
        a.setflags(write=False)
    return gt, rays, pts, truth, ref, opt


def _winner(ref):
    best = max(c[4] for c in ref["cands"])
    h = min(c[0] for c in ref["cands"] if c[4] == best)
    return best, h, [c[3] for c in ref["cands"] if c[0] == h]


def _is_candidate_of(ptz_hyp, cands):
    return any(abs(ptz_hyp[0] - c[0]) < 1e-9 and abs(ptz_hyp[1] - c[1]) < 1e-9 and
               abs(ptz_hyp[2] - c[2]) < 1e-9 * c[2] for c in cands)


def _same_result(r, r2):
    assert np.array_equal(r.ptz, r2.ptz) and np.array_equal(r.ptz_hyp, r2.ptz_hyp) and r.cost == r2.cost
    assert np.array_equal(r.mask, r2.mask)
    assert (r.found, r.best_sample, r.hyp_inliers, r.n_inliers) == (r2.found, r2.best_sample, r2.hyp_inliers,
                                                                     r2.n_inliers)


# ------------------------------------------------------------------------------------------------ pose RANSAC
@pytest.mark.parametrize("case", sorted(CASES))
def test_pose_ransac_matches_reference_and_scipy(gpu_available, case):
    import ptzba
    n_hyp = CASES[case][4]
    gt, rays, pts, truth, ref, opt = _case(*CASES[case])
    assert ref["margin"] > 1e-6  # the condition on the inputs
    best, h, cands = _winner(ref)
    kw = dict(threshold=THR, n_hyp=n_hyp, seed=SEED, ftol=1e-14, xtol=1e-14, displacement=LAMBDA)
    r = ptzba.pose_ransac(U, V, rays, pts, **kw)
    print("case", case, r, "reference:", best, h, "margin", ref["margin"], "scipy", opt)
    assert r.found
    assert r.hyp_inliers == best
    assert r.best_sample == h
    assert _is_candidate_of(r.ptz_hyp, cands), (r.ptz_hyp, cands)
    assert np.array_equal(r.mask, truth) and r.n_inliers == int(truth.sum())
    _close(r.ptz, opt)
    print("error against the ground truth (deg, deg, px):", np.abs(r.ptz - gt))
    _same_result(r, ptzba.pose_ransac(U, V, rays, pts, **kw))


def test_no_displacement_is_todays_call_bytewise(gpu_available):
    import ptzba
    gt, rays, pts, truth = pr.make_scene(11, 96, 0.5, 0.5)
    today = ptzba.pose_ransac(U, V, rays, pts, threshold=THR, n_hyp=256, seed=SEED)
    assert today.found
    for d in (None, np.zeros(6)):
        r = ptzba.pose_ransac(U, V, rays, pts, threshold=THR, n_hyp=256, seed=SEED, displacement=d)
        _same_result(today, r)
        assert today.ptz.tobytes() == r.ptz.tobytes() and today.ptz_hyp.tobytes() == r.ptz_hyp.tobytes()
    init = gt + np.random.default_rng(2).uniform(-1, 1, (16, 3)) * np.array([2.0, 1.0, 200.0])
    base = ptzba.refine_poses(U, V, init, rays[truth], pts[truth])
    for d in (None, np.zeros(6)):
        out = ptzba.refine_poses(U, V, init, rays[truth], pts[truth], displacement=d)
        for a, b in zip(base, out):
            assert a.tobytes() == b.tobytes()


def test_refusals(gpu_available):
    """A NaN in the displacement and n_corr < 2 are refused with a message, the outputs as the caller left them."""
    import ptzba
    gt, rays, pts, truth, _, _ = _case(*CASES[1])
    L = ptzba.lib()
    bad = LAMBDA.copy()
    bad[2] = np.nan
    rays, pts = np.ascontiguousarray(rays), np.ascontiguousarray(pts)
    ptz = np.array([[1.0, 2.0, 3.0]])
    cost = np.array([-5.0])
    rc = L.ptz_refine_poses_disp(0, 1, ptzba._ptr(ptz), len(rays), ptzba._ptr(rays), ptzba._ptr(pts), U, V, None, None,
                                 None, ptzba._ptr(cost), None, None, ptzba._ptr(bad))
    assert rc != 0 and b"non-finite" in L.ptzba_last_error()
    assert np.array_equal(ptz, [[1.0, 2.0, 3.0]]) and cost[0] == -5.0
    for n, d6, word in ((len(rays), bad, b"non-finite"), (1, LAMBDA.copy(), b"at least 2")):
        out = np.array([-1.0, -2.0, -3.0])
        hyp = np.array([-4.0, -5.0, -6.0])
        mask = np.full(len(rays), 7, np.uint8)
        smp, hin, nin, st = (ctypes.c_int32(-7) for _ in range(4))
        c = ctypes.c_double(-5.0)
        rc = L.ptz_pose_ransac_disp(0, n, ptzba._ptr(rays), ptzba._ptr(pts), U, V, None, ptzba._ptr(out),
                                    ptzba._ptr(hyp), ctypes.byref(smp), ctypes.byref(hin), ptzba._ptr(mask),
                                    ctypes.byref(nin), ctypes.byref(c), ctypes.byref(st), ptzba._ptr(d6))
        assert rc != 0 and word in L.ptzba_last_error()
        assert np.array_equal(out, [-1.0, -2.0, -3.0]) and np.array_equal(hyp, [-4.0, -5.0, -6.0])
        assert (mask == 7).all() and c.value == -5.0
        assert [x.value for x in (smp, hin, nin, st)] == [-7] * 4
    with pytest.raises(ptzba.PtzbaError):
        ptzba.pose_ransac(U, V, rays, pts, displacement=bad)
    with pytest.raises(ptzba.PtzbaError):
        ptzba.refine_poses(U, V, ptz, rays, pts, displacement=bad)


# ------------------------------------------------------------------------------------------------ pose LM
def test_refine_multistart_converges_to_scipy(gpu_available):
    import ptzba
    gt, rays, pts, truth, _, opt = _case(*CASES[1])
    init = opt + np.random.default_rng(0).uniform(-1, 1, (64, 3)) * np.array([2.0, 1.0, 200.0])
    ptz, cost, its, st = ptzba.refine_poses(U, V, init, rays[truth], pts[truth], ftol=1e-14, xtol=1e-14,
                                            displacement=LAMBDA)
    ref_cost = 0.5 * float(np.sum(rd.residual(opt, rays[truth], pts[truth], U, V, LAMBDA) ** 2))
    for k in range(64):
        _close(ptz[k], opt)
        assert abs(cost[k] - ref_cost) <= 1e-9 * ref_cost


@pytest.mark.parametrize("loss", [0, 1])
def test_refine_subsets_match_scipy(gpu_available, loss):
    """Sixteen hypotheses, each on its own 32-correspondence CSR subset, linear and Huber (f_scale 1)."""
    import ptzba
    gt, rays, pts, truth, _, _ = _case(*CASES[1])
    r, p = rays[truth], pts[truth]
    rng = np.random.default_rng(1)
    subsets = [rng.choice(len(r), 32, replace=False) for _ in range(16)]
    x0 = gt + [0.5, 0.3, 50.0]
    ptz, cost, its, st = ptzba.refine_poses(U, V, np.repeat(x0[None], 16, 0), r, p, subsets=subsets, ftol=1e-14,
                                            xtol=1e-14, loss=loss, f_scale=1.0, displacement=LAMBDA)
    for k, s in enumerate(subsets):
        ref = rd.scipy_optimum(x0, r[s], p[s], U, V, LAMBDA, loss='huber' if loss else 'linear', f_scale=1.0)
        _close(ptz[k], ref.x)
        assert abs(cost[k] - ref.cost) <= 1e-7 * ref.cost


def test_refine_three_correspondences(gpu_available):
    import ptzba
    gt, rays, pts, truth, _, _ = _case(*CASES[1])
    r, p = rays[truth][:3], pts[truth][:3]
    x0 = gt + [0.5, 0.3, 50.0]
    ref = rd.scipy_optimum(x0, r, p, U, V, LAMBDA).x
    ptz, cost, its, st = ptzba.refine_poses(U, V, x0[None], r, p, ftol=1e-14, xtol=1e-14, displacement=LAMBDA)
    _close(ptz[0], ref)


# ------------------------------------------------------------------------------------------------ exact inverse
def test_exact_back_projection_round_trip(gpu_available):
    import ptzba
    rng = np.random.default_rng(4)
    worst = 0.0
    for n in (1, 67, 300):  # below a wave, not a multiple of 64, more than one 256-thread block
        pose = np.array([rng.uniform(40, 65), rng.uniform(-14, -4), rng.uniform(1800, 4300)])
        pix = rng.uniform(0.0, [1280.0, 720.0], (n, 2))
        rays, valid = ptzba.back_project_rays(U, V, pose[2], pose[0], pose[1], pix, LAMBDA, exact=True)
        assert valid.dtype == bool and valid.all() and rays.shape == (n, 2)
        xy = ptzba.project_rays(U, V, pose[2], pose[0], pose[1], rays, LAMBDA)
        worst = max(worst, float(np.abs(xy - pix).max()))
        ref, _ = rd.back_project_exact(U, V, pose[2], pose[0], pose[1], pix, LAMBDA)
        np.testing.assert_allclose(rays, ref, rtol=0, atol=1e-11)
    print("exact back-projection round trip, worst px:", worst)
    assert worst <= 1e-9
    # a pixel behind the (theta, phi) chart
    rays, valid = ptzba.back_project_rays(U, V, 2000.0, 85.0, -8.0, [[1279.0, 360.0], [640.0, 360.0]], LAMBDA,
                                          exact=True)
    assert not valid[0] and np.isnan(rays[0]).all()
    assert valid[1] and np.isfinite(rays[1]).all()
    # valid_out may be NULL
    pix = np.ascontiguousarray([[100.0, 200.0]])
    out = np.zeros((1, 2))
    assert ptzba.lib().ptz_back_project_rays_exact(0, 1, U, V, 2000.0, 50.0, -8.0, ptzba._ptr(LAMBDA.copy()),
                                                   ptzba._ptr(pix), ptzba._ptr(out), None) == 0
    assert np.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ the maps
KF_POSES = np.array([[45.0, -9.0, 2500.0], [52.0, -8.0, 2600.0], [60.0, -9.5, 2400.0]])
Q_POSE = np.array([55.0, -8.7, 2700.0])
RELOC = dict(threshold=3.0, n_hyp=1024, seed=0, ftol=1e-14, xtol=1e-14)


def _visible(pose, rays):
    xy, q2 = disp_ref.project(U, V, np.tile(pose, (len(rays), 1)), rays, LAMBDA)
    keep = np.flatnonzero((q2 > 0) & (xy[:, 0] > 0) & (xy[:, 0] < 1280) & (xy[:, 1] > 0) & (xy[:, 1] < 720))
    return keep, xy[keep]


@functools.lru_cache(maxsize=None)
def _map_scene():
    """700 rays with their own integer descriptors seen through the displaced camera: three keyframes (noise-free
    features) and a lost frame at Q_POSE with 0.3 px noise and 30 % of its descriptors swapped for those of other
    rays of the map.  Returns (frames, lost points, lost descriptors, true-match flags, scipy's optimum on the true
    matches)."""
    rng = np.random.default_rng(21)
    rays = np.stack([rng.uniform(30, 80, 700), rng.uniform(-17, -1, 700)], 1)
    des = rng.integers(0, 256, (700, 128)).astype(np.float32)
    frames = []
    for pose in KF_POSES:
        idx, pts = _visible(pose, rays)
        frames.append((pose, pts, des[idx]))
    in_map = np.unique(np.concatenate([_visible(pose, rays)[0] for pose in KF_POSES]))
    idx, pts = _visible(Q_POSE, rays)
    seen = np.isin(idx, in_map)
    idx, pts = idx[seen], pts[seen]
    q_pts = pts + rng.normal(0.0, 0.3, pts.shape)
    q_des = des[idx].copy()
    wrong = rng.choice(len(idx), int(round(0.3 * len(idx))), replace=False)
    matched = idx.copy()
    for k in wrong:
        matched[k] = rng.choice(in_map[in_map != idx[k]])
        q_des[k] = des[matched[k]]
    good = np.ones(len(idx), bool)
    good[wrong] = False
    opt = rd.scipy_optimum(Q_POSE, rays[idx[good]], q_pts[good], U, V, LAMBDA).x
    # the condition on the inputs: at the optimum the true matches, and no wrong one, lie within the threshold
    assert np.array_equal(rd.inlier_mask_disp(opt, rays[matched], q_pts, U, V, LAMBDA, 3.0), good)
    assert good.sum() >= 30
    return frames, q_pts, q_des, good, opt


def _keyframes(displacement=None):
    import key_frame
    out = []
    for k, (pose, pts, des) in enumerate(_map_scene()[0]):
        kf = key_frame.KeyFrame(None, k, np.zeros(3), np.eye(3), U, V, pose[0], pose[1], pose[2])
        kf.feature_pts = pts.copy()
        kf.feature_des = des.copy()
        if displacement is not None:
            kf.displacement = displacement
        out.append(kf)
    return out


def _lost():
    import key_frame
    _, q_pts, q_des, _, _ = _map_scene()
    kf = key_frame.KeyFrame(None, -1, np.zeros(3), np.eye(3), U, V, 0.0, 0.0, 1000.0)  # its pose is not read
    kf.feature_pts = q_pts.copy()
    kf.feature_des = q_des.copy()
    return kf


def test_nn_map_relocalises_under_the_displacement(gpu_available):
    import nearest_neighbor
    frames, q_pts, q_des, good, opt = _map_scene()
    m = nearest_neighbor.NNBasedMap(displacement=LAMBDA)
    try:
        m.add_keyframes(_keyframes())
        assert len(m.global_ray) == len(m.global_des) == sum(len(f[1]) for f in frames)
        # the stored rays are the exact inverse projections
        pose, pts, _ = frames[0]
        xy, _ = disp_ref.project(U, V, np.tile(pose, (len(pts), 1)), m.global_ray[:len(pts)], LAMBDA)
        assert np.abs(xy - pts).max() <= 1e-9
        ptz, n_inliers, found = m.relocalize_robust(_lost(), **RELOC)
        print("displaced map:", ptz, n_inliers, found, "scipy", opt, "truth", Q_POSE)
        assert found and n_inliers == int(good.sum())
        _close(ptz, opt)
        res = m.compute_residual(opt, m.global_ray[:len(pts)], pts, U, V, displacement=m.displacement)
        np.testing.assert_allclose(res, rd.residual(opt, m.global_ray[:len(pts)], pts, U, V, LAMBDA), atol=1e-8)
    finally:
        m.close()
    # the same map without the displacement
    m = nearest_neighbor.NNBasedMap()
    try:
        m.add_keyframes(_keyframes())
        ptz, n_inliers, found = m.relocalize_robust(_lost(), **RELOC)
        print("displacement-free map:", ptz, n_inliers, found)
        assert (not found) or max(abs(ptz[0] - opt[0]), abs(ptz[1] - opt[1])) > 0.1 or abs(ptz[2] - opt[2]) > 10.0
    finally:
        m.close()


def test_random_forest_map_reloc_displacement(gpu_available):
    import scene_map
    opt = _map_scene()[4]
    rf = scene_map.RandomForestMap(reloc_displacement=True)
    rf.keyframe_list = _keyframes(displacement=LAMBDA)
    rf.reloc_options = dict(RELOC)
    lost = [10.0, -5.0, 1500.0]
    try:
        pose = rf.relocalize(_lost(), lost)
        assert np.array_equal(rf._nn_map.displacement, LAMBDA)
        _close(pose, opt)
    finally:
        rf._drop_nn_map()


class _FrontEnd:
    """Detector / matcher hooks over known rays seen through the displaced camera: an 'image' is an index into
    `cams`; keypoints are the displaced projections inside the image plus 0.3 px noise, descriptors carry the ray id."""

    def __init__(self, rays, cams):
        self.rays, self.cams = rays, cams

    def detect(self, im, nfeatures=0, verbose=False):
        import image_process
        idx, pts = _visible(self.cams[int(im)], self.rays)
        if nfeatures:
            idx, pts = idx[:nfeatures], pts[:nfeatures]
        pts = pts + np.random.default_rng(100 + int(im)).normal(0.0, 0.3, pts.shape)
        keep = (pts[:, 0] > 1) & (pts[:, 0] < 1279) & (pts[:, 1] > 1) & (pts[:, 1] < 719)  # the mask is indexed by pixel
        idx, pts = idx[keep], pts[keep]
        des = np.zeros((len(idx), 128), np.float32)
        des[:, 1] = idx
        return image_process.KeyPoint.from_rows(pts, np.ones(len(idx)), np.zeros(len(idx)), np.ones(len(idx))), des

    @staticmethod
    def match(kp1, des1, kp2, des2, pts_array=False, verbose=False):
        r1, r2 = np.asarray(des1)[:, 1].astype(np.int64), np.asarray(des2)[:, 1].astype(np.int64)
        pos2 = {int(r): j for j, r in enumerate(r2)}
        idx1 = [i for i, r in enumerate(r1) if int(r) in pos2]
        idx2 = [pos2[int(r1[i])] for i in idx1]
        if len(idx1) <= 8:
            return None, [], None, []
        p1 = np.asarray(kp1, np.float64).reshape(-1, 2)[idx1]
        p2 = np.asarray(kp2, np.float64).reshape(-1, 2)[idx2]
        return p1, np.array(idx1, np.int32), p2, np.array(idx2, np.int32)


def test_relocalization_camera_displacement(gpu_available, monkeypatch):
    """relocalization_camera(displacement=): the rays handed to the LM are the exact inverse projections of the
    matched keyframe's points (each within 0.05 degrees of its scene ray; the approximate inverse is degrees off), the
    LM runs under the displacement, and the pose is scipy's optimum on those rays and points."""
    import image_process
    import key_frame
    import ptzba
    import relocalization
    import scene_map
    rng = np.random.default_rng(33)
    rays = np.stack([rng.uniform(30, 80, 400), rng.uniform(-17, -1, 400)], 1)
    cams = np.vstack([KF_POSES, Q_POSE[None]])
    fe = _FrontEnd(rays, cams)
    monkeypatch.setattr(image_process, "detect_compute_sift", fe.detect)
    monkeypatch.setattr(image_process, "match_sift_features", fe.match)
    seen = {}
    refine = ptzba.refine_poses

    def spy(u, v, init, r, p, **kw):
        seen.update(rays=np.array(r), points=np.array(p), kw=kw)
        return refine(u, v, init, r, p, **kw)

    monkeypatch.setattr(ptzba, "refine_poses", spy)
    m = scene_map.Map('sift', cache_correspondences=False)
    for k in range(3):
        m.keyframe_list.append(key_frame.KeyFrame(k, k, np.zeros(3), np.eye(3), U, V, *cams[k]))
    lost = Q_POSE + [1.0, 0.5, 100.0]
    pose = relocalization.relocalization_camera(m, 3, lost, ftol=1e-14, displacement=LAMBDA)
    assert np.array_equal(seen["kw"]["displacement"], LAMBDA) and len(seen["rays"]) > 8
    d = np.abs(seen["rays"][:, None, :] - rays[None, :, :]).max(axis=2).min(axis=1)
    assert d.max() < 0.05, d.max()
    opt = rd.scipy_optimum(lost, seen["rays"], seen["points"], U, V, LAMBDA).x
    # relocalization_camera leaves xtol at its default 1e-8 (relative step): 1e-6 degrees / 1e-4 px hold beyond it
    _close(pose, opt)
    d = np.abs(pose - Q_POSE)
    assert max(d[0], d[1]) < 0.01 and d[2] < 2.0, (pose, Q_POSE)
