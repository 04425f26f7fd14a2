"""CPU checks of relocalisation under the displaced camera: the yardstick tests/reloc_disp_ref.py (the
exact inverse projection, the displaced two-point minimal solver and its scored candidate list, which
test_gpu_reloc_disp.py compares the kernels with), and the host side of the feature (keywords, prototypes, refusals
that need no device, how the maps resolve their displacement).  Displacement disp_ref.LAMBDA, u, v = 640, 360.

The four scenes (scene seed, N, outlier fraction, noise px, samples) = (11, 96, 0.5, 0.5, 256), (12, 67, 0.4, 0.5, 70),
(15, 300, 0.7, 0.5, 512), (16, 1100, 0.5, 0.5, 64), RANSAC seed 7, threshold 3 px.  Measured with the analytic dg/df
(six Newton steps): the nearest reprojection error of any candidate to the threshold is 1.3e-2, 9.1e-3, 1.9e-4 and
9.6e-3 px (the condition is > 1e-6 px); the winners hold 48, 40, 90 and 550 inliers, exactly the true ones; the
displacement-free pose_ransac_ref wins with 9, 8, 11 and 54 of them on the same scenes.  The exact inverse returns
to its pixel within 1.4e-12 px (300 poses x 50 pixels); the reference's back_project_to_ray is 128 px off in the median
there; all 2,000 noise-free pairs give back their pose."""
import ctypes
import functools
import inspect
import os

import numpy as np
import pytest

import disp_ref
import pose_ransac_ref as pr
import reloc_disp_ref as rd
from disp_ref import LAMBDA
from oracle import ptz_oracle as orc

U, V, SEED, THR = 640.0, 360.0, 7, 3.0
SCENES = [(11, 96, 0.5, 0.5, 256), (12, 67, 0.4, 0.5, 70), (15, 300, 0.7, 0.5, 512), (16, 1100, 0.5, 0.5, 64)]
TRUE_INLIERS = {11: 48, 12: 40, 15: 90, 16: 550}


def _pose(rng):
    return np.array([rng.uniform(40, 65), rng.uniform(-14, -4), rng.uniform(1800, 4300)])


@functools.lru_cache(maxsize=None)
def _round_trip_data():
    rng = np.random.default_rng(0)
    out = []
    for _ in range(300):
        gt = _pose(rng)
        pix = rng.uniform(0.0, [1280.0, 720.0], (50, 2))
        out.append((gt, pix))
    return out


def test_exact_inverse_round_trip():
    worst = 0.0
    for gt, pix in _round_trip_data():
        rays, valid = rd.back_project_exact(U, V, gt[2], gt[0], gt[1], pix, LAMBDA)
        assert valid.all()
        xy, q2 = disp_ref.project(U, V, np.tile(gt, (len(pix), 1)), rays, LAMBDA)
        assert (q2 > 0).all()
        worst = max(worst, float(np.abs(xy - pix).max()))
    print("exact inverse round trip, worst px:", worst)
    assert worst <= 1e-9


def test_approximate_inverse_stays_discriminating():
    """The reference's back_project_to_ray on the same data is far off: the round trip above is not a property of
    every inverse at hand."""
    err = []
    for gt, pix in _round_trip_data():
        rays = orc.back_project_to_rays(U, V, gt[2], gt[0], gt[1], pix, LAMBDA)
        xy, _ = disp_ref.project(U, V, np.tile(gt, (len(pix), 1)), rays, LAMBDA)
        err.append(np.hypot(xy[:, 0] - pix[:, 0], xy[:, 1] - pix[:, 1]))
    med = float(np.median(np.concatenate(err)))
    print("approximate inverse round trip, median px:", med)
    assert med > 10.0


def test_exact_inverse_flags_pixels_without_a_ray():
    rays, valid = rd.back_project_exact(U, V, 2000.0, 85.0, -8.0, [[1279.0, 360.0], [640.0, 360.0]], LAMBDA)
    assert not valid[0] and np.isnan(rays[0]).all()
    assert valid[1] and np.isfinite(rays[1]).all()


def test_zero_displacement_exact_inverse_is_from_image_to_ray():
    gt, pix = _round_trip_data()[0]
    rays, valid = rd.back_project_exact(U, V, gt[2], gt[0], gt[1], pix, disp_ref.ZERO)
    th, ph = orc.from_image_to_ray(U, V, gt[2], gt[0], gt[1], pix[:, 0], pix[:, 1])
    assert valid.all()
    np.testing.assert_allclose(rays, np.stack([th, ph], 1), rtol=0, atol=1e-11)


def _pair(rng):
    gt = _pose(rng)
    pix = rng.uniform(0.0, [1280.0, 720.0], (2, 2))
    rays, valid = rd.back_project_exact(U, V, gt[2], gt[0], gt[1], pix, LAMBDA)
    assert valid.all()
    p0, p1 = pr.ray_dirs(rays)
    return gt, (p0[0], p1[0]), (p0[1], p1[1]), pix[0] - [U, V], pix[1] - [U, V]


def test_analytic_slope_of_g():
    rng = np.random.default_rng(3)
    for _ in range(50):
        gt, pi, pj, ai, aj = _pair(rng)
        f = gt[2] * rng.uniform(0.8, 1.2)
        g, gp = rd.g_and_slope(pi, pj, ai, aj, f, LAMBDA)
        h = 1e-3
        fd = (rd.g_and_slope(pi, pj, ai, aj, f + h, LAMBDA)[0] - rd.g_and_slope(pi, pj, ai, aj, f - h, LAMBDA)[0]) / (2 * h)
        # g is O(1) with rounding 1e-16: the central difference carries 1e-13 of noise, and h^2 g''' / 6 of truncation
        assert abs(gp - fd) <= 1e-6 * abs(gp) + 1e-12, (gp, fd)


def test_noise_free_pairs_recover_the_pose():
    """The true pose is among the candidates to 1e-8 degrees / 1e-8 f on at least 99 % of 2,000 random pairs (the
    misses are degenerate pairs)."""
    rng = np.random.default_rng(1)
    miss = 0
    for _ in range(2000):
        gt, pi, pj, ai, aj = _pair(rng)
        ok = False
        for _, c in rd.minimal_solver_disp(pi, pj, ai, aj, LAMBDA):
            ptz = pr.cand_to_ptz(c)
            ok = ok or (abs(ptz[0] - gt[0]) < 1e-8 and abs(ptz[1] - gt[1]) < 1e-8 and abs(ptz[2] - gt[2]) < 1e-8 * gt[2])
        miss += 0 if ok else 1
    print("noise-free pairs without their pose:", miss, "of 2000")
    assert miss < 20


@functools.lru_cache(maxsize=None)
def _scene(scene_seed, n, outlier_frac, noise, n_hyp):
    gt, rays, pts, truth = rd.make_scene_disp(scene_seed, n, outlier_frac, noise)
    ref = rd.pose_ransac_ref_disp(U, V, rays, pts, LAMBDA, THR, n_hyp, SEED)
    return gt, rays, pts, truth, ref


@pytest.mark.parametrize("scene", SCENES, ids=[str(s[0]) for s in SCENES])
def test_scene_winner_holds_the_true_inliers(scene):
    gt, rays, pts, truth, ref = _scene(*scene)
    n_true = TRUE_INLIERS[scene[0]]
    assert int(truth.sum()) == n_true
    print("scene", scene, "margin", ref["margin"], "candidates", len(ref["cands"]))
    assert ref["margin"] > 1e-6
    h, slot, c, ptz, count = ref["cands"][ref["best"]]
    assert count == n_true
    assert np.array_equal(rd.inlier_mask_disp(ptz, rays, pts, U, V, LAMBDA, THR), truth)
    # the displacement-free solver on the same scene explains fewer than half of them
    free = pr.pose_ransac_ref(U, V, rays, pts, THR, scene[4], SEED)
    free_count = free["cands"][free["best"]][4] if free["best"] is not None else 0
    print("displacement-free winner:", free_count)
    assert free_count < n_true / 2


def test_zero_displacement_gives_the_closed_form_candidates():
    gt, rays, pts, truth = pr.make_scene(11, 96, 0.5, 0.5)
    a = pr.pose_ransac_ref(U, V, rays, pts, THR, 256, SEED)
    b = rd.pose_ransac_ref_disp(U, V, rays, pts, disp_ref.ZERO, THR, 256, SEED)
    assert [(c[0], c[1], c[4]) for c in a["cands"]] == [(c[0], c[1], c[4]) for c in b["cands"]]
    assert a["best"] == b["best"]
    for ca, cb in zip(a["cands"], b["cands"]):
        assert abs(ca[3][0] - cb[3][0]) < 1e-9 and abs(ca[3][1] - cb[3][1]) < 1e-9
        assert abs(ca[3][2] - cb[3][2]) < 1e-9 * ca[3][2]


# ------------------------------------------------------------------------------------------------ the host side
def test_keywords_and_prototypes():
    import nearest_neighbor
    import ptzba
    import relocalization
    import scene_map
    assert inspect.signature(ptzba.back_project_rays).parameters["exact"].default is False
    assert inspect.signature(ptzba.refine_poses).parameters["displacement"].default is None
    assert inspect.signature(ptzba.pose_ransac).parameters["displacement"].default is None
    assert inspect.signature(relocalization.relocalization_camera).parameters["displacement"].default is None
    assert inspect.signature(nearest_neighbor.NNBasedMap.__init__).parameters["displacement"].default is None
    assert inspect.signature(scene_map.Map.__init__).parameters["reloc_displacement"].default is False
    assert inspect.signature(scene_map.RandomForestMap.__init__).parameters["reloc_displacement"].default is False
    for name in ("ptz_back_project_rays_exact", "ptz_refine_poses_disp", "ptz_pose_ransac_disp"):
        assert name in ptzba.EXPORTED_SYMBOLS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptzba.h")).read()
    for name, n_args in (("ptz_back_project_rays_exact", 11), ("ptz_refine_poses_disp", 15),
                         ("ptz_pose_ransac_disp", 16)):
        assert "PTZBA_EXPORT int %s(" % name in header
        if os.path.exists(ptzba.LIB_PATH):
            fn = getattr(ptzba.lib(), name)
            assert len(fn.argtypes) == n_args and fn.restype is ctypes.c_int
    if os.path.exists(ptzba.LIB_PATH):
        assert b"ptzba 0.10" in ptzba.lib().ptzba_version()


def test_refusals_need_no_device():
    """A non-finite displacement and n_corr < 2 are refused before anything touches a device; the outputs stay."""
    import ptzba
    if not os.path.exists(ptzba.LIB_PATH):
        pytest.skip("libptzba.so is not built")
    L = ptzba.lib()
    bad = LAMBDA.copy()
    bad[4] = np.nan
    rays = np.ascontiguousarray(np.array([[50.0, -8.0], [51.0, -9.0], [52.0, -7.0]]))
    pts = np.ascontiguousarray(np.array([[100.0, 200.0], [300.0, 400.0], [500.0, 100.0]]))
    ptz = np.array([[1.0, 2.0, 3.0]])
    rc = L.ptz_refine_poses_disp(0, 1, ptzba._ptr(ptz), 3, ptzba._ptr(rays), ptzba._ptr(pts), U, V, None, None, None,
                                 None, None, None, ptzba._ptr(bad))
    assert rc != 0 and b"non-finite" in L.ptzba_last_error()
    assert np.array_equal(ptz, [[1.0, 2.0, 3.0]])
    out = np.array([-1.0, -2.0, -3.0])
    hyp = np.array([-4.0, -5.0, -6.0])
    mask = np.full(3, 7, np.uint8)
    st = ctypes.c_int32(-7)
    for n, d6, word in ((3, bad, b"non-finite"), (1, LAMBDA.copy(), b"at least 2")):
        rc = L.ptz_pose_ransac_disp(0, n, ptzba._ptr(rays), ptzba._ptr(pts), U, V, None, ptzba._ptr(out),
                                    ptzba._ptr(hyp), None, None, ptzba._ptr(mask), None, None, ctypes.byref(st),
                                    ptzba._ptr(d6))
        assert rc != 0 and word in L.ptzba_last_error()
        assert np.array_equal(out, [-1.0, -2.0, -3.0]) and np.array_equal(hyp, [-4.0, -5.0, -6.0])
        assert (mask == 7).all() and st.value == -7
    rc = L.ptz_back_project_rays_exact(0, 3, U, V, 2000.0, 50.0, -8.0, ptzba._ptr(bad), ptzba._ptr(pts),
                                       ptzba._ptr(rays), None)
    assert rc != 0 and b"non-finite" in L.ptzba_last_error()
    with pytest.raises(ptzba.PtzbaError):
        ptzba.refine_poses(U, V, ptz, rays, pts, displacement=bad)
    with pytest.raises(ptzba.PtzbaError):
        ptzba.pose_ransac(U, V, rays, pts, displacement=bad)


def _kf(i, displacement=None):
    from key_frame import KeyFrame
    k = KeyFrame(i, 100 + i, np.zeros(3), np.eye(3), U, V, 10.0 + 2.0 * i, -8.0, 3000.0)
    if displacement is not None:
        k.displacement = displacement
    return k


def test_maps_resolve_the_relocalisation_displacement():
    import nearest_neighbor
    import scene_map
    # NNBasedMap: six finite values; all zero is none
    assert nearest_neighbor.NNBasedMap().displacement is None
    assert nearest_neighbor.NNBasedMap(displacement=np.zeros(6)).displacement is None
    assert np.array_equal(nearest_neighbor.NNBasedMap(displacement=LAMBDA).displacement, LAMBDA)
    for bad in (np.zeros(5), [0, 0, 0, 0, 0, np.inf]):
        with pytest.raises(ValueError):
            nearest_neighbor.NNBasedMap(displacement=bad)
    # Map: off by default; six values; True = the bundle adjuster's value, or else the first keyframe's non-zero one
    m = scene_map.Map("sift", cache_correspondences=False)
    m.keyframe_list = [_kf(0, LAMBDA)]
    assert m.displacement_for_reloc() is None
    m = scene_map.Map("sift", cache_correspondences=False, reloc_displacement=2 * LAMBDA)
    assert np.array_equal(m.displacement_for_reloc(), 2 * LAMBDA)
    m = scene_map.Map("sift", cache_correspondences=False, ba_displacement=3 * LAMBDA, reloc_displacement=True)
    m.keyframe_list = [_kf(0, LAMBDA)]
    assert np.array_equal(m.displacement_for_reloc(), 3 * LAMBDA)
    m = scene_map.Map("sift", cache_correspondences=False, reloc_displacement=True)
    assert m.displacement_for_reloc() is None  # no keyframe yet: looked for again at the next call
    m.keyframe_list = [_kf(0), _kf(1, np.zeros(6)), _kf(2, LAMBDA)]
    assert np.array_equal(m.displacement_for_reloc(), LAMBDA)
    with pytest.raises(ValueError):
        scene_map.Map("sift", reloc_displacement=np.zeros(6))
    # RandomForestMap
    rf = scene_map.RandomForestMap()
    rf.keyframe_list = [_kf(0, LAMBDA)]
    assert rf.displacement_for_reloc() is None
    rf = scene_map.RandomForestMap(reloc_displacement=True)
    rf.keyframe_list = [_kf(0), _kf(1, LAMBDA)]
    assert np.array_equal(rf.displacement_for_reloc(), LAMBDA)
    assert np.array_equal(scene_map.RandomForestMap(reloc_displacement=LAMBDA).displacement_for_reloc(), LAMBDA)
