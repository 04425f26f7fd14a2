"""GPU tests of the joint posterior covariance (ptzba_covariance_joint: BAHandle.covariance_joint,
BAHandle.relative_pose_covariance, LMSolver.covariance_joint and the "joint" entry of the drop-in's `covariance=`).

Reference (tests/cov_joint_ref.py): the sub-matrix of np.linalg.inv(H) at the chosen parameters in the chosen order, H
from cov_ref.normal_matrix (ray_prior_ref.normal_matrix with priors).  Metric over the whole n x n matrix:
max |got_ij - ref_ij| / sqrt(ref_ii ref_jj); rows and columns of a fixed frame or a record-less landmark must be zero
exactly.  Tolerances: test_gpu_covariance.TOL, 1e-7 for fp64 records and 2e-3 for fp32 records.  A mis-signed or
dropped cross block is off by more than 0.7 in this metric (test_cov_joint_cpu.py)."""
import ctypes

import numpy as np
import pytest

from conftest import golden

import cov_joint_ref as jref
from test_gpu_covariance import TOL, _config2_landmarks, _handle

pytestmark = pytest.mark.gpu


def _config1_selection(p):
    """All 9 free frames in a permuted order with the fixed frame 0 among them, all 130 landmarks permuted: one ragged
    pose block, nine ray blocks (the last holds 2 landmarks), one row tile."""
    rng = np.random.default_rng(11)
    frames = list(rng.permutation(np.arange(1, p.n_pose)))
    frames.insert(4, 0)
    landmarks = rng.permutation(p.n_landmark)
    assert len(frames) == 10 and len(landmarks) == 130
    return np.array(frames, np.int32), landmarks.astype(np.int32)


def _config2_selection(p):
    """All 49 free frames in reverse order (five pose blocks over five row tiles: differing first tiles) and
    test_gpu_covariance's 50 landmarks."""
    return np.arange(p.n_pose - 1, 0, -1).astype(np.int32), _config2_landmarks(p)


@pytest.mark.parametrize("precision", [0, 1])
def test_config1_matches_dense_inverse(gpu_available, precision):
    p, C = jref.synthetic_inverse("config1")
    frames, landmarks = _config1_selection(p)
    h = _handle(p, precision)
    si = h.solver_info()
    assert si["n_aug"] == 27 and si["ld"] == 32  # one row tile, the augmented row inside it
    cov, info = h.covariance_joint(frames, landmarks)
    h.close()
    ref = jref.cut(C, jref.param_index(p, frames, landmarks))
    err = jref.joint_err(cov, ref)
    print(f"config1 precision {precision}: joint {err:.3e} over {cov.shape} (tol {TOL[precision]:.0e}); {info}")
    assert cov.shape == (290, 290) and not cov[12:15].any() and not cov[:, 12:15].any()  # frame 0 sits fifth
    assert info["scale"] == 1.0 and info["min_pivot"] > 0 and info["n_free"] == 3 * (p.n_pose - 1) + 2 * p.n_landmark
    assert cov.tobytes() == cov.T.tobytes()
    assert err <= TOL[precision], err


@pytest.mark.parametrize("ordering", [0, 2])
@pytest.mark.parametrize("precision", [0, 1])
def test_config2_matches_dense_inverse(gpu_available, precision, ordering):
    p, C = jref.synthetic_inverse("config2")
    frames, landmarks = _config2_selection(p)
    h = _handle(p, precision, ordering)
    if ordering == 2:
        assert h.solver_info()["ordering"] == "nested"
    cov, info = h.covariance_joint(frames, landmarks)
    h.close()
    ref = jref.cut(C, jref.param_index(p, frames, landmarks))
    err = jref.joint_err(cov, ref)
    nf = 3 * len(frames)
    d = np.sqrt(np.diag(ref))
    rel = np.abs(cov - ref) / np.outer(d, d)
    diag = max(max(rel[3 * q:3 * q + 3, 3 * q:3 * q + 3].max() for q in range(len(frames))),
               max(rel[nf + 2 * q:nf + 2 * q + 2, nf + 2 * q:nf + 2 * q + 2].max() for q in range(len(landmarks))))
    print(f"config2 ordering {ordering} precision {precision}: joint {err:.3e} (diagonal blocks {diag:.3e}, pose-pose "
          f"{rel[:nf, :nf].max():.3e}, pose-ray {rel[:nf, nf:].max():.3e}, ray-ray {rel[nf:, nf:].max():.3e}; tol "
          f"{TOL[precision]:.0e}); {info}")
    assert cov.shape == (247, 247) and cov.tobytes() == cov.T.tobytes()
    assert err <= TOL[precision], err


def test_degenerate_shapes(gpu_available):
    """config 1, fp64: frames only, landmarks only, one frame + one landmark (5 x 5), two frames; a selected landmark
    without records (zero rows and columns); n_fixed = 2 (frames 0 and 1 zero, the rest against the inverse with both
    poses removed)."""
    p, C = jref.synthetic_inverse("config1")
    h = _handle(p)
    for frames, landmarks in (([3, 9, 1], []), ([], [129, 0, 64]), ([7], [33]), ([2, 8], [])):
        cov, _ = h.covariance_joint(frames, landmarks)
        err = jref.joint_err(cov, jref.cut(C, jref.param_index(p, frames, landmarks)))
        print(f"frames {frames} landmarks {landmarks}: {cov.shape} {err:.3e}")
        assert cov.shape == (3 * len(frames) + 2 * len(landmarks),) * 2
        assert err <= 1e-7, (frames, landmarks, err)
    # one more landmark than the records name: it has no records and is selected
    h.set_problem(p.n_pose, p.n_landmark + 1, p.frame, p.landmark, p.xy, p.u, p.v)
    h.set_state(p.init_ptz, np.concatenate([p.init_rays, [[1.0, 2.0]]]))
    frames, landmarks = [4, 6], [5, p.n_landmark, 77]
    cov, info = h.covariance_joint(frames, landmarks)
    ref = jref.cut(C, jref.param_index(p, frames, landmarks, dead=(p.n_landmark,)))
    err = jref.joint_err(cov, ref)
    print(f"record-less landmark: {err:.3e}")
    assert not cov[8:10].any() and not cov[:, 8:10].any() and cov[10:, :8].all()
    assert info["n_free"] == 3 * (p.n_pose - 1) + 2 * p.n_landmark
    assert err <= 1e-7, err
    h.close()
    p2, C2 = jref.synthetic_inverse("config1", n_fixed=2)
    g = _handle(p2, n_fixed=2)
    frames, landmarks = [1, 5, 0, 2], [10, 20]
    cov, info = g.covariance_joint(frames, landmarks)
    g.close()
    err = jref.joint_err(cov, jref.cut(C2, jref.param_index(p2, frames, landmarks, n_fixed=2)))
    print(f"n_fixed 2: {err:.3e}")
    assert not cov[0:3].any() and not cov[6:9].any() and cov[3:6, 9:].all()
    assert info["n_free"] == 3 * (p.n_pose - 2) + 2 * p.n_landmark
    assert err <= 1e-7, err


def test_huber_weights(gpu_available):
    """Huber (config 2, fp64, f_scale 1): the joint matrix matches the sqrt(rho')-weighted reference."""
    import ptzba
    p, C = jref.synthetic_inverse("config2", "huber", 1.0)
    frames, landmarks = _config2_selection(p)
    h = _handle(p, loss=ptzba.LOSS_HUBER, f_scale=1.0)
    cov, _ = h.covariance_joint(frames, landmarks)
    h.close()
    err = jref.joint_err(cov, jref.cut(C, jref.param_index(p, frames, landmarks)))
    _, Clin = jref.synthetic_inverse("config2")
    away = jref.joint_err(cov, jref.cut(Clin, jref.param_index(p, frames, landmarks)))
    print(f"huber: {err:.3e} (against the unweighted reference {away:.3e})")
    assert err <= 1e-7, err
    assert away > 1e-3  # (the weights matter: the comparison can fail)


def test_residual_scale_at_optimum(gpu_available):
    """LMSolver solves config 1 in fp64; covariance_joint(scale="residual") == s^2 inv(H) at the returned state."""
    import ptzba
    import synthetic
    import cov_ref
    from oracle import ptz_oracle as orc
    p = synthetic.make_problem("config1", seed=0)
    h = _handle(p)
    solver = ptzba.LMSolver(h, ftol=1e-10, xtol=1e-12)
    res = solver.run()
    frames, landmarks = _config1_selection(p)
    cov, info = solver.covariance_joint(frames, landmarks, scale="residual")
    ptz, rays = h.get_state()
    h.close()
    assert res.status > 0, res
    r = orc.compute_residual_records(np.concatenate([ptz.reshape(-1), rays.reshape(-1)]), p.n_pose, p.u, p.v,
                                     p.frame.astype(np.int64), p.landmark.astype(np.int64), p.xy)
    n_free = 3 * (p.n_pose - 1) + 2 * p.n_landmark
    s2 = float(np.sum(r * r)) / (len(r) - n_free)
    C = np.linalg.inv(cov_ref.normal_matrix(p, ptz, rays))
    err = jref.joint_err(cov, s2 * jref.cut(C, jref.param_index(p, frames, landmarks)))
    print(f"optimum: s2 {s2:.6e} (gpu {info['scale']:.6e}); joint {err:.3e}")
    assert abs(info["scale"] - s2) <= 1e-9 * s2 and info["n_free"] == n_free
    assert err <= 1e-7, err


def test_pose_and_ray_priors(gpu_available):
    """config 1, fp64, prior_ref.factor_set pose priors and ray_prior_ref.standard_set ray priors both set: the joint
    matrix matches the inverse of ray_prior_ref.normal_matrix."""
    import prior_ref
    import ray_prior_ref as rref
    from test_gpu_ray_priors import _handle as prior_handle
    p = rref.problem("config1")
    factors = prior_ref.factor_set(p)
    rpriors = rref.standard_set(p)
    C = np.linalg.inv(rref.normal_matrix(p, p.init_ptz, p.init_rays, rpriors, factors))
    frames, landmarks = _config1_selection(p)
    h = prior_handle("config1", rpriors=rpriors, factors=factors)
    cov, _ = h.covariance_joint(frames, landmarks)
    h.close()
    idx = jref.param_index(p, frames, landmarks)
    err = jref.joint_err(cov, jref.cut(C, idx))
    _, Cfree = jref.synthetic_inverse("config1")
    away = jref.joint_err(cov, jref.cut(Cfree, idx))
    print(f"priors: {err:.3e} (against the prior-free reference {away:.3e})")
    assert err <= 1e-7, err
    assert away > 1e-3


def test_consistency_with_covariance(gpu_available):
    """config 2, fp32 records, nested order.  The joint matrix's diagonal blocks are covariance()'s blocks bit for bit
    (the bound was 1e-12 in the metric: the same factor and the same Z; they turned out equal); it is
    symmetric bit for bit; two calls return the same bytes; permuting the selection permutes the matrix (1e-12);
    covariance() before and after a joint call returns the same bytes."""
    p, _ = jref.synthetic_inverse("config2")
    frames, landmarks = _config2_selection(p)
    h = _handle(p, precision=1, ordering=2)
    pose0, ray0, _ = h.covariance(landmarks)
    cov, _ = h.covariance_joint(frames, landmarks)
    cov2, _ = h.covariance_joint(frames, landmarks)
    pose1, ray1, _ = h.covariance(landmarks)
    assert pose0.tobytes() == pose1.tobytes() and ray0.tobytes() == ray1.tobytes()
    assert cov.tobytes() == cov2.tobytes()
    assert cov.tobytes() == cov.T.tobytes()
    nf = 3 * len(frames)
    worst, equal = 0.0, True
    for q, f in enumerate(frames):
        blk = cov[3 * q:3 * q + 3, 3 * q:3 * q + 3]
        d = np.sqrt(np.diag(pose0[f]))
        worst = max(worst, float(np.max(np.abs(blk - pose0[f]) / np.outer(d, d))))
        equal = equal and blk.tobytes() == pose0[f].tobytes()
    for q in range(len(landmarks)):
        blk = cov[nf + 2 * q:nf + 2 * q + 2, nf + 2 * q:nf + 2 * q + 2]
        d = np.sqrt(np.diag(ray0[q]))
        worst = max(worst, float(np.max(np.abs(blk - ray0[q]) / np.outer(d, d))))
        equal = equal and blk.tobytes() == ray0[q].tobytes()
    print(f"diagonal blocks against covariance(): {worst:.3e} (bit-equal: {equal})")
    assert worst <= 1e-12, worst
    # measured bit-equal: a column of Z does not depend on the block it is packed into, and both kernels sum a block's
    # tiles in the same order with the same matrix-core products, so equality is what is asserted
    assert equal
    # a permuted selection: other blocks, other first tiles, the same numbers
    rng = np.random.default_rng(5)
    pf, pl = rng.permutation(len(frames)), rng.permutation(len(landmarks))
    covp, _ = h.covariance_joint(frames[pf], landmarks[pl])
    h.close()
    perm = np.concatenate([(3 * pf[:, None] + np.arange(3)).reshape(-1), nf + (2 * pl[:, None] + np.arange(2)).reshape(-1)])
    want = cov[np.ix_(perm, perm)]
    d = np.sqrt(np.diag(want))
    e = float(np.max(np.abs(covp - want) / np.outer(d, d)))
    print(f"permuted selection: {e:.3e}")
    assert e <= 1e-12, e


def test_relative_pose_covariance(gpu_available):
    """config 2: Cov(x_a - x_b) = R C R^T, R = [I -I], of the dense inverse, for an adjacent pair and for the pair
    furthest apart, relative to the reference's diagonal; against frame 0 it is S_aa."""
    p, C = jref.synthetic_inverse("config2")
    R = np.concatenate([np.eye(3), -np.eye(3)], 1)
    for precision in (0, 1):
        h = _handle(p, precision)
        for a, b in ((24, 25), (1, p.n_pose - 1)):
            got = h.relative_pose_covariance(a, b)
            ref = R @ jref.cut(C, jref.param_index(p, [a, b], [])) @ R.T
            d = np.sqrt(np.diag(ref))
            e = float(np.max(np.abs(got - ref) / np.outer(d, d)))
            print(f"precision {precision} frames ({a}, {b}): {e:.3e} (sigma {d})")
            assert got.shape == (3, 3) and e <= TOL[precision], (a, b, e)
        got = h.relative_pose_covariance(7, 0)
        joint, _ = h.covariance_joint([7])
        pose, _, _ = h.covariance(None)
        h.close()
        assert np.array_equal(got, joint)
        assert jref.joint_err(got, jref.cut(C, jref.param_index(p, [7], []))) <= TOL[precision]
        assert jref.joint_err(got, pose[7]) <= 1e-12


def test_no_side_effect_on_a_following_solve(gpu_available):
    """config 2, fp32 + Huber: a device-loop solve from x0, and one with a joint call between set_state and the solve,
    give the same state, njev and status bit for bit."""
    import ptzba
    import synthetic
    p = synthetic.make_problem("config2", seed=0)
    frames, landmarks = _config2_selection(p)
    out = []
    for with_cov in (False, True):
        h = _handle(p, precision=1, loss=ptzba.LOSS_HUBER)
        if with_cov:
            h.covariance_joint(frames, landmarks, scale="residual")
        res = ptzba.LMSolver(h, ftol=1e-4, xtol=1e-8).run()
        ptz, rays = h.get_state()
        h.close()
        out.append((ptz.tobytes(), rays.tobytes(), res.njev, res.status, res.cost))
    assert out[0][2] > 1
    assert out[0] == out[1], (out[0][2:], out[1][2:])


def test_errors_leave_the_handle_usable(gpu_available):
    """Every refusal one process can reach names its condition, writes nothing into the output array and leaves the
    handle computing the right matrix afterwards."""
    import ptzba
    p1, C1 = jref.synthetic_inverse("config1")
    p2, C2 = jref.synthetic_inverse("config2")

    def refused(h, p, C, match, frames, landmarks, **kw):
        n = 3 * len(frames) + 2 * len(landmarks)
        out = np.full((n, n), 7.25)
        with pytest.raises(ptzba.PtzbaError, match=match):
            h.covariance_joint(frames, landmarks, _out=out, **kw)
        assert np.all(out == 7.25)
        if C is not None:
            good_f, good_l = [2, 1], [3]
            cov, _ = h.covariance_joint(good_f, good_l)
            assert jref.joint_err(cov, jref.cut(C, jref.param_index(p, good_f, good_l))) <= 1e-7

    h = _handle(p1)
    refused(h, p1, C1, "named twice", [1, 2, 1], [])
    refused(h, p1, C1, "named twice", [1], [5, 6, 5])
    refused(h, p1, C1, "out of range", [p1.n_pose], [])
    refused(h, p1, C1, "out of range", [-1], [])
    refused(h, p1, C1, "out of range", [1], [p1.n_landmark])
    refused(h, p1, C1, "columns", [], [])
    refused(h, p1, C1, "struct_size", [1], [], _struct_size=ctypes.sizeof(ptzba.ptzba_cov_opts) + 8)
    refused(h, p1, C1, "bad options", [1], [], scale=-1.0)
    # one free frame without records: S is singular, the factorisation reports it, no numbers come back
    keep = p1.frame != 5
    h.set_problem(p1.n_pose, p1.n_landmark, p1.frame[keep], p1.landmark[keep], p1.xy[keep], p1.u, p1.v)
    h.set_state(p1.init_ptz, p1.init_rays)
    refused(h, p1, None, "not positive definite", [1, 2], [3])
    h.set_problem(p1.n_pose, p1.n_landmark, p1.frame, p1.landmark, p1.xy, p1.u, p1.v)
    h.set_state(p1.init_ptz, p1.init_rays)
    cov, _ = h.covariance_joint([2, 1], [3])
    assert jref.joint_err(cov, jref.cut(C1, jref.param_index(p1, [2, 1], [3]))) <= 1e-7
    h.close()
    # 2,049 columns: one frame and 1,023 distinct landmarks (config 2 has 1,609); 2,048 pass the check
    g = _handle(p2)
    assert p2.n_landmark >= 1023
    refused(g, p2, C2, "columns", [1], np.arange(1023))
    g.close()
    e = ptzba.BAHandle(0)
    with pytest.raises(ptzba.PtzbaError, match="no problem set"):
        e.covariance_joint([1])
    e.close()


def test_column_cap_is_reachable(gpu_available):
    """PTZBA_COV_JOINT_MAX_COLS columns exactly (config 2: 1,024 landmarks, 64 full ray blocks) are computed; checked
    on a spread of entries against the dense inverse."""
    p, C = jref.synthetic_inverse("config2")
    landmarks = np.arange(p.n_landmark - 1024, p.n_landmark).astype(np.int32)
    h = _handle(p)
    cov, _ = h.covariance_joint([], landmarks)
    h.close()
    assert cov.shape == (2048, 2048) and cov.tobytes() == cov.T.tobytes()
    err = jref.joint_err(cov, jref.cut(C, jref.param_index(p, [], landmarks)))
    print(f"2048 columns: {err:.3e}")
    assert err <= 1e-7, err


def test_dropin_keyword(gpu_available):
    """bundle_adjustment() on the ba_6x120 golden: covariance={"joint": (frames, landmarks)} returns the blocks of
    covariance=True plus the joint matrix of BAHandle.covariance_joint at that solution (1e-7 in the metric: the
    drop-in's handle holds the same records in the match graph's order); covariance=True returns what it returns
    today, without the key."""
    import random
    import image_process
    import bundle_adjustment as ba
    import ptzba
    from test_gpu_ba import _install_fixture_frontend, _problem_from_golden
    d = golden("ba_6x120.npz")
    n = int(d["n_pose"])
    sel_f, sel_l = [3, 0, 1], [5, 17, 2]
    runs = []
    for cov_arg in (True, {"joint": (sel_f, sel_l)}):
        saved, _ = _install_fixture_frontend(d)
        try:
            random.seed(int(d["seed"]))
            out = ba.bundle_adjustment(list(range(n)), list(range(100, 100 + n)), "sift", d["init_ptz"].copy(),
                                       np.array([0.0, -10.0, 5.0]), np.eye(3), float(d["u"]), float(d["v"]), "",
                                       ftol=1e-14, xtol=1e-14, max_iter=200, covariance=cov_arg)
        finally:
            image_process.detect_compute_sift, image_process.match_sift_features = saved
        assert len(out) == 3
        runs.append(out)
    plain, joint = runs[0][2], runs[1][2]
    assert sorted(plain) == ["info", "pose_cov", "ray_cov"] and "joint" not in plain["info"]
    assert sorted(joint) == ["info", "joint", "pose_cov", "ray_cov"] and joint["info"]["joint"] is joint["joint"]
    assert plain["pose_cov"].tobytes() == joint["pose_cov"].tobytes()
    assert plain["ray_cov"].tobytes() == joint["ray_cov"].tobytes()
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    landmarks, keyframes = runs[1][:2]
    ptz = np.array([[k.pan, k.tilt, k.f] for k in keyframes])
    n_pose, n_lm, frame, landmark, xy, u, v = _problem_from_golden(d)
    h = ptzba.BAHandle(0)
    h.set_problem(n_pose, n_lm, frame, landmark, xy, u, v)
    h.set_state(ptz, landmarks)
    ref, _ = h.covariance_joint(sel_f, sel_l)
    h.close()
    C = joint["joint"]
    assert C.shape == (15, 15) and not C[3:6].any() and C[:3, 6:].all()
    err = jref.joint_err(C, ref)
    print(f"drop-in joint vs BAHandle.covariance_joint: {err:.3e}")
    assert err <= 1e-7, err
    # its diagonal blocks are the blocks the same call returns
    for q, f in enumerate(sel_f):
        assert jref.joint_err(C[3 * q:3 * q + 3, 3 * q:3 * q + 3], joint["pose_cov"][f]) <= 1e-12
    for q, l in enumerate(sel_l):
        assert jref.joint_err(C[9 + 2 * q:11 + 2 * q, 9 + 2 * q:11 + 2 * q], joint["ray_cov"][l]) <= 1e-12
