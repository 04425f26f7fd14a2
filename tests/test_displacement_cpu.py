"""CPU tests of the displaced camera model's reference (tests/disp_ref.py): its projection and Jacobian against the
oracle's PTZCamera projection with a displacement, its reduction to the oracle's displacement-free Jacobian, and what
the displacement is worth on config 1 -- the displaced Gauss-Newton solve recovers the ground truth, the
displacement-free model on the same observations does not.  Also the Python-side plumbing that needs no GPU."""
import numpy as np
import pytest

import disp_ref
from disp_ref import LAMBDA, ZERO


def _sample(n=400, seed=5):
    """Per-record poses and rays well inside the field of view (q2 ~ 1), around a broadcast camera's range."""
    rng = np.random.default_rng(seed)
    ptz = np.stack([rng.uniform(-40, 40, n), rng.uniform(-15, -2, n), rng.uniform(1500, 5000, n)], 1)
    rays = np.stack([ptz[:, 0] + rng.uniform(-8, 8, n), ptz[:, 1] + rng.uniform(-5, 5, n)], 1)
    return ptz, rays


def _oracle_project(u, v, ptz, rays, lam):
    from oracle import ptz_oracle as orc
    return np.concatenate([orc.project_rays(u, v, f, pan, tilt, ray[None], lam)
                           for (pan, tilt, f), ray in zip(ptz, rays)])


def test_projection_equals_the_oracle_with_displacement():
    """disp_ref.project == oracle.project_rays(..., displacement) to 1e-9 px where q2 > 0, and moves the points."""
    u, v = 640.0, 360.0
    ptz, rays = _sample()
    xy, q2 = disp_ref.project(u, v, ptz, rays, LAMBDA)
    assert q2.min() > 0
    ref = _oracle_project(u, v, ptz, rays, LAMBDA)
    err = np.abs(xy - ref).max()
    moved = np.abs(xy - disp_ref.project(u, v, ptz, rays, ZERO)[0]).max()
    print(f"projection vs oracle: {err:.3e} px; the displacement moves the points by up to {moved:.1f} px")
    assert err <= 1e-9
    assert moved > 10.0


def test_jacobian_equals_central_differences_of_the_oracle():
    """The analytic Jacobian == central differences of oracle.project_rays with the displacement, 1e-8 relative to the
    column's largest entry (steps 1e-4 deg / 1e-2 px: truncation ~1e-11 relative, rounding ~1e-10)."""
    u, v = 640.0, 360.0
    ptz, rays = _sample(200)
    J = disp_ref.record_jacobian(u, v, ptz, rays, LAMBDA)
    x = np.concatenate([ptz, rays], 1)
    worst = 0.0
    for c, h in enumerate([1e-4, 1e-4, 1e-2, 1e-4, 1e-4]):
        xp, xm = x.copy(), x.copy()
        xp[:, c] += h
        xm[:, c] -= h
        fd = (_oracle_project(u, v, xp[:, :3], xp[:, 3:], LAMBDA) -
              _oracle_project(u, v, xm[:, :3], xm[:, 3:], LAMBDA)) / (2 * h)
        err = np.abs(J[:, :, c] - fd).max() / np.abs(fd).max()
        worst = max(worst, err)
    # the f column differs from the displacement-free one (the part a build that only moved the projection would miss)
    J0 = disp_ref.record_jacobian(u, v, ptz, rays, ZERO)
    print(f"Jacobian vs central differences: {worst:.3e}; f column moved by "
          f"{np.abs(J[:, :, 2] - J0[:, :, 2]).max() / np.abs(J0[:, :, 2]).max():.3e}")
    assert worst <= 1e-8, worst
    assert np.abs(J[:, :, 2] - J0[:, :, 2]).max() > 1e-3 * np.abs(J0[:, :, 2]).max()


def test_zero_displacement_is_the_oracle_jacobian_exactly():
    from oracle import ptz_oracle as orc
    ptz, rays = _sample()
    J = disp_ref.record_jacobian(640.0, 360.0, ptz, rays, ZERO)
    np.testing.assert_array_equal(J, orc.record_jacobian(640.0, 360.0, ptz, rays))
    p = disp_ref.prior_ref.problem("config1")
    r = orc.compute_residual_records(np.concatenate([p.init_ptz.reshape(-1), p.init_rays.reshape(-1)]), p.n_pose, p.u,
                                     p.v, p.frame.astype(np.int64), p.landmark.astype(np.int64), p.xy)
    np.testing.assert_allclose(disp_ref.residual(p, p.init_ptz, p.init_rays, ZERO), r, rtol=0, atol=1e-9)


def test_displaced_problem_shape():
    """The displaced problems keep the records and the noise, move the observations by hundreds of pixels and keep
    every record in front of the camera."""
    for cfg, n_pose, n_rec in (("config1", 10, 2550), ("config2", 50, 294064)):
        p, shift, q2 = disp_ref.displaced_problem(cfg)
        p0 = disp_ref.prior_ref.problem(cfg)
        print(f"{cfg}: observations move by up to {shift:.1f} px; smallest q2 at the initial state {q2:.3f}")
        assert (p.n_pose, len(p.frame)) == (n_pose, n_rec)
        assert shift > 100.0 and q2 > 1.0
        # the noise is kept: residuals at the ground truth are the undisplaced problem's
        np.testing.assert_allclose(disp_ref.residual(p, p.gt_ptz, p.gt_rays, LAMBDA),
                                   disp_ref.residual(p0, p0.gt_ptz, p0.gt_rays, ZERO), rtol=0, atol=1e-9)
        # the initial rays are the oracle's back-projection of the source records (the reference's back_project_to_ray
        # subtracts d from the z = 1 point, an approximate inverse once d is non-zero: no round trip is asserted)
        from oracle import ptz_oracle as orc
        rec = disp_ref.source_records(p)
        l = p.n_landmark // 2
        pan, tilt, f = p.init_ptz[p.frame[rec[l]]]
        back = orc.back_project_to_rays(p.u, p.v, f, pan, tilt, p.xy[rec[l]][None], LAMBDA)[0]
        np.testing.assert_array_equal(p.init_rays[l], back)
        assert p.landmark[rec[l]] == l and rec[l] % 2 == 0 and not np.any(p.landmark[rec[l] + 2::2] == l)


def test_displaced_solve_recovers_the_ground_truth_and_the_plain_model_does_not():
    """Config 1: Gauss-Newton under the displaced model ends within 0.02 deg / 5 px of the ground truth; the
    displacement-free model on the same observations misses by more than 0.5 deg."""
    p, _, _ = disp_ref.displaced_problem("config1")
    ptz, rays, c, it = disp_ref.solve(p, p.init_ptz, p.init_rays, LAMBDA)
    ea, ef = disp_ref.pose_error(ptz, p.gt_ptz)
    ptz0, rays0, c0, it0 = disp_ref.solve(p, p.init_ptz, p.init_rays, ZERO)
    ea0, ef0 = disp_ref.pose_error(ptz0, p.gt_ptz)
    dx1 = disp_ref.gn_step(p, p.init_ptz, p.init_rays, LAMBDA)[0]
    dx0 = disp_ref.gn_step(p, p.init_ptz, p.init_rays, ZERO)[0]
    print(f"displaced model: {ea:.4f} deg / {ef:.2f} px from the ground truth, cost {c:.1f}, {it} iterations; "
          f"displacement-free model: {ea0:.3f} deg / {ef0:.1f} px, cost {c0:.1f}; first step differs by "
          f"{np.abs(dx1 - dx0).max() / np.abs(dx1).max():.3f} of its largest entry")
    assert ea <= 0.02 and ef <= 5.0, (ea, ef)
    assert ea0 > 0.5, ea0


def test_python_plumbing_without_a_gpu():
    """The two entry points are bound and exported; solve() and the drop-in validate a displacement before any GPU
    work."""
    import ptzba
    import bundle_adjustment as ba
    for s in ("ptzba_set_displacement", "ptzba_displacement_info"):
        assert s in ptzba.EXPORTED_SYMBOLS and hasattr(ptzba.lib(), s)
    for name in ("set_displacement", "clear_displacement", "displacement_info"):
        assert callable(getattr(ptzba.BAHandle, name))
    with pytest.raises(ValueError, match="displacement"):
        ptzba.solve(2, 1, [0, 1], [0, 0], np.zeros((2, 2)), 0.0, 0.0, np.zeros((2, 3)), np.zeros((1, 2)),
                    displacement=[0, 0, np.nan, 0, 0, 0])
    with pytest.raises(ValueError, match="displacement"):
        ba.bundle_adjustment([None], [0], "sift", np.zeros((1, 3)), np.zeros(3), np.eye(3), 0.0, 0.0, "",
                             displacement=[1.0, 2.0])
