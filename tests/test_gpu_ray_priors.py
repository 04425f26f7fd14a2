"""GPU tests of the Gaussian ray priors (ptzba_set_ray_priors: BAHandle.set_ray_priors, ptzba.solve's and the
drop-in's `ray_priors=`).

Reference (tests/ray_prior_ref.py, pinned to scipy by test_ray_priors_cpu.py): the oracle's residual and analytic
Jacobian plus the priors' 2 x 2 blocks on the landmark part.  The standard set S (ray_prior_ref.standard): a prior on
every third observed landmark, sigma 0.02 x 0.06 deg at a random angle, means up to 3 x 0.02 deg off the initial ray,
and a second prior on the first five of those landmarks (listed after all the others).  Tolerances are the project's
own: the Gauss-Newton step's (test_gpu_ba) and the covariance blocks' (test_gpu_covariance)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

import prior_ref
import ray_prior_ref as rref
from test_gpu_covariance import TOL

pytestmark = pytest.mark.gpu

STEP_TOL = {0: 1e-7, 1: 2e-3}  # test_gpu_ba.test_single_gauss_newton_step_is_exact's own


def _handle(cfg, precision=0, ordering=0, loss=0, f_scale=1.0, rpriors=None, factors=None, state=None):
    import ptzba
    p = rref.problem(cfg)
    win = ptzba.prior_window(p.n_pose, p.frame, p.landmark, factors) if factors else None
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=precision, ordering=ordering,
                  loss=loss, f_scale=f_scale, frame_win_hi=win)
    if factors:
        h.set_pose_priors(factors)
    if rpriors:
        h.set_ray_priors(rpriors)
    ptz, rays = state if state is not None else (p.init_ptz, p.init_rays)
    h.set_state(ptz, rays)
    return h


def _gpu_step(h, p, linearize=True):
    """One undamped step from the initial state, as [free poses | rays]; the trial is accepted."""
    if linearize:
        h.linearize()
    h.build_reduced(0.0)
    h.solve_reduced()
    s = h.read_scalars()
    assert s[5] == 0
    h.accept(True)
    ptz1, rays1 = h.get_state()
    return np.concatenate([(ptz1 - p.init_ptz)[1:].reshape(-1), (rays1 - p.init_rays).reshape(-1)]), s


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref_steps(cfg):
    """(dx with S, dx without) of one undamped Gauss-Newton step at the initial state."""
    p = rref.problem(cfg)
    dx1 = rref.gn_step(p, p.init_ptz, p.init_rays, list(rref.standard(cfg)))[0]
    dx0 = rref.gn_step(p, p.init_ptz, p.init_rays, [])[0]
    return _frozen(dx1), _frozen(dx0)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cfg,ordering", [("config1", 0), ("config2", 0), ("config2", 2)])
@pytest.mark.parametrize("precision", [0, 1])
def test_gauss_newton_step_with_ray_priors_is_exact(gpu_available, precision, cfg, ordering):
    """One undamped step == the dense solve of (H + P_ray) dx = -(g + P_ray e), to
    test_single_gauss_newton_step_is_exact's tolerance; the reference step without the priors is at least 10
    tolerances away, so a build that dropped them from V or g could not pass."""
    p = rref.problem(cfg)
    dx, dx_plain = _ref_steps(cfg)
    tol = STEP_TOL[precision]
    moved = np.abs(dx - dx_plain).max() / np.abs(dx).max()
    assert moved >= 10 * tol, moved
    h = _handle(cfg, precision, ordering, rpriors=list(rref.standard(cfg)))
    if ordering == 2:
        assert h.solver_info()["ordering"] == "nested"
    dx_gpu, _ = _gpu_step(h, p)
    h.close()
    err = np.abs(dx_gpu - dx).max() / np.abs(dx).max()
    print(f"{cfg} ordering {ordering} precision {precision}: step error {err:.3e} (tol {tol:.0e}); ray priors move the "
          f"step by {moved:.3e}")
    assert err < tol, err


# ------------------------------------------------------------------------------------------------ 2
@functools.lru_cache(maxsize=None)
def _ref_stiff():
    p = rref.problem("config2")
    assert len(rref.observed(p)) == p.n_landmark
    dx1 = rref.gn_step_schur(p, p.init_ptz, p.init_rays, rref.stiff_set(p))[0]
    dx0 = rref.gn_step(p, p.init_ptz, p.init_rays, [])[0]
    return _frozen(dx1), _frozen(dx0)


@pytest.mark.parametrize("precision", [0, 1])
def test_stiff_priors(gpu_available, precision):
    """Every second landmark of config 2 pinned at its initial ray with Lambda = 1e12 I, the rest free: V^-1 spans 17
    orders of magnitude inside one K2 batch.  The step equals the dense reference with the same Lambda (block-wise
    Schur elimination in fp64, ray_prior_ref.gn_step_schur) to the same tolerance.  The pinned rays' own steps
    (~1e-6 deg, V^-1 times a gradient of ~1e6) are printed beside the reference's."""
    p = rref.problem("config2")
    dx, dx_plain = _ref_stiff()
    tol = STEP_TOL[precision]
    moved = np.abs(dx - dx_plain).max() / np.abs(dx).max()
    assert moved >= 10 * tol, moved
    S = rref.stiff_set(p)
    h = _handle("config2", precision, rpriors=S)
    dx_gpu, _ = _gpu_step(h, p)
    h.close()
    err = np.abs(dx_gpu - dx).max() / np.abs(dx).max()
    k = 3 * (p.n_pose - 1)
    ids = [s[0] for s in S]
    pinned, pinned_ref = np.abs(dx_gpu[k:].reshape(-1, 2)[ids]).max(), np.abs(dx[k:].reshape(-1, 2)[ids]).max()
    print(f"stiff priors precision {precision}: step error {err:.3e} (tol {tol:.0e}); moved {moved:.3e}; largest "
          f"pinned-ray step {pinned:.3e} deg (reference {pinned_ref:.3e})")
    assert err < tol, err


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("cfg", ["config1", "config2"])
def test_ray_prior_cost(gpu_available, cfg):
    """ray_prior_info: the counts, and the cost == numpy's 1/2 sum e^T Lambda e (1e-12 relative), bitwise repeatable;
    the cost linearize() reports with the priors minus the one after clearing them is that cost (1e-9 of the total);
    the trial cost of a step includes the prior at the trial state."""
    p = rref.problem(cfg)
    S = list(rref.standard(cfg))
    # a state off the means' centre, so that e is not the draw itself
    rays = p.init_rays + 0.01
    h = _handle(cfg, rpriors=S, state=(p.init_ptz, rays))
    n, n_lm, rows, c = h.ray_prior_info()
    ref = rref.ray_prior_cost(S, rays)
    assert (n, n_lm, rows) == (len(S), len(S) - 5, 2 * len(S))
    print(f"{cfg}: ray prior cost {c!r} vs {ref!r}")
    assert ref > 0 and abs(c - ref) <= 1e-12 * ref
    assert h.ray_prior_info() == (n, n_lm, rows, c)
    h.linearize()
    with_p = h.read_scalars()[0]
    h.linearize()
    assert h.read_scalars()[0] == with_p
    h.step(1e-3)
    s = h.read_scalars()
    h.accept(True)
    ptz1, rays1 = h.get_state()
    assert abs(s[1] - rref.cost(p, ptz1, rays1, S)) <= 1e-9 * s[1]  # the trial cost includes the prior
    h.set_state(p.init_ptz, rays)
    h.clear_ray_priors()
    assert h.ray_prior_info() == (0, 0, 0, 0.0)
    h.linearize()
    without = h.read_scalars()[0]
    h.close()
    assert abs((with_p - without) - ref) <= 1e-9 * with_p, (with_p, without, ref)
    assert abs(without - rref.cost(p, p.init_ptz, rays, [])) <= 1e-9 * without


# ------------------------------------------------------------------------------------------------ 4
@functools.lru_cache(maxsize=None)
def _optimum_config1():
    p = rref.problem("config1")
    ptz, rays, c = rref.solve(p, p.init_ptz, p.init_rays, list(rref.standard("config1")))
    return _frozen(ptz), _frozen(rays), c


def test_converged_solve_device_and_host_loops(gpu_available):
    """Config 1, fp64, linear, S: the device loop and the host loop take identical iterates (the assertions of
    test_gpu_priors' same test) and both stop at ray_prior_ref's optimum (1e-6 deg / 1e-4 px); the reported costs
    include the prior."""
    import ptzba
    p = rref.problem("config1")
    S = list(rref.standard("config1"))
    ptz_ref, rays_ref, c_ref = _optimum_config1()
    _, rays_plain, _ = rref.solve(p, p.init_ptz, p.init_rays, [])
    assert np.abs(rays_plain - rays_ref).max() >= 10 * 1e-6  # the priors move the optimum
    out = []
    for device_loop in (False, True):
        h = _handle("config1", rpriors=S)
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
        assert abs(res.initial_cost - rref.cost(p, p.init_ptz, p.init_rays, S)) <= 1e-9 * res.initial_cost


def test_one_shot_solves_agree(gpu_available):
    """ptzba_solve and ptzba_solve_resident (the device-driven loop run in C) with S end at ray_prior_ref's optimum
    too (the same 1e-6 deg / 1e-4 px gate), with the prior in the reported cost."""
    import ptzba
    p = rref.problem("config1")
    S = list(rref.standard("config1"))
    ptz0, rays0, c_ref = _optimum_config1()
    h = _handle("config1", rpriors=S)
    out = h.solve(p.init_ptz, p.init_rays, ftol=1e-14, xtol=1e-14, max_iter=100)
    ptz1, rays1 = h.get_state()
    h.set_state(p.init_ptz, p.init_rays)
    h.save_state()
    res = h.solve_resident(restore=True, ftol=1e-14, xtol=1e-14, max_iter=100)
    ptz2, rays2 = h.get_state()
    assert h.ray_prior_info()[0] == len(S)  # the priors persist over set_state / save_state / restore_state
    h.close()
    print(out[2], res)
    for r, ptz, rays in ((out[2], ptz1, rays1), (res, ptz2, rays2)):
        np.testing.assert_allclose(ptz[:, :2], ptz0[:, :2], rtol=0, atol=1e-6)
        np.testing.assert_allclose(ptz[:, 2], ptz0[:, 2], rtol=0, atol=1e-4)
        np.testing.assert_allclose(rays, rays0, rtol=0, atol=1e-6)
        assert abs(r.cost - c_ref) <= 1e-9 * c_ref


# ------------------------------------------------------------------------------------------------ 5
def test_converged_solve_config2_fp32_huber(gpu_available):
    """Config 2, fp32, Huber, through ptzba.solve(ray_priors=S): the solve stops at ray_prior_ref's stationary point of
    the Huber objective with S (pose RMSE <= 1e-4, the project's gate).  That point is recorded
    (tests/golden/ray_priors_config2_huber.npz) and its stationarity re-checked here; it is not the optimum without
    priors (tests/golden/config2_optimum.npz).

    The solve runs plain IRLS (huber_curvature=1, the weights the reference's normal matrix uses) until no cost
    decrease is resolvable.  With the priors' means up to 3 px off, a few hundred records sit on Huber's linear branch
    and the iteration's tail is linear; measured on an MI355X: IRLS ends 8.2e-8 / 4.6e-8 deg, 2.2e-5 px from the
    recorded point (status 5), the default curvature heuristic (0.1 after the switch) takes the same iterates in fp32
    and fp64 for 19 iterations, then its cost decreases (3e-5 of 1.9e5) fall below what fp32 sums resolve and it stops
    on xtol 1.9e-6 / 2.3e-7 deg, 3.0e-4 px short, where fp64 goes on to 3.7e-6 px; started at the recorded point, fp32
    stays within 2e-7 px of it."""
    import ptzba
    import synthetic
    p = rref.problem("config2")
    S = list(rref.standard("config2"))
    xt = golden("config2_optimum.npz")["x_tight_huber"]
    ptz_plain = np.concatenate([p.init_ptz[0], xt[:3 * (p.n_pose - 1)]]).reshape(-1, 3)
    golden(rref.CONFIG2_HUBER)
    ptz_ref, _, c_ref = rref.config2_huber_point(os.path.join(GOLDEN, rref.CONFIG2_HUBER))
    assert np.any(synthetic.pose_rmse(ptz_ref, ptz_plain) > 1e-3)
    for keep in (False, True):  # the private-handle path and the kept-handle path
        ptz, rays, res = ptzba.solve(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, p.init_ptz,
                                     p.init_rays, precision=ptzba.FP32, loss=ptzba.LOSS_HUBER, f_scale=1.0, ftol=1e-12,
                                     xtol=1e-12, max_iter=100, huber_curvature=1.0, ray_priors=S, keep_handle=keep)
        rmse = synthetic.pose_rmse(ptz, ptz_ref)
        print(f"config2 fp32 huber with ray priors (keep_handle={keep}): {res}; pose RMSE {rmse}; cost {res.cost!r} vs "
              f"{c_ref!r}")
        assert np.all(rmse <= 1e-4), rmse
        assert abs(res.cost - c_ref) <= 1e-5 * c_ref
    ptzba.release_solve_handles()


# ------------------------------------------------------------------------------------------------ 6
@functools.lru_cache(maxsize=None)
def _ref_cov(cfg):
    import cov_ref
    p = rref.problem(cfg)
    H = rref.normal_matrix(p, p.init_ptz, p.init_rays, list(rref.standard(cfg)))
    pose, ray = cov_ref._cut(np.linalg.inv(H), p.n_pose, p.n_landmark, 1)
    return _frozen(pose), _frozen(ray)


@pytest.mark.parametrize("cfg,ordering,precision", [("config1", 0, 0), ("config1", 0, 1), ("config2", 2, 0)])
def test_covariance_blocks_match_inverse_with_ray_priors(gpu_available, cfg, ordering, precision):
    """covariance() == the blocks of inv(H + P_ray) (test_gpu_covariance's metric and TOL), and not those of inv(H)."""
    import cov_ref
    p = rref.problem(cfg)
    pose_ref, ray_ref = _ref_cov(cfg)
    plain_pose, plain_ray = cov_ref.synthetic_reference(cfg)[1:]
    assert cov_ref.block_err(ray_ref, plain_ray) >= 10 * TOL[precision]  # the priors show in the reference
    h = _handle(cfg, precision, ordering, rpriors=list(rref.standard(cfg)))
    idx = np.arange(p.n_landmark) if cfg == "config1" else np.arange(0, p.n_landmark, 7)
    pose, ray, info = h.covariance(idx)
    h.close()
    ep, er = cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref[idx])
    print(f"{cfg} ordering {ordering} precision {precision}: pose {ep:.3e} ray {er:.3e} (tol {TOL[precision]:.0e}); "
          f"the priors change the ray blocks by {cov_ref.block_err(ray_ref, plain_ray):.3e}")
    assert ep <= TOL[precision] and er <= TOL[precision], (ep, er)


def test_residual_scale_counts_the_ray_priors(gpu_available):
    """covariance(scale="residual") at the config 1 optimum with S: s^2 = (sum r^2 + sum e^T Lambda e) / (2 R + 2 n_prior
    - n_free), every ray prior two rows."""
    import ptzba
    p = rref.problem("config1")
    S = list(rref.standard("config1"))
    h = _handle("config1", rpriors=S)
    res = ptzba.LMSolver(h, ftol=1e-12, xtol=1e-12, max_iter=100).run()
    _, _, info = h.covariance(None, scale="residual")
    ptz, rays = h.get_state()
    h.close()
    assert res.status > 0, res
    n_free = 3 * (p.n_pose - 1) + 2 * p.n_landmark
    prior2 = 2.0 * rref.ray_prior_cost(S, rays)
    s2 = 2.0 * rref.cost(p, ptz, rays, S) / (2 * len(p.frame) + 2 * len(S) - n_free)
    s2_without_rows = 2.0 * rref.cost(p, ptz, rays, S) / (2 * len(p.frame) - n_free)
    print(f"residual scale {info['scale']!r} vs {s2!r}; prior share of the numerator {prior2:.6e}")
    assert abs(info["scale"] - s2) <= 1e-9 * s2, (info, s2)
    assert abs(s2_without_rows - s2) > 1e-6 * s2 and prior2 > 1e-6 * s2 * n_free
    assert info["n_free"] == n_free


# ------------------------------------------------------------------------------------------------ 7
def test_composition_with_pose_priors_and_the_marginal(gpu_available):
    """Pose priors (prior_ref.factor_set) and S together at config 1, fp64: step and covariance blocks equal the dense
    reference with both.  marginal_prior([1]) returns bitwise the same marginal with S set and with it cleared (a ray
    prior belongs to the landmark that stays), and leaves the handle linearised with S: a step built straight after
    the call still matches the reference."""
    import cov_ref
    p = rref.problem("config1")
    S = list(rref.standard("config1"))
    factors = prior_ref.factor_set(p)
    dx = rref.gn_step(p, p.init_ptz, p.init_rays, S, factors)[0]
    dx_pose_only = prior_ref.gn_step(p, p.init_ptz, p.init_rays, factors)[0]
    dx_ray_only = _ref_steps("config1")[0]
    for other in (dx_pose_only, dx_ray_only):
        assert np.abs(dx - other).max() / np.abs(dx).max() >= 10 * STEP_TOL[0]
    h = _handle("config1", rpriors=S, factors=factors)
    assert h.pose_prior_info()[0] == len(factors) and h.ray_prior_info()[0] == len(S)
    dx_gpu, _ = _gpu_step(h, p)
    err = np.abs(dx_gpu - dx).max() / np.abs(dx).max()
    h.set_state(p.init_ptz, p.init_rays)
    H = rref.normal_matrix(p, p.init_ptz, p.init_rays, S, factors)
    pose_ref, ray_ref = cov_ref._cut(np.linalg.inv(H), p.n_pose, p.n_landmark, 1)
    pose, ray, _ = h.covariance("all")
    ep, er = cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref)
    print(f"pose + ray priors: step error {err:.3e}; covariance pose {ep:.3e} ray {er:.3e}")
    assert err < STEP_TOL[0] and ep <= TOL[0] and er <= TOL[0]
    # the marginal of frame 1 with S set ...
    m1, st1 = h.marginal_prior([1])
    dx_after, _ = _gpu_step(h, p, linearize=False)
    err_after = np.abs(dx_after - dx).max() / np.abs(dx).max()
    print(f"step built straight after marginal_prior: error {err_after:.3e}")
    assert err_after < STEP_TOL[0]
    # ... and with it cleared
    h.set_state(p.init_ptz, p.init_rays)
    h.clear_ray_priors()
    m0, st0 = h.marginal_prior([1])
    h.close()
    assert m1.frames.tobytes() == m0.frames.tobytes() and m1.lin.tobytes() == m0.lin.tobytes()
    assert m1.info.tobytes() == m0.info.tobytes() and m1.grad.tobytes() == m0.grad.tobytes() and m1.offset == m0.offset
    assert st1["dropped_records"] == st0["dropped_records"] and st1["absorbed"] == st0["absorbed"]


# ------------------------------------------------------------------------------------------------ 8
def test_no_trace(gpu_available):
    """Ray priors set and cleared leave no trace: the solve is bitwise that of a handle that never had any (state,
    cost, iterations) and solver_info / info are unchanged; set_problem clears them; a covariance() call between
    setting the priors and the solve does not change the solve; two solves with the same priors are bitwise equal."""
    import ptzba
    p = rref.problem("config2")
    S = list(rref.standard("config2"))

    def run(h):
        h.set_state(p.init_ptz, p.init_rays)
        res = ptzba.LMSolver(h, ftol=1e-10, xtol=1e-12, max_iter=30).run()
        ptz, rays = h.get_state()
        return ptz.tobytes(), rays.tobytes(), res.cost, res.njev, res.nfev, res.status

    fresh = _handle("config2", precision=1, loss=1)
    a = run(fresh)
    infos = fresh.solver_info(), {k: v for k, v in fresh.info().items() if k != "device_bytes"}
    fresh.close()
    h = _handle("config2", precision=1, loss=1, rpriors=S)
    assert (h.solver_info(), {k: v for k, v in h.info().items() if k != "device_bytes"}) == infos
    with_1 = run(h)
    with_2 = run(h)
    assert with_1 == with_2
    assert with_1[1] != a[1]
    h.set_state(p.init_ptz, p.init_rays)
    h.covariance("all")
    with_3 = run(h)
    assert with_3 == with_1
    h.clear_ray_priors()
    b = run(h)
    assert b == a
    h.set_ray_priors(S)
    assert h.ray_prior_info()[0] == len(S)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=1, loss=1)
    assert h.ray_prior_info() == (0, 0, 0, 0.0)
    c = run(h)
    h.close()
    assert c == a


# ------------------------------------------------------------------------------------------------ 9
def _native_set(h, landmarks, means, infos, struct_size=None):
    """ptzba_set_ray_priors straight through ctypes (no Python-side validation); returns (rc, message)."""
    import ptzba
    lm = np.ascontiguousarray(landmarks, np.int32)
    mean = np.ascontiguousarray(np.asarray(means, np.float64).reshape(-1))
    info = np.ascontiguousarray(np.asarray(infos, np.float64).reshape(-1))
    pr = ptzba.ptzba_ray_priors(ctypes.sizeof(ptzba.ptzba_ray_priors) if struct_size is None else struct_size, len(lm),
                                lm.ctypes.data, mean.ctypes.data, info.ctypes.data)
    rc = ptzba.lib().ptzba_set_ray_priors(h.h, ctypes.byref(pr))
    return rc, ptzba.lib().ptzba_last_error().decode()


def test_refusals(gpu_available):
    """Every refusal of ptzba_set_ray_priors, each with its message and the handle's priors left as they were."""
    import ptzba
    p = rref.problem("config1")
    keep = p.landmark != 4  # landmark 4 loses its records
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame[keep], p.landmark[keep], p.xy[keep], p.u, p.v)
    h.set_state(p.init_ptz, p.init_rays)
    S = [s for s in rref.standard("config1") if s[0] != 4]
    h.set_ray_priors(S)
    before = h.ray_prior_info()
    assert before[0] == len(S) and before[3] > 0
    z2, eye = [0.0, 0.0], [1.0, 0.0, 1.0]
    cases = [
        ("out of range", [p.n_landmark], [z2], [eye]),
        ("out of range", [-1], [z2], [eye]),
        ("out of range", [3, p.n_landmark + 7], [z2, z2], [eye, eye]),
        ("no records", [4], [z2], [eye]),
        ("non-finite mean", [3], [[0.0, np.inf]], [eye]),
        ("non-finite mean", [3], [[np.nan, 0.0]], [eye]),
        ("non-finite information", [3], [z2], [[1.0, np.nan, 1.0]]),
        ("non-finite information", [3], [z2], [[np.inf, 0.0, 1.0]]),
        ("negative diagonal", [3], [z2], [[-1e-3, 0.0, 1.0]]),
        ("negative diagonal", [3], [z2], [[1.0, 0.0, -1.0]]),
        ("not positive semi-definite", [3], [z2], [[1.0, 1.0 + 1e-9, 1.0]]),
        ("not positive semi-definite", [3], [z2], [[0.0, 1e-3, 5.0]]),
    ]
    for needle, lms, means, infos in cases:
        rc, msg = _native_set(h, lms, means, infos)
        assert rc != 0 and "ptzba_set_ray_priors" in msg and needle in msg, (needle, rc, msg)
        assert h.ray_prior_info() == before, needle
    rc, msg = _native_set(h, [3], [z2], [eye], struct_size=24)
    assert rc != 0 and "struct_size" in msg and h.ray_prior_info() == before
    # a rank-one information matrix (L01^2 == L00 L11) is positive semi-definite: accepted
    rc, msg = _native_set(h, [3], [p.init_rays[3] + 1.0], [[4.0, 2.0, 1.0]])
    assert rc == 0, msg
    assert h.ray_prior_info()[:3] == (1, 1, 2) and abs(h.ray_prior_info()[3] - 4.5) <= 1e-12
    h.set_ray_priors(S)
    assert h.ray_prior_info() == before
    # the Python layer passes the library's refusal on
    with pytest.raises(ptzba.PtzbaError, match="no records"):
        h.set_ray_priors([(4, z2, np.eye(2))])
    assert h.ray_prior_info() == before
    # a pending LM trial
    h.linearize()
    h.step(1e-3)
    rc, msg = _native_set(h, [3], [z2], [eye])
    assert rc != 0 and "trial is pending" in msg
    h.accept(False)
    assert h.ray_prior_info() == before
    # with ray priors set, an exchange cannot be attached
    with pytest.raises(ptzba.PtzbaError, match="ray priors"):
        h.set_exchange_hook(lambda kind, ptr, count, stream: None)
    rc = ptzba.lib().ptzba_attach_comm(h.h, ctypes.c_void_p(1))  # (refused before the pointer is looked at)
    assert rc != 0 and "ray priors" in ptzba.lib().ptzba_last_error().decode()
    # a handle with a hook, a handle on the caller-run exchange protocol and a sharded handle take no ray priors
    h.clear_ray_priors()
    h.set_exchange_hook(lambda kind, ptr, count, stream: None)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        h.set_ray_priors(S)
    h.set_exchange_hook(None)
    h.set_ray_priors(S)
    assert h.ray_prior_info() == before
    h.clear_ray_priors()
    h.exchange()
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        h.set_ray_priors(S)
    assert h.ray_prior_info() == (0, 0, 0, 0.0)
    h.close()
    g = ptzba.BAHandle(0)
    w1 = ptzba.frame_coupling_window(p.n_pose, p.frame, p.landmark)
    g.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, frame_win_hi=w1, dist_world=2,
                  dist_rank=0)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        g.set_ray_priors(list(rref.standard("config1")))
    g.close()
    e = ptzba.BAHandle(0)
    with pytest.raises(ptzba.PtzbaError, match="no problem set"):
        e.ray_prior_info()
    e.close()


# ------------------------------------------------------------------------------------------------ 10
def test_dropin_ray_priors_from_the_first_call(gpu_available):
    """bundle_adjustment() on the ba_6x120 golden twice: the second call takes ray_priors_from_result of the first
    (inflate 1, means at the first call's rays).  Every key resolves (none skipped); each returned ray lies within one
    prior sigma of the first call's ray (e^T info e <= 1); every ray covariance block with a prior is smaller than the
    first call's (trace ratio < 1).  (Posterior as prior over the same observations counts them twice -- here that is
    the point: the second posterior must be tighter.)"""
    import random
    import image_process
    import bundle_adjustment as ba
    import ptzba
    from test_gpu_ba import _install_fixture_frontend
    d = golden("ba_6x120.npz")
    n = int(d["n_pose"])

    def call(**kw):
        saved, _ = _install_fixture_frontend(d)
        try:
            random.seed(int(d["seed"]))
            return ba.bundle_adjustment(list(range(n)), list(range(100, 100 + n)), "sift", d["init_ptz"].copy(),
                                        np.array([0.0, -10.0, 5.0]), np.eye(3), float(d["u"]), float(d["v"]), "",
                                        ftol=1e-14, xtol=1e-14, max_iter=200, covariance=True, **kw)
        finally:
            image_process.detect_compute_sift, image_process.match_sift_features = saved

    lm0, kf0, cov0 = call()
    assert "ray_priors_used" not in ba.LAST_RESULT
    keyed = ptzba.ray_priors_from_result(kf0, lm0, cov0["ray_cov"], inflate=1.0)
    has = np.array([c.any() for c in cov0["ray_cov"]])
    assert len(keyed) == int(has.sum()) > 0
    lm1, kf1, cov1 = call(ray_priors=keyed)
    assert ba.LAST_RESULT["ray_priors_skipped"] == [] and ba.LAST_RESULT["ray_priors_used"] == len(keyed)
    assert lm1.shape == lm0.shape
    ids = np.flatnonzero(has)
    worst_m, worst_t = 0.0, 0.0
    for l, (_, _, mean, info) in zip(ids, keyed):
        np.testing.assert_array_equal(mean, lm0[l])
        e = lm1[l] - lm0[l]
        worst_m = max(worst_m, float(e @ info @ e))
        worst_t = max(worst_t, float(np.trace(cov1["ray_cov"][l]) / np.trace(cov0["ray_cov"][l])))
    print(f"{len(keyed)} ray priors: largest e^T info e {worst_m:.3e}; largest trace ratio {worst_t:.3f}")
    assert worst_m <= 1.0
    assert worst_t < 1.0
