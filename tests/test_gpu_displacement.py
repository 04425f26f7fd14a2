"""GPU tests of the projection-centre displacement in the bundle adjuster (ptzba_set_displacement:
BAHandle.set_displacement, ptzba.solve's and the drop-in's `displacement=`).

Reference (tests/disp_ref.py, pinned to the oracle's PTZCamera projection by test_displacement_cpu.py): the displaced
model's residual and analytic Jacobian in fp64.  The problems are synthetic configs 1 and 2 seen through the camera
with the golden fixtures' displacement (disp_ref.displaced_problem): observations move by up to 234 / 274 px.
Tolerances are the project's own for the same quantities: the Gauss-Newton step's and the residual's (test_gpu_ba),
the covariance blocks' (test_gpu_covariance), the marginal's (test_gpu_marginal), the converged solve's gates of
test_gpu_ray_priors."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, golden

import disp_ref
import prior_ref
import ray_prior_ref as rref
from disp_ref import LAMBDA, ZERO
from test_gpu_covariance import TOL
from test_gpu_k1_merge import _knob_off
from test_gpu_ray_priors import STEP_TOL, _frozen, _gpu_step

pytestmark = pytest.mark.gpu

# px; fp32: test_gpu_ba.test_residual_matches_reference's own (times max(1, largest residual / 1e3), as there); fp64:
# 1e-9, ten times tighter than that test's 1e-8 -- the reference here is evaluated on the same records in fp64
RESID_TOL = {0: 1e-9, 1: 2e-3}


def _problem(cfg):
    return disp_ref.displaced_problem(cfg)[0]


def _handle(p, precision=0, ordering=0, loss=0, lam=LAMBDA, factors=None, rpriors=None, state=None, records=None):
    """records: (frame, landmark, xy, weight) in place of p's own pair form."""
    import ptzba
    win = ptzba.prior_window(p.n_pose, p.frame, p.landmark, factors) if factors else None
    h = ptzba.BAHandle(0)
    fr, lm, xy, w = records if records is not None else (p.frame, p.landmark, p.xy, None)
    h.set_problem(p.n_pose, p.n_landmark, fr, lm, xy, p.u, p.v, weight=w, precision=precision, ordering=ordering,
                  loss=loss, f_scale=1.0, frame_win_hi=win)
    if factors:
        h.set_pose_priors(factors)
    if rpriors:
        h.set_ray_priors(rpriors)
    if lam is not None:
        h.set_displacement(lam)
    ptz, rays = state if state is not None else (p.init_ptz, p.init_rays)
    h.set_state(ptz, rays)
    return h


@functools.lru_cache(maxsize=None)
def _ref_steps(cfg):
    """(dx under LAMBDA, dx of the displacement-free model) of one undamped Gauss-Newton step at the initial state."""
    p = _problem(cfg)
    dx1 = disp_ref.gn_step(p, p.init_ptz, p.init_rays, LAMBDA)[0]
    dx0 = disp_ref.gn_step(p, p.init_ptz, p.init_rays, ZERO)[0]
    return _frozen(dx1), _frozen(dx0)


def _step_err(dx_gpu, dx):
    return np.abs(dx_gpu - dx).max() / np.abs(dx).max()


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cfg,ordering", [("config1", 0), ("config2", 0), ("config2", 2)])
@pytest.mark.parametrize("precision", [0, 1])
def test_gauss_newton_step_under_the_displaced_model_is_exact(gpu_available, precision, cfg, ordering):
    """One undamped step == disp_ref.gn_step under LAMBDA, to test_single_gauss_newton_step_is_exact's tolerance; the
    displacement-free reference step is at least 10 tolerances away (measured 0.43 / 0.52 of the step's largest
    entry), so a build that ignored the displacement could not pass."""
    p = _problem(cfg)
    dx, dx_plain = _ref_steps(cfg)
    tol = STEP_TOL[precision]
    moved = _step_err(dx_plain, dx)
    assert moved >= 10 * tol, moved
    h = _handle(p, precision, ordering)
    if ordering == 2:
        assert h.solver_info()["ordering"] == "nested"
    dx_gpu, _ = _gpu_step(h, p)
    h.close()
    err = _step_err(dx_gpu, dx)
    print(f"{cfg} ordering {ordering} precision {precision}: step error {err:.3e} (tol {tol:.0e}); the displacement "
          f"moves the step by {moved:.3e}")
    assert err < tol, err


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("form", ["pair_one_record", "pair_unmerged", "dedup_weighted"])
@pytest.mark.parametrize("precision", [0, 1])
def test_every_k1_form_takes_the_displaced_path(gpu_available, precision, form):
    """Config 2 through each linearisation kernel form: the pair form merges to one record per segment
    (k_linearize_one), the same records with PTZBA_K1_MERGE=0 run the general k_linearize without weights, the
    de-duplicated records with multiplicities run its weighted instantiation.  All against the same reference step."""
    import synthetic
    p = _problem("config2")
    dx, dx_plain = _ref_steps("config2")
    tol = STEP_TOL[precision]
    if form == "pair_one_record":
        h = _handle(p, precision)
        info = h.k1_merge_info()
        assert info["merged"] and info["one_record"], info
    elif form == "pair_unmerged":
        with _knob_off():
            h = _handle(p, precision)
        info = h.k1_merge_info()
        assert not info["merged"] and not info["one_record"], info
    else:
        f, l, xy, w, _ = synthetic.dedup_records(p.frame, p.landmark, p.xy)
        assert len(f) < len(p.frame) and w.max() > 1
        h = _handle(p, precision, records=(f, l, xy, w))
        info = h.k1_merge_info()
        assert not info["one_record"], info
    dx_gpu, _ = _gpu_step(h, p)
    h.close()
    err = _step_err(dx_gpu, dx)
    print(f"{form} precision {precision}: step error {err:.3e} (tol {tol:.0e}); displacement-free step "
          f"{_step_err(dx_plain, dx):.3e} away; {info}")
    assert err < tol, err


@functools.lru_cache(maxsize=None)
def _crafted(kind):
    """k1_cases.craft() -- 400 frames, landmarks seen by every frame: workgroups on the global-table fallback of the
    LDS-table kernels, landmarks walked in four segment windows -- under LAMBDA.  The observations move by
    proj_LAMBDA(x0) - proj_0(x0), so the residuals at x0 stay what k1_cases made them and only the Jacobian tells the
    two models apart.  kind: "general" (k_linearize, unweighted), "weighted" (integer multiplicities), "one_record"
    (the first record of every segment, twice: merged to one record per segment, k_linearize_one);
    "one_record_plain": the same with the observations left where k1_cases put them (a problem of the displacement-free
    model).  Returns
    (problem for the handle, weight, reference step under LAMBDA, displacement-free reference step)."""
    import types
    import k1_cases as kc
    u, v, ptz0, rays0, frame, landmark, xy, weight = kc.craft(weighted=kind == "weighted")
    if kind.startswith("one_record"):
        _, first = np.unique(landmark.astype(np.int64) * len(ptz0) + frame, return_index=True)
        first = np.sort(first)
        frame, landmark, xy = np.repeat(frame[first], 2), np.repeat(landmark[first], 2), np.repeat(xy[first], 2, axis=0)
    if not kind.endswith("_plain"):
        xy = xy + (disp_ref.project(u, v, ptz0[frame], rays0[landmark], LAMBDA)[0] -
                   disp_ref.project(u, v, ptz0[frame], rays0[landmark], ZERO)[0])
    p = types.SimpleNamespace(n_pose=len(ptz0), n_landmark=len(rays0), frame=frame, landmark=landmark, xy=xy, u=u, v=v,
                              init_ptz=ptz0, init_rays=rays0)
    k = np.ones(len(frame), np.int64) if weight is None else weight.astype(np.int64)
    full = types.SimpleNamespace(**{**vars(p), "frame": np.repeat(frame, k), "landmark": np.repeat(landmark, k),
                                    "xy": np.repeat(xy, k, axis=0)})  # every record repeated `weight` times
    dx1 = disp_ref.gn_step(full, ptz0, rays0, LAMBDA)[0]
    dx0 = disp_ref.gn_step(full, ptz0, rays0, ZERO)[0]
    _crafted_full[kind] = full
    return p, weight, _frozen(dx1), _frozen(dx0)


_crafted_full = {}  # kind -> the expanded records of _crafted(kind), for the robust reference below


@functools.lru_cache(maxsize=None)
def _crafted_lin(kind, lam_key):
    """(J, r) of _crafted(kind)'s expanded records at x0 under LAMBDA ("disp") or without a displacement ("plain")."""
    _crafted(kind)
    full = _crafted_full[kind]
    lam = LAMBDA if lam_key == "disp" else ZERO
    return (disp_ref.jacobian(full, full.init_ptz, full.init_rays, lam),
            _frozen(disp_ref.residual(full, full.init_ptz, full.init_rays, lam)))


@functools.lru_cache(maxsize=None)
def _crafted_robust_step(kind, loss, hcurv, lam_key):
    """One undamped step of the robust cost on _crafted(kind): disp_ref's displaced Jacobian and residual with
    loss_ref.weights' gradient weight w1 = rho' and curvature weight w2 = max(rho' + 2 z rho'', hcurv rho') (huber:
    hcurv rho' beyond the unit), f_scale 1 as _handle sets it: (J^T diag(w2) J) dx = -J^T (w1 r)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    import loss_ref
    J, r = _crafted_lin(kind, lam_key)
    _, _, w1, w2 = loss_ref.weights(r, loss, hcurv, 1.0)
    H = (J.T @ sp.diags(w2) @ J).tocsc()
    return _frozen(spla.spsolve(H, -np.asarray(J.T @ (w1 * r)).reshape(-1)))


@pytest.mark.parametrize("kind", ["general", "weighted", "one_record"])
@pytest.mark.parametrize("precision", [0, 1])
def test_global_table_fallback_takes_the_displaced_path(gpu_available, precision, kind):
    """The `!ftl_ok` workgroups (frame range beyond the LDS table) of k_linearize and k_linearize_one under LAMBDA: one
    undamped step on k1_cases' 400-frame problem against disp_ref.gn_step; k1_info says the launch had workgroups on
    both table paths."""
    p, weight, dx, dx_plain = _crafted(kind)
    tol = STEP_TOL[precision]
    moved = _step_err(dx_plain, dx)
    assert moved >= 10 * tol, moved
    h = _handle(p, precision, records=(p.frame, p.landmark, p.xy, weight))
    info, merge = h.k1_info(), h.k1_merge_info()
    assert 1 <= info[2] < info[1], info  # at least one workgroup on either frame-table path
    assert merge["one_record"] == (kind == "one_record"), merge
    dx_gpu, _ = _gpu_step(h, p)
    h.close()
    err = _step_err(dx_gpu, dx)
    print(f"crafted {kind} precision {precision}: step error {err:.3e} (tol {tol:.0e}); displacement-free step "
          f"{moved:.3e} away; k1_info {info}; {merge}")
    assert err < tol, err


@pytest.mark.parametrize("loss", ["huber", "soft_l1", "cauchy", "arctan"])
@pytest.mark.parametrize("kind", ["general", "weighted", "one_record"])
@pytest.mark.parametrize("precision", [0, 1])
def test_robust_losses_take_the_displaced_path_on_both_table_paths(gpu_available, precision, kind, loss):
    """The displaced instantiations of k_linearize (unweighted, weighted) and k_linearize_one under each robust loss,
    with workgroups on the LDS table and on the `!ftl_ok` fallback in one launch: the same problem, gate (STEP_TOL) and
    guard as the linear test above, against _crafted_robust_step.  Curvature weight: the library's default
    (ptzba.HUBER_CURVATURE = 0.1), so the floor branch of w2 is taken by a share of the records
    (loss_ref.negative_curvature_share) and Huber's outer branch scales by it."""
    import ptzba
    p, weight, _, _ = _crafted(kind)
    hc = ptzba.HUBER_CURVATURE
    dx = _crafted_robust_step(kind, loss, hc, "disp")
    dx_plain = _crafted_robust_step(kind, loss, hc, "plain")
    tol = STEP_TOL[precision]
    moved = _step_err(dx_plain, dx)
    assert moved >= 10 * tol, moved
    h = _handle(p, precision, loss=ptzba.LOSS_IDS[loss], records=(p.frame, p.landmark, p.xy, weight))
    h.set_huber_curvature(hc)
    info, merge = h.k1_info(), h.k1_merge_info()
    assert 1 <= info[2] < info[1], info  # at least one workgroup on either frame-table path
    assert merge["one_record"] == (kind == "one_record"), merge
    dx_gpu, _ = _gpu_step(h, p)
    h.close()
    err = _step_err(dx_gpu, dx)
    print(f"crafted {kind} {loss} precision {precision}: step error {err:.3e} (tol {tol:.0e}); displacement-free "
          f"step {moved:.3e} away; k1_info {info}; {merge}")
    assert err < tol, err


@pytest.mark.parametrize("loss", ["linear", "huber", "soft_l1", "cauchy", "arctan"])
@pytest.mark.parametrize("precision", [0, 1])
def test_one_record_kernel_without_displacement_on_both_table_paths(gpu_available, precision, loss):
    """k_linearize_one's displacement-free instantiations under every loss with workgroups on both table paths (the
    merge tests run it on 140 frames, inside the LDS table): k1_cases' own observations in the one-record pair form, no
    displacement set, against _crafted_robust_step without one; STEP_TOL and the library's default curvature weight as
    above."""
    import ptzba
    p, weight, _, _ = _crafted("one_record_plain")
    hc = ptzba.HUBER_CURVATURE
    dx = _crafted_robust_step("one_record_plain", loss, hc, "plain")
    tol = STEP_TOL[precision]
    h = _handle(p, precision, loss=ptzba.LOSS_IDS[loss], lam=None, records=(p.frame, p.landmark, p.xy, weight))
    h.set_huber_curvature(hc)
    info, merge = h.k1_info(), h.k1_merge_info()
    assert 1 <= info[2] < info[1], info
    assert merge["one_record"] and h.displacement_info()[0] == 0, (merge, h.displacement_info())
    dx_gpu, _ = _gpu_step(h, p)
    h.close()
    err = _step_err(dx_gpu, dx)
    print(f"crafted one_record_plain {loss} precision {precision}: step error {err:.3e} (tol {tol:.0e}); k1_info {info}")
    assert err < tol, err


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("cfg", ["config1", "config2"])
@pytest.mark.parametrize("precision", [0, 1])
def test_residual_in_record_order(gpu_available, precision, cfg):
    """ptzba_residual under LAMBDA == disp_ref.residual in record order (test_gpu_ba's residual tolerances), and
    is the displacement-free residual again after clearing."""
    p = _problem(cfg)
    x = np.concatenate([p.init_ptz.reshape(-1), p.init_rays.reshape(-1)])
    ref = disp_ref.residual(p, p.init_ptz, p.init_rays, LAMBDA)
    plain = disp_ref.residual(p, p.init_ptz, p.init_rays, ZERO)
    h = _handle(p, precision)
    r = h.residual(x)
    h.clear_displacement()
    r0 = h.residual(x)
    h.close()
    tol = RESID_TOL[precision] * (1.0 if precision == 0 else max(1.0, np.abs(ref).max() / 1e3))
    tol0 = RESID_TOL[precision] * (1.0 if precision == 0 else max(1.0, np.abs(plain).max() / 1e3))
    err, err0 = np.abs(r - ref).max(), np.abs(r0 - plain).max()
    print(f"{cfg} precision {precision}: residual error {err:.3e} px (tol {tol:.1e}), largest residual "
          f"{np.abs(ref).max():.1f} px; cleared {err0:.3e} px; the two models differ by "
          f"{np.abs(ref - plain).max():.1f} px")
    assert r.shape == ref.shape
    assert np.abs(ref - plain).max() > 100.0
    assert err <= tol and err0 <= tol0, (err, err0)


# ------------------------------------------------------------------------------------------------ 4
@functools.lru_cache(maxsize=None)
def _optimum_config1():
    p = _problem("config1")
    ptz, rays, c, _ = disp_ref.solve(p, p.init_ptz, p.init_rays, LAMBDA)
    return _frozen(ptz), _frozen(rays), c


def test_converged_solve_on_every_path(gpu_available):
    """Config 1, fp64: the host loop, the device loop, ptzba_solve and ptzba_solve_resident take identical iterates
    and all stop at disp_ref's stationary point (1e-6 deg / 1e-4 px, test_gpu_ray_priors' gate), within 0.02 deg /
    5 px of the ground truth; the displacement persists over set_state / save_state / restore_state."""
    import ptzba
    p = _problem("config1")
    ptz_ref, rays_ref, c_ref = _optimum_config1()
    kw = dict(ftol=1e-14, xtol=1e-14, max_iter=100)
    out = []
    for device_loop in (False, True):
        h = _handle(p)
        res = ptzba.LMSolver(h, device_loop=device_loop, **kw).run()
        out.append((res,) + h.get_state())
        h.close()
    h = _handle(p)
    one = h.solve(p.init_ptz, p.init_rays, **kw)
    out.append((one[2],) + h.get_state())
    h.set_state(p.init_ptz, p.init_rays)
    h.save_state()
    res = h.solve_resident(restore=True, **kw)
    out.append((res,) + h.get_state())
    active, lam = h.displacement_info()
    h.close()
    assert active and np.array_equal(lam, LAMBDA)
    r0, p0, y0 = out[0]
    for name, (r, ptz, rays) in zip(("host loop", "device loop", "ptzba_solve", "ptzba_solve_resident"), out):
        ea, ef = disp_ref.pose_error(ptz, ptz_ref)
        ga, gf = disp_ref.pose_error(ptz, p.gt_ptz)
        print(f"{name}: {r}; {ea:.2e} deg / {ef:.2e} px from the reference optimum, {ga:.4f} deg / {gf:.2f} px from "
              f"the ground truth")
        assert (r.njev, r.nfev, r.status) == (r0.njev, r0.nfev, r0.status), (name, r, r0)
        assert abs(r.cost - r0.cost) <= 1e-12 * r0.cost
        np.testing.assert_allclose(ptz, p0, rtol=0, atol=1e-10)
        np.testing.assert_allclose(rays, y0, rtol=0, atol=1e-10)
        np.testing.assert_allclose(ptz[:, :2], ptz_ref[:, :2], rtol=0, atol=1e-6)
        np.testing.assert_allclose(ptz[:, 2], ptz_ref[:, 2], rtol=0, atol=1e-4)
        np.testing.assert_allclose(rays, rays_ref, rtol=0, atol=1e-6)
        assert abs(r.cost - c_ref) <= 1e-9 * c_ref
        assert ga <= 0.02 and gf <= 5.0, (ga, gf)


# ------------------------------------------------------------------------------------------------ 5
def test_converged_solve_config2_fp32_huber(gpu_available):
    """Config 2, Huber (f_scale 1), through ptzba.solve(displacement=LAMBDA) against disp_ref's stationary point of the
    displaced Huber objective, recorded (tests/golden/displacement_config2_huber.npz) and its stationarity re-checked
    here.  fp32: the poses stop within 1e-6 deg / 1e-4 px of it.  The default curvature heuristic reaches that gate
    here (measured on an MI355X: 6.6e-8 deg / 2.5e-5 px, status 5, 5 iterations; plain IRLS, huber_curvature=1, ends
    1.5e-7 deg / 5.1e-5 px away after 11), so the solve runs with the defaults.

    The rays are gated in fp64, at test 4's 1e-6 deg (measured 8.2e-8), and printed, not gated, in fp32: the project
    gates its fp32 solves on the poses (test_gpu_ba.test_config2_huber, test_gpu_ray_priors' same test; DESIGN 4.11:
    the largest single fp32 difference is a weakly observed ray -- a pose's gradient sums thousands of fp32 terms, a
    ray seen by two or three frames a handful).  Measured here: the worst fp32 ray ends 4.8e-5 deg away."""
    import ptzba
    p = _problem("config2")
    golden(disp_ref.CONFIG2_HUBER)
    ptz_ref, rays_ref, c_ref = disp_ref.config2_huber_point(os.path.join(GOLDEN, disp_ref.CONFIG2_HUBER))
    for precision, name in ((ptzba.FP32, "fp32"), (ptzba.FP64, "fp64")):
        ptz, rays, res = ptzba.solve(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, p.init_ptz,
                                     p.init_rays, precision=precision, loss=ptzba.LOSS_HUBER, f_scale=1.0, ftol=1e-12,
                                     xtol=1e-12, max_iter=100, displacement=LAMBDA, keep_handle=False)
        ea, ef = disp_ref.pose_error(ptz, ptz_ref)
        er = float(np.abs(rays - rays_ref).max())
        print(f"config2 {name} huber under the displacement: {res}; {ea:.3e} deg / {ef:.3e} px / rays {er:.3e} deg "
              f"from the recorded point; cost {res.cost!r} vs {c_ref!r}")
        assert ea <= 1e-6 and ef <= 1e-4, (name, ea, ef)
        if precision == ptzba.FP64:
            assert er <= 1e-6, er
            assert abs(res.cost - c_ref) <= 1e-9 * c_ref
        else:
            assert abs(res.cost - c_ref) <= 1e-5 * c_ref


# ------------------------------------------------------------------------------------------------ 6
@functools.lru_cache(maxsize=None)
def _ref_inverse(cfg):
    p = _problem(cfg)
    C = np.linalg.inv(disp_ref.normal_matrix(p, p.init_ptz, p.init_rays, LAMBDA))
    C0 = np.linalg.inv(disp_ref.normal_matrix(p, p.init_ptz, p.init_rays, ZERO)) if cfg == "config1" else None
    return _frozen(C), C0


@pytest.mark.parametrize("cfg,ordering,precision", [("config1", 0, 0), ("config1", 0, 1), ("config2", 2, 0)])
def test_covariance_blocks_and_joint_cut(gpu_available, cfg, ordering, precision):
    """covariance() and one covariance_joint cut == the blocks of inv(disp_ref.normal_matrix) (test_gpu_covariance's
    metric and TOL), and not those of the displacement-free inverse."""
    import cov_ref
    import cov_joint_ref as jref
    p = _problem(cfg)
    C, C0 = _ref_inverse(cfg)
    pose_ref, ray_ref = cov_ref._cut(C, p.n_pose, p.n_landmark, 1)
    if C0 is not None:
        assert cov_ref.block_err(cov_ref._cut(C0, p.n_pose, p.n_landmark, 1)[0], pose_ref) >= 10 * TOL[precision]
    h = _handle(p, precision, ordering)
    idx = np.arange(p.n_landmark) if cfg == "config1" else np.arange(0, p.n_landmark, 7)
    pose, ray, info = h.covariance("all" if cfg == "config1" else idx)
    frames = np.array([p.n_pose - 1, 0, 1, p.n_pose // 2], np.int32)
    lms = np.array([p.n_landmark - 1, 3, 0], np.int32)
    joint, _ = h.covariance_joint(frames, lms)
    h.close()
    ep, er = cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref[idx])
    ej = jref.joint_err(joint, jref.cut(C, jref.param_index(p, frames, lms)))
    print(f"{cfg} ordering {ordering} precision {precision}: pose {ep:.3e} ray {er:.3e} joint {ej:.3e} "
          f"(tol {TOL[precision]:.0e})")
    assert ep <= TOL[precision] and er <= TOL[precision] and ej <= TOL[precision], (ep, er, ej)


def test_residual_scale_uses_the_displaced_residual(gpu_available):
    """covariance(scale="residual") at the config 1 optimum == sum r^2 / (2 R - n_free) with disp_ref's residual
    (1e-9); the displacement-free residual at that state gives a scale hundreds of times larger."""
    import ptzba
    p = _problem("config1")
    h = _handle(p)
    res = ptzba.LMSolver(h, ftol=1e-12, xtol=1e-12, max_iter=100).run()
    _, _, info = h.covariance(None, scale="residual")
    info_j = h.covariance_joint([1, 2], [0], scale="residual")[1]
    ptz, rays = h.get_state()
    h.close()
    assert res.status > 0, res
    n_free = 3 * (p.n_pose - 1) + 2 * p.n_landmark
    r = disp_ref.residual(p, ptz, rays, LAMBDA)
    r0 = disp_ref.residual(p, ptz, rays, ZERO)
    s2 = float(r @ r) / (len(r) - n_free)
    print(f"residual scale {info['scale']!r} vs {s2!r} (displacement-free residual: "
          f"{float(r0 @ r0) / (len(r) - n_free):.1f})")
    assert abs(info["scale"] - s2) <= 1e-9 * s2, (info, s2)
    assert abs(info_j["scale"] - s2) <= 1e-9 * s2, (info_j, s2)
    assert float(r0 @ r0) > 100.0 * float(r @ r)


# ------------------------------------------------------------------------------------------------ 7
def test_composition_with_priors_and_the_marginal(gpu_available, monkeypatch):
    """Displacement + pose priors (prior_ref.factor_set) + ray priors (ray_prior_ref.standard_set) together at config
    1, fp64: the step equals the dense reference with all three, and not the reference that lacks any one of them.
    marginal_prior([1]) on that handle equals marg_ref's marginal computed from disp_ref's Jacobian and residual
    (test_gpu_marginal's metric and tolerances), and not the displacement-free one."""
    import marg_ref
    from test_gpu_marginal import _assert_marginal, marg_err
    p = _problem("config1")
    S = rref.standard_set(p)
    factors = prior_ref.factor_set(p)
    dx = disp_ref.gn_step(p, p.init_ptz, p.init_rays, LAMBDA, factors, S)[0]
    for other in (disp_ref.gn_step(p, p.init_ptz, p.init_rays, ZERO, factors, S)[0],
                  disp_ref.gn_step(p, p.init_ptz, p.init_rays, LAMBDA, (), S)[0],
                  disp_ref.gn_step(p, p.init_ptz, p.init_rays, LAMBDA, factors, ())[0]):
        assert _step_err(other, dx) >= 10 * STEP_TOL[0]
    h = _handle(p, factors=factors, rpriors=S)
    assert h.pose_prior_info()[0] == len(factors) and h.ray_prior_info()[0] == len(S) and h.displacement_info()[0]
    dx_gpu, _ = _gpu_step(h, p)
    err = _step_err(dx_gpu, dx)
    print(f"displacement + pose priors + ray priors: step error {err:.3e} (tol {STEP_TOL[0]:.0e})")
    assert err < STEP_TOL[0], err
    h.set_state(p.init_ptz, p.init_rays)
    got, stats = h.marginal_prior([1])
    h.close()
    plain = marg_ref.marginal(p, p.init_ptz, p.init_rays, [1], factors=factors)[0]
    monkeypatch.setattr(prior_ref, "_records", lambda q, ptz, rays, loss, f_scale:
                        disp_ref.records(q, ptz, rays, LAMBDA, loss, f_scale))
    ref, absorbed = marg_ref.marginal(p, p.init_ptz, p.init_rays, [1], factors=factors)
    assert stats["absorbed"] == absorbed and len(absorbed) >= 1
    assert max(marg_err(plain, ref)) >= 10 * STEP_TOL[0]
    _assert_marginal(got, ref, 0, "config1 E=[1] under the displacement")


# ------------------------------------------------------------------------------------------------ 8
def test_off_means_off(gpu_available):
    """Config 2, fp32 + Huber: a solve after set + clear, after setting six zeros, and after a new set_problem is
    bitwise the solve of a handle that never had a displacement (state, cost, iterations), with solver_info / info
    unchanged; covariance() between setting the displacement and the solve leaves that solve bitwise the same."""
    import ptzba
    p = _problem("config2")

    def run(h):
        h.set_state(p.init_ptz, p.init_rays)
        res = ptzba.LMSolver(h, ftol=1e-10, xtol=1e-12, max_iter=30).run()
        ptz, rays = h.get_state()
        return ptz.tobytes(), rays.tobytes(), res.cost, res.njev, res.nfev, res.status

    def infos(h):
        return h.solver_info(), {k: v for k, v in h.info().items() if k != "device_bytes"}

    fresh = _handle(p, precision=1, loss=1, lam=None)
    assert fresh.displacement_info()[0] is False
    a = run(fresh)
    base = infos(fresh)
    fresh.close()
    h = _handle(p, precision=1, loss=1)
    assert infos(h) == base
    with_1 = run(h)
    assert with_1 == run(h)
    assert with_1[0] != a[0]
    h.set_state(p.init_ptz, p.init_rays)
    h.covariance("all")
    assert run(h) == with_1
    h.clear_displacement()
    assert h.displacement_info()[0] is False and not h.displacement_info()[1].any()
    assert run(h) == a
    h.set_displacement(LAMBDA)
    h.set_displacement(np.zeros(6))
    assert h.displacement_info()[0] is False
    assert run(h) == a
    h.set_displacement(LAMBDA)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=1, loss=1)
    assert h.displacement_info()[0] is False
    assert run(h) == a
    h.close()


# ------------------------------------------------------------------------------------------------ 9
def test_refusals(gpu_available):
    """Every refusal of ptzba_set_displacement, each with its message and the handle's displacement left as it was;
    attach / hook are refused while a displacement is set; displacement_info round-trips."""
    import ptzba
    p = _problem("config1")
    h = _handle(p)
    active, lam = h.displacement_info()
    assert active is True and lam.tobytes() == LAMBDA.tobytes()
    out8 = np.full(8, -1.0)
    assert ptzba.lib().ptzba_displacement_info(h.h, ctypes.c_void_p(out8.ctypes.data)) == 0
    assert out8[0] == 1.0 and out8[7] == 0.0 and out8[1:7].tobytes() == LAMBDA.tobytes()

    def native(d6):
        d = np.ascontiguousarray(d6, np.float64)
        rc = ptzba.lib().ptzba_set_displacement(h.h, ctypes.c_void_p(d.ctypes.data))
        return rc, ptzba.lib().ptzba_last_error().decode()

    for k, bad in ((2, np.nan), (5, np.inf), (0, -np.inf)):
        d = 2.0 * LAMBDA
        d[k] = bad
        rc, msg = native(d)
        assert rc != 0 and "ptzba_set_displacement" in msg and "non-finite" in msg, (rc, msg)
        assert h.displacement_info()[1].tobytes() == LAMBDA.tobytes()
    with pytest.raises(ptzba.PtzbaError, match="non-finite"):
        h.set_displacement([0, 0, 0, np.nan, 0, 0])
    # a pending LM trial
    h.linearize()
    h.step(1e-3)
    rc, msg = native(2.0 * LAMBDA)
    assert rc != 0 and "trial is pending" in msg
    rc, msg = native(np.zeros(6))
    assert rc != 0 and "trial is pending" in msg
    h.accept(False)
    assert h.displacement_info()[1].tobytes() == LAMBDA.tobytes()
    # with a displacement set, an exchange cannot be attached
    with pytest.raises(ptzba.PtzbaError, match="displacement"):
        h.set_exchange_hook(lambda kind, ptr, count, stream: None)
    # (the library's communicators need RCCL ranks, so the call gets a token pointer: it must be refused before the
    # pointer is looked at.  Should it ever be accepted, the token is detached again before the assertion fails, so
    # that the handle is not left holding it)
    rc = ptzba.lib().ptzba_attach_comm(h.h, ctypes.c_void_p(1))
    msg = ptzba.lib().ptzba_last_error().decode()
    if rc == 0:
        ptzba.lib().ptzba_attach_comm(h.h, None)
    assert rc != 0 and "displacement" in msg, (rc, msg)
    # a handle with a hook, a handle on the caller-run exchange protocol and a sharded handle take no displacement
    h.clear_displacement()
    h.set_exchange_hook(lambda kind, ptr, count, stream: None)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        h.set_displacement(LAMBDA)
    h.set_displacement(None)  # (clearing is always allowed)
    h.set_exchange_hook(None)
    h.set_displacement(2.0 * LAMBDA)
    assert h.displacement_info()[1].tobytes() == (2.0 * LAMBDA).tobytes()
    h.clear_displacement()
    h.exchange()
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        h.set_displacement(LAMBDA)
    assert h.displacement_info()[0] is False
    h.close()
    g = ptzba.BAHandle(0)
    w1 = ptzba.frame_coupling_window(p.n_pose, p.frame, p.landmark)
    g.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, frame_win_hi=w1, dist_world=2,
                  dist_rank=0)
    with pytest.raises(ptzba.PtzbaError, match="single rank"):
        g.set_displacement(LAMBDA)
    g.close()
    e = ptzba.BAHandle(0)
    with pytest.raises(ptzba.PtzbaError, match="no problem set"):
        e.displacement_info()
    with pytest.raises(ptzba.PtzbaError, match="no problem set"):
        e.set_displacement(LAMBDA)
    e.close()


# ------------------------------------------------------------------------------------------------ 10
class _DisplacedFrontEnd:
    """synthetic.RayFrontEnd with the keypoints rendered by the displaced model (disp_ref.project)."""

    def __init__(self, rays, cams, lam):
        import synthetic
        self.fe = synthetic.RayFrontEnd(rays, cams)
        self.lam = np.asarray(lam, np.float64)
        self.fe.keypoints = self.keypoints

    def keypoints(self, im, nfeatures=0):
        fe = self.fe
        n = len(fe.rays)
        xy, q2 = disp_ref.project(fe.u, fe.v, np.tile(fe.cams[int(im)], (n, 1)), fe.rays, self.lam)
        vis = np.flatnonzero((q2 > 0) & (xy[:, 0] > 0) & (xy[:, 0] < fe.width) & (xy[:, 1] > 0) &
                             (xy[:, 1] < fe.height))
        if nfeatures:
            vis = vis[:nfeatures]
        pts = xy[vis].copy()
        for k, r in enumerate(vis):
            g = np.random.default_rng(fe.seed * 1000003 + int(im) * 100003 + int(r))
            pts[k] += g.normal(0, fe.noise, 2)
        return pts, vis


def test_dropin_displacement(gpu_available):
    """bundle_adjustment(..., displacement=LAMBDA) on a 6-keyframe scene whose keypoints are rendered with LAMBDA
    returns poses as close to the truth as the plain call does on the same scene rendered without a displacement
    (within twice that error); the plain call on the displaced keypoints misses by more than ten times it."""
    import image_process
    import bundle_adjustment as ba
    rng = np.random.default_rng(21)
    rays = np.stack([rng.uniform(25, 75, 600), rng.uniform(-20, 4, 600)], 1)
    cams = np.stack([np.linspace(40.0, 60.0, 6), rng.uniform(-9.0, -7.0, 6), rng.uniform(2800.0, 3200.0, 6)], 1)
    init = cams.copy()
    init[1:] += rng.normal(0.0, 1.0, (5, 3)) * np.array([0.5, 0.2, 40.0])

    def call(lam_scene, **kw):
        fe = _DisplacedFrontEnd(rays, cams, lam_scene).fe
        saved = image_process.detect_compute_sift, image_process.match_sift_features
        image_process.detect_compute_sift, image_process.match_sift_features = fe.detect, fe.match
        try:
            random.seed(0)
            _, kfs = ba.bundle_adjustment(list(range(6)), list(range(100, 106)), "sift", init.copy(),
                                          np.array([0.0, -10.0, 5.0]), np.eye(3), fe.u, fe.v, "", ftol=1e-14,
                                          xtol=1e-14, max_iter=200, **kw)[:2]
        finally:
            image_process.detect_compute_sift, image_process.match_sift_features = saved
        return np.array([[k.pan, k.tilt, k.f] for k in kfs]), ba.LAST_RESULT["n_landmark"]

    yard, n0 = call(ZERO)
    got, n1 = call(LAMBDA, displacement=LAMBDA)
    miss, _ = call(LAMBDA)
    zeros, _ = call(ZERO, displacement=np.zeros(6))
    ya, yf = disp_ref.pose_error(yard, cams)
    ga, gf = disp_ref.pose_error(got, cams)
    ma, mf = disp_ref.pose_error(miss, cams)
    print(f"yardstick (no displacement anywhere, {n0} landmarks): {ya:.4f} deg / {yf:.2f} px; displaced scene with "
          f"displacement= ({n1} landmarks): {ga:.4f} deg / {gf:.2f} px; without: {ma:.3f} deg / {mf:.1f} px")
    assert n0 > 50 and n1 > 50
    assert zeros.tobytes() == yard.tobytes()  # six zeros: the call is unchanged
    assert ga <= 2.0 * ya and gf <= 2.0 * yf, (ga, gf, ya, yf)
    assert ma > 10.0 * ya, (ma, ya)
