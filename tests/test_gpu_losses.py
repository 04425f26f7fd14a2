"""GPU tests of the robust losses soft_l1, cauchy and arctan (PTZBA_LOSS_SOFT_L1 / _CAUCHY / _ARCTAN) through every
layer that takes a loss: K1 (k_linearize) one step against the dense fp64 reference on the crafted problems, its cost
terms on a small-residual case, converged solves on contaminated synthetic problems, the covariance blocks and residual
scale, the marginal, the pose refinement and the Python surface.

Reference: tests/loss_ref.py (pinned to scipy by test_loss_cpu.py).  Gates are the project's own for the same chains:
test_gpu_k1_paths.py's (fp64 cost 1e-10, step 1e-7; fp32 cost 2e-6, step 2e-3, |delta|^2 4e-3, max |gradient| 10x the
float32 rounding of the reference), test_gpu_ba.py's 1e-6 deg / 1e-4 px (fp64) and 1e-4 (fp32), test_gpu_covariance.py's
TOL, test_gpu_marginal.py's STEP_TOL / COST_TOL, test_gpu_reloc.py's 1e-6 deg / 1e-4 px / 1e-7 cost.  Every case prints
its measured errors (DESIGN records the worst)."""
import functools

import numpy as np
import pytest

import k1_cases as kc
import loss_ref
from conftest import golden
from test_gpu_covariance import TOL
from test_gpu_marginal import COST_TOL, STEP_TOL, marg_err

pytestmark = pytest.mark.gpu

IDS = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}
# loss, curvature setting hc, f_scale
SETTINGS = {"soft_l1_s1_c1": ("soft_l1", 1.0, 1.0), "cauchy_s1_c1": ("cauchy", 1.0, 1.0),
            "cauchy_s2.5_c0.1": ("cauchy", 0.1, 2.5), "arctan_s2.5_c0.1": ("arctan", 0.1, 2.5),
            "soft_l1_s2.5_c0.1": ("soft_l1", 0.1, 2.5)}
_cache = {}


def _lin(weighted, setting, round32=False):
    """The reference linearisation at x0, computed once per case family and never modified."""
    k = ("lin", weighted, setting, round32)
    if k not in _cache:
        loss, hcurv, f_scale = SETTINGS[setting]
        _cache[k] = loss_ref.linearise(kc.craft(weighted=weighted), loss, hcurv, f_scale, round32=round32)
    return _cache[k]


def _open(p, precision, loss, hcurv, f_scale, paths=True):
    """set_problem + the k1_info assertions of test_gpu_k1_paths.py + set_state + curvature + linearize."""
    import ptzba
    u, v, ptz0, rays0, frame, landmark, xy, weight = p
    h = ptzba.BAHandle(0)
    h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, weight=weight, precision=precision,
                  loss=IDS[loss], f_scale=f_scale)
    info = h.k1_info()
    if paths:
        assert info[0] == len(rays0) and info[1] == (info[0] + 3) // 4
        assert 1 <= info[2] < info[1], info  # at least one workgroup on either frame-table path
        assert info[3] >= 4, info            # a landmark walked in >= 4 windows
    h.set_state(ptz0, rays0)
    if loss != "linear":
        h.set_huber_curvature(hcurv)
    h.linearize()
    return h, info


def _step(h, lam):
    h.build_reduced(lam)
    h.solve_reduced()
    s = h.read_scalars()
    assert s[5] == 0
    return s


def _rel(a, b):
    return abs(a - b) / abs(b)


def _delta(ptz1, rays1, ptz0, rays0):
    return np.concatenate([(ptz1 - ptz0)[1:].reshape(-1), (rays1 - rays0).reshape(-1)])


def _step_errors(dx_gpu, ref):
    nf = ref["n_free_pose"]
    kg, kr = kc.split_kinds(dx_gpu, nf), kc.split_kinds(ref["dx"], nf)
    err = {k: float(np.abs(kg[k] - kr[k]).max() / np.abs(kr[k]).max()) for k in kr}
    err["all"] = float(np.abs(dx_gpu - ref["dx"]).max() / np.abs(ref["dx"]).max())
    return err


# ------------------------------------------------------------------------------------------------ A
def test_new_losses_are_accepted(gpu_available):
    """set_problem with each new loss id succeeds and linearize() returns a finite cost; id 5 is refused; a robust
    loss needs f_scale > 0."""
    import ptzba
    assert (ptzba.LOSS_SOFT_L1, ptzba.LOSS_CAUCHY, ptzba.LOSS_ARCTAN) == (2, 3, 4)
    p = kc.craft()
    costs = {}
    for loss in loss_ref.SMOOTH:
        h, _ = _open(p, 0, loss, 1.0, 1.0)
        costs[loss] = h.read_scalars()[0]
        h.close()
        assert np.isfinite(costs[loss]) and costs[loss] > 0
    assert len(set(costs.values())) == 3
    h = ptzba.BAHandle(0)
    u, v, ptz0, rays0, frame, landmark, xy, _ = p
    with pytest.raises(ptzba.PtzbaError, match="bad loss 5"):
        h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, loss=5)
    with pytest.raises(ptzba.PtzbaError, match="f_scale"):
        h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, loss=ptzba.LOSS_CAUCHY, f_scale=0.0)
    h.close()


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("precision", [0, 1])
def test_step_matches_fp64_reference(gpu_available, precision, setting, weighted, lam):
    """One (damped) step from x0 on k1_cases.craft(), the scheme of test_gpu_k1_paths.test_step_matches_fp64_reference:
    cost, the step per parameter kind, predicted reduction, |delta|^2 and max |gradient| against the reference; the
    trial cost against the reference cost at the GPU's own trial state."""
    p = kc.craft(weighted=weighted)
    loss, hcurv, f_scale = SETTINGS[setting]
    ref = kc.reference(p, lam, lin=_lin(weighted, setting))
    h, info = _open(p, precision, loss, hcurv, f_scale)
    s = _step(h, lam)
    h.accept(True)
    ptz1, rays1 = h.get_state()
    h.close()
    err = _step_errors(_delta(ptz1, rays1, p[2], p[3]), ref)
    e_cost = _rel(s[0], ref["cost"])
    e_trial = _rel(s[1], loss_ref.cost_at(p, ptz1, rays1, loss, f_scale))
    e_pred, e_dx2, e_g = _rel(s[2], ref["pred"]), _rel(s[3], ref["dx2"]), _rel(s[6], ref["gmax"])
    g64, g32 = ref["gmax"], _lin(weighted, setting, round32=True)["gmax"]
    g_gate = 1e-7 if precision == 0 else max(10.0 * abs(g32 - g64) / g64, 1e-6)
    print(f"LOSSES step precision={precision} setting={setting} weighted={weighted} lam={lam} k1_info={info} "
          f"cost={e_cost:.3e} trial_cost={e_trial:.3e} dx={ {k: f'{x:.3e}' for k, x in err.items()} } pred={e_pred:.3e} "
          f"dx2={e_dx2:.3e} gmax={e_g:.3e} gmax_gate={g_gate:.3e}")
    c_tol, d_tol, d2_tol = (1e-10, 1e-7, 1e-7) if precision == 0 else (2e-6, 2e-3, 4e-3)
    assert e_cost <= c_tol and e_trial <= c_tol, (e_cost, e_trial)
    assert max(err.values()) <= d_tol, err
    assert e_pred <= d_tol and e_dx2 <= d2_tol, (e_pred, e_dx2)
    assert e_g <= g_gate, (e_g, g_gate)


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("loss", loss_ref.SMOOTH + ("linear",))
@pytest.mark.parametrize("precision", [0, 1])
def test_small_residual_cost(gpu_available, precision, loss):
    """Residuals ~0.005 px at f_scale 2.5 (every z << 1, where the direct float32 forms of log(1 + z) and
    sqrt(1 + z) - 1 miss the cost by 2.8e-4 / 1.5e-2: test_loss_cpu.py): the cost after linearize() and the trial cost
    after one lambda = 1e-2 step against loss_ref, fp64 1e-10, fp32 2e-6.  The linear loss runs on the same case and
    meets the same gates: the case is fair."""
    p = loss_ref.small_residual_case()
    fs = 2.5
    h, _ = _open(p, precision, loss, 1.0, fs)
    c0 = h.read_scalars()[0]
    s = _step(h, 1e-2)
    h.accept(True)
    ptz1, rays1 = h.get_state()
    h.close()
    e_cost = _rel(c0, loss_ref.cost_at(p, p[2], p[3], loss, fs))
    e_trial = _rel(s[1], loss_ref.cost_at(p, ptz1, rays1, loss, fs))
    print(f"LOSSES small residuals precision={precision} loss={loss}: cost={e_cost:.3e} trial_cost={e_trial:.3e}")
    tol = 1e-10 if precision == 0 else 2e-6
    assert s[0] == c0
    assert e_cost <= tol and e_trial <= tol, (e_cost, e_trial)


# ------------------------------------------------------------------------------------------------ D
def _handle(p, precision, loss, f_scale=1.0, state=None):
    import ptzba
    h = ptzba.BAHandle(0)
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, precision=precision, loss=IDS[loss],
                  f_scale=f_scale)
    ptz, rays = state if state is not None else (p.init_ptz, p.init_rays)
    h.set_state(ptz, rays)
    return h


def _dist(ptz, rays, ptz_ref, rays_ref):
    """(max |pan, tilt, ray| difference in deg, max |f| difference in px)."""
    d = np.abs(ptz - ptz_ref)
    return float(max(d[:, :2].max(), np.abs(rays - rays_ref).max())), float(d[:, 2].max())


def _robust_differs_from_linear(cfg, name, ang, fpx):
    _, ptz_l, rays_l, _ = loss_ref.point(cfg + "_linear")
    _, ptz_r, rays_r, _ = loss_ref.point(name)
    da, df = _dist(ptz_r, rays_r, ptz_l, rays_l)
    print(f"{name} vs the linear-loss optimum: {da:.3e} deg, {df:.3e} px")
    assert da > 100 * ang and df > 100 * fpx, (da, df)


def test_solve_fp64_config1(gpu_available):
    """Config 1 with 10 % of the records 8 px off, fp64, Cauchy f_scale 1: the device loop, the host loop, ptzba_solve
    and ptzba_solve_resident take the same trial sequence (equal iteration and evaluation counts and status, cost to 1e-12,
    final state to 1e-10, as test_gpu_ba.test_device_loop_equals_host_loop) and end within 1e-6 deg / 1e-4 px of the recorded stationary
    point; soft_l1 through ptzba_solve."""
    import ptzba
    golden(loss_ref.GOLDEN)
    p, ptz_ref, rays_ref, c_ref = loss_ref.point("c1_cauchy")
    _robust_differs_from_linear("c1", "c1_cauchy", 1e-6, 1e-4)
    _robust_differs_from_linear("c1", "c1_soft_l1", 1e-6, 1e-4)
    kw = dict(ftol=1e-14, xtol=1e-14, max_iter=200)
    out = {}
    for device_loop in (True, False):
        h = _handle(p, 0, "cauchy")
        res = ptzba.LMSolver(h, device_loop=device_loop, **kw).run()
        out["device" if device_loop else "host"] = (res,) + h.get_state()
        h.close()
    h = _handle(p, 0, "cauchy")
    ptz, rays, res = h.solve(p.init_ptz, p.init_rays, **kw)
    out["solve"] = (res, ptz, rays)
    h.set_state(p.init_ptz, p.init_rays)
    h.save_state()
    res = h.solve_resident(restore=True, **kw)
    out["resident"] = (res,) + h.get_state()
    h.close()
    r0, ptz0, rays0 = out["device"]
    for k, (r, ptz, rays) in out.items():
        da, df = _dist(ptz, rays, ptz_ref, rays_ref)
        print(f"LOSSES solve config1 fp64 cauchy {k}: {r}; vs the recorded point {da:.3e} deg {df:.3e} px; cost "
              f"{_rel(r.cost, c_ref):.3e}")
        assert (r.njev, r.nfev, r.status) == (r0.njev, r0.nfev, r0.status), (k, r, r0)
        assert abs(r.cost - r0.cost) <= 1e-12 * r0.cost
        np.testing.assert_allclose(ptz, ptz0, rtol=0, atol=1e-10)
        np.testing.assert_allclose(rays, rays0, rtol=0, atol=1e-10)
        assert r.status > 0 and da <= 1e-6 and df <= 1e-4, (k, da, df)
        assert _rel(r.cost, c_ref) <= 1e-9
    p, ptz_ref, rays_ref, c_ref = loss_ref.point("c1_soft_l1")
    h = _handle(p, 0, "soft_l1")
    ptz, rays, r = h.solve(p.init_ptz, p.init_rays, **kw)
    h.close()
    da, df = _dist(ptz, rays, ptz_ref, rays_ref)
    print(f"LOSSES solve config1 fp64 soft_l1 solve: {r}; vs the recorded point {da:.3e} deg {df:.3e} px")
    assert r.status > 0 and da <= 1e-6 and df <= 1e-4, (da, df)


def _pose_dist(ptz, ptz_ref):
    """(pan / tilt RMSE in deg, f RMSE in px): synthetic.pose_rmse, the metric of the project's fp32 gate (1e-4)."""
    import synthetic
    r = synthetic.pose_rmse(ptz, ptz_ref)
    return float(max(r[0], r[1])), float(r[2])


def test_solve_fp32_config2(gpu_available):
    """Config 2 with 10 % of the records 8 px off, fp32, plain IRLS (huber_curvature=1, as
    test_gpu_ray_priors.test_converged_solve_config2_fp32_huber): Cauchy ends within 1e-4 deg / 1e-4 px (pose RMSE, the
    project's fp32 gate) of its recorded stationary point.  Huber on the same problem against its own recorded point is
    the yardstick: where Huber itself stops further than 1e-4 away, the Cauchy gate is twice Huber's distance (the two
    trial sequences differ; the fp32 acceptance noise is the known limit); the same rule gates the largest single
    difference over poses and rays.  Started at the recorded point, the fp32
    solve stays within 1e-4 px."""
    golden(loss_ref.GOLDEN)
    _robust_differs_from_linear("c2", "c2_cauchy", 1e-4, 1e-4)
    kw = dict(ftol=1e-12, xtol=1e-12, max_iter=100, huber_curvature=1.0)
    dist, worst = {}, {}
    for loss in ("huber", "cauchy"):
        p, ptz_ref, rays_ref, c_ref = loss_ref.point("c2_" + loss)
        h = _handle(p, 1, loss)
        ptz, rays, r = h.solve(p.init_ptz, p.init_rays, **kw)
        dist[loss] = _pose_dist(ptz, ptz_ref)
        worst[loss] = _dist(ptz, rays, ptz_ref, rays_ref)
        print(f"LOSSES solve config2 fp32 {loss}: {r}; pose RMSE vs the recorded point {dist[loss][0]:.3e} deg "
              f"{dist[loss][1]:.3e} px; max {worst[loss]}; cost {_rel(r.cost, c_ref):.3e}")
        if loss == "cauchy":
            ptz, rays, r = h.solve(ptz_ref, rays_ref, **kw)
            stay = _dist(ptz, rays, ptz_ref, rays_ref)
            print(f"LOSSES solve config2 fp32 cauchy from the recorded point: {r}; max {stay[0]:.3e} deg {stay[1]:.3e} px")
        h.close()
    gate = [1e-4 if d <= 1e-4 else 2.0 * d for d in dist["huber"]]
    print(f"LOSSES solve config2 fp32 gates: {gate[0]:.3e} deg {gate[1]:.3e} px")
    assert dist["cauchy"][0] <= gate[0] and dist["cauchy"][1] <= gate[1], (dist, gate)
    # the largest single difference (poses and rays): 1e-4, or twice Huber's where Huber stops further away
    wgate = [1e-4 if d <= 1e-4 else 2.0 * d for d in worst["huber"]]
    print(f"LOSSES solve config2 fp32 largest single difference gates: {wgate[0]:.3e} deg {wgate[1]:.3e} px")
    assert worst["cauchy"][0] <= wgate[0] and worst["cauchy"][1] <= wgate[1], (worst, wgate)
    assert stay[0] <= 1e-4 and stay[1] <= 1e-4, stay


# ------------------------------------------------------------------------------------------------ E
@functools.lru_cache(maxsize=None)
def _cov_reference():
    import cov_ref
    p, ptz, rays, _ = loss_ref.point("c1_cauchy")
    H = loss_ref.normal_matrix(p, ptz, rays, "cauchy", 1.0)
    pose, ray = cov_ref._cut(np.linalg.inv(H), p.n_pose, p.n_landmark, 1)
    _, r, _, w1, _ = loss_ref.records(p, ptz, rays, "cauchy", 1.0)
    n_free = 3 * (p.n_pose - 1) + 2 * p.n_landmark
    return pose, ray, float(np.sum(w1 * r * r)) / (len(r) - n_free), n_free


@pytest.mark.parametrize("precision", [0, 1])
def test_covariance_at_cauchy_optimum(gpu_available, precision):
    """At config 1's recorded Cauchy point: pose and ray blocks against inv(J^T diag(rho') J) at test_gpu_covariance.py's
    gates, whatever curvature was set; scale="residual" against sum rho' r^2 / (2 R - n_free) to 1e-9 in either
    precision (the kernel sums in fp64; fp32 rounds the records' residuals only)."""
    import cov_ref
    golden(loss_ref.GOLDEN)
    p, ptz, rays, _ = loss_ref.point("c1_cauchy")
    pose_ref, ray_ref, s2, n_free = _cov_reference()
    h = _handle(p, precision, "cauchy", state=(ptz, rays))
    h.set_huber_curvature(0.1)
    pose, ray, info = h.covariance("all")
    pose_s, ray_s, info_s = h.covariance("all", scale="residual")
    h.close()
    ep, er = cov_ref.block_err(pose, pose_ref), cov_ref.block_err(ray, ray_ref)
    e_s = _rel(info_s["scale"], s2)
    eps, ers = cov_ref.block_err(pose_s, s2 * pose_ref), cov_ref.block_err(ray_s, s2 * ray_ref)
    print(f"LOSSES covariance precision={precision}: pose {ep:.3e} ray {er:.3e} (tol {TOL[precision]:.0e}); residual "
          f"scale {info_s['scale']:.6e} vs {s2:.6e}: {e_s:.3e}; scaled blocks pose {eps:.3e} ray {ers:.3e}")
    assert info["scale"] == 1.0 and info["n_free"] == n_free
    assert ep <= TOL[precision] and er <= TOL[precision], (ep, er)
    assert e_s <= 1e-9, e_s
    assert eps <= TOL[precision] and ers <= TOL[precision], (eps, ers)


# ------------------------------------------------------------------------------------------------ F
def test_marginal_with_cauchy(gpu_available):
    """Config 1, Cauchy, fp64, marginal_prior([1]) at x0: info, grad and offset against the dense formula with the rows
    scaled by sqrt(rho') and offset 1/2 f^2 sum rho over the dropped records (test_gpu_marginal.py's gates); a solve
    started after the call is bitwise the solve without it."""
    import ptzba
    p = loss_ref.contaminated("config1")
    ref = loss_ref.marginal(p, p.init_ptz, p.init_rays, [1], "cauchy", 1.0)
    out = []
    for with_call in (False, True):
        h = _handle(p, 0, "cauchy")
        if with_call:
            got, stats = h.marginal_prior([1])
        res = ptzba.LMSolver(h, ftol=1e-8, xtol=1e-12, max_iter=40).run()
        ptz, rays = h.get_state()
        h.close()
        out.append((ptz.tobytes(), rays.tobytes(), res.njev, res.nfev, res.status, res.cost))
    assert got.frames.tolist() == ref.frames.tolist()
    np.testing.assert_array_equal(got.lin, ref.lin)
    e_info, e_grad = marg_err(got, ref)
    e_off = _rel(got.offset, ref.offset)
    print(f"LOSSES marginal config1 cauchy E=[1]: Lambda {e_info:.3e} eta {e_grad:.3e} offset {e_off:.3e}; {stats}")
    assert stats["dropped_records"] == int((ptzba.drop_mask(p.frame, [1]) != 0).sum()) and stats["min_pivot"] > 0
    assert e_info < STEP_TOL[0] and e_grad < STEP_TOL[0], (e_info, e_grad)
    assert e_off <= COST_TOL[0], e_off
    assert out[0][2] > 1 and out[0] == out[1], (out[0][2:], out[1][2:])


# ------------------------------------------------------------------------------------------------ G
@functools.lru_cache(maxsize=None)
def _reloc_references():
    """Per subset the linear-loss scipy optimum (the start) and, per loss, scipy's trf from that start polished by
    loss_ref.reloc_polish (the polish must move scipy's x by less than 1e-4 deg / 1e-2 px)."""
    from scipy.optimize import least_squares
    from oracle import ptz_oracle as orc
    d = golden("reloc.npz")
    u, v = float(d["u"]), float(d["v"])
    rng = np.random.default_rng(1)
    n = len(d["rays"])
    subsets = [rng.choice(n, 32, replace=False) for _ in range(16)]
    kw = dict(x_scale='jac', ftol=1e-15, xtol=1e-15, gtol=1e-15, method='trf')
    starts, refs = [], {loss: [] for loss in loss_ref.SMOOTH}
    for s in subsets:
        args = (d["rays"][s], d["points"][s], u, v)
        x0 = least_squares(orc.reloc_residual, d["pose0"], args=args, **kw).x
        starts.append(x0)
        for loss in loss_ref.SMOOTH:
            r = least_squares(orc.reloc_residual, x0, loss=loss, f_scale=1.0, args=args, **kw)
            assert r.status in (2, 3), (loss, r.status)
            x, c, g = loss_ref.reloc_polish(r.x, *args, loss, 1.0)
            moved = np.abs(x - r.x)
            assert moved[:2].max() < 1e-4 and moved[2] < 1e-2 and g < 1e-9, (loss, moved, g)
            assert c <= r.cost * (1 + 1e-12)
            refs[loss].append((x, c, float(np.max(np.abs(x - x0) / np.array([1e-6, 1e-6, 1e-4])))))
    return d, u, v, subsets, np.array(starts), refs


@pytest.mark.parametrize("loss", loss_ref.SMOOTH)
def test_pose_refinement(gpu_available, loss):
    """reloc.npz, 16 subsets of 32 correspondences, f_scale 1, from each subset's linear-loss optimum: the refined poses
    against scipy's (polished) optimum of the loss, test_gpu_reloc.py's gates 1e-6 deg / 1e-4 px / cost 1e-7."""
    import ptzba
    d, u, v, subsets, starts, refs = _reloc_references()
    ptz, cost, its, st = ptzba.refine_poses(u, v, starts, d["rays"], d["points"], subsets=subsets, ftol=1e-14,
                                            xtol=1e-14, loss=IDS[loss], f_scale=1.0)
    worst = [0.0, 0.0, 0.0]
    for k, (x, c, moved) in enumerate(refs[loss]):
        assert moved > 10.0, moved  # the start (the linear-loss optimum) is more than 10 gates from the robust one
        e = np.abs(ptz[k] - x)
        worst = [max(worst[0], float(e[:2].max())), max(worst[1], float(e[2])), max(worst[2], _rel(cost[k], c))]
    print(f"LOSSES pose refinement {loss}: {worst[0]:.3e} deg {worst[1]:.3e} px cost {worst[2]:.3e}")
    assert worst[0] < 1e-6 and worst[1] < 1e-4 and worst[2] <= 1e-7, worst
    with pytest.raises(ptzba.PtzbaError, match="bad loss"):
        ptzba.refine_poses(u, v, starts, d["rays"], d["points"], subsets=subsets, loss=5)


# ------------------------------------------------------------------------------------------------ H
def test_python_surface(gpu_available):
    """Names and ids are interchangeable in BAHandle.set_problem, ptzba.solve and refine_poses; an unknown name raises
    ValueError from set_problem and from bundle_adjustment (which used to run the linear loss silently)."""
    import bundle_adjustment as ba
    import ptzba
    assert ptzba.LOSS_IDS == IDS
    p = loss_ref.contaminated("config1")
    for name, lid in IDS.items():
        cost = []
        for loss in (name, lid):
            h = ptzba.BAHandle(0)
            h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, loss=loss, f_scale=1.5)
            assert h.loss == lid
            h.set_state(p.init_ptz, p.init_rays)
            h.linearize()
            cost.append(h.read_scalars()[0])
            h.close()
        assert cost[0] == cost[1]
    a = ptzba.solve(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, p.init_ptz, p.init_rays,
                    loss="soft_l1", max_iter=3, keep_handle=False)
    b = ptzba.solve(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, p.init_ptz, p.init_rays,
                    loss=ptzba.LOSS_SOFT_L1, max_iter=3, keep_handle=False)
    assert a[0].tobytes() == b[0].tobytes() and a[2].cost == b[2].cost
    d = golden("reloc.npz")
    u, v = float(d["u"]), float(d["v"])
    ra = ptzba.refine_poses(u, v, d["pose0"][None], d["rays"], d["points"], loss="arctan")
    rb = ptzba.refine_poses(u, v, d["pose0"][None], d["rays"], d["points"], loss=ptzba.LOSS_ARCTAN)
    assert ra[0].tobytes() == rb[0].tobytes() and ra[1][0] == rb[1][0]
    h = ptzba.BAHandle(0)
    with pytest.raises(ValueError, match="unknown loss"):
        h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, loss="tukey")
    h.close()
    with pytest.raises(ValueError, match="unknown loss"):
        ptzba.refine_poses(u, v, d["pose0"][None], d["rays"], d["points"], loss="tukey")
    with pytest.raises(ValueError, match="unknown loss"):
        ba.bundle_adjustment([np.zeros((4, 4, 3), np.uint8)], [0], "sift", np.array([[50.0, -10.0, 3000.0]]),
                             np.zeros(3), np.eye(3), 640.0, 360.0, "", loss="tukey")
