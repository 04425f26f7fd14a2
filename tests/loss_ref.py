"""CPU reference of the robust losses soft_l1, cauchy and arctan (shared by test_loss_cpu.py and test_gpu_losses.py).
The oracle's _loss_weights knows linear and huber only, so the new losses' rho functions live here, on top of
orc.ba_jacobian, orc.compute_residual_records and orc.reloc_residual.

Per scalar residual r, z = (r / f_scale)^2 (scipy least_squares' convention; csrc/robust_loss.h on the device):

    loss      rho(z)               w1 = rho'       Newton curvature wn = rho' + 2 z rho''
    soft_l1   2 (sqrt(1+z) - 1)    (1+z)^-1/2      (1+z)^-3/2
    cauchy    ln(1+z)              1 / (1+z)       (1 - z) / (1+z)^2
    arctan    atan z               1 / (1+z^2)     (1 - 3 z^2) / (1+z^2)^2

cost = 1/2 f_scale^2 sum w rho(z); gradient weight w1; curvature weight w2 = max(wn, hc w1), hc the library's
"huber curvature" setting (1: IRLS, because rho'' <= 0).  linear and huber are k1_cases._weights' (huber: the same
rule, its Newton curvature being 1 inside the unit and 0 beyond it)."""
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_ROOT, "pan-tilt-zoom-slam_amd"), _ROOT):  # (`python tests/loss_ref.py`: no conftest)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import k1_cases as kc  # noqa: E402
from oracle import ptz_oracle as orc  # noqa: E402

SMOOTH = ("soft_l1", "cauchy", "arctan")
GOLDEN = "loss_points.npz"


def rho_all(z, loss):
    """(rho, rho', rho' + 2 z rho'') at z >= 0, fp64, accurate relative to each value for z << 1."""
    z = np.asarray(z, np.float64)
    if loss == "soft_l1":
        t = 1.0 + z
        s = np.sqrt(t)
        return 2.0 * z / (s + 1.0), 1.0 / s, 1.0 / (t * s)
    if loss == "cauchy":
        t = 1.0 + z
        return np.log1p(z), 1.0 / t, (1.0 - z) / (t * t)
    if loss == "arctan":
        t = 1.0 + z * z
        return np.arctan(z), 1.0 / t, (1.0 - 3.0 * z * z) / (t * t)
    raise ValueError(loss)


def weights(r, loss, hcurv, f_scale):
    """(z, rho, w1, w2) per scalar residual: k1_cases._weights extended by the smooth losses."""
    if loss in ("linear", "huber"):
        return kc._weights(r, loss, hcurv, f_scale)
    z = (r / f_scale) ** 2
    rho, w1, wn = rho_all(z, loss)
    return z, rho, w1, np.maximum(wn, hcurv * w1)


def rho32(z, loss, naive):
    """rho(z) evaluated in numpy float32: the direct forms (naive) or the ones the kernels use."""
    z = np.asarray(z, np.float32)
    one = np.float32(1.0)
    if loss == "soft_l1":
        s = np.sqrt(one + z)
        return np.float32(2.0) * (s - one) if naive else np.float32(2.0) * z / (s + one)
    if loss == "cauchy":
        return np.log(one + z) if naive else np.log1p(z)
    if loss == "arctan":
        return np.arctan(z)
    assert loss == "linear"
    return z


def cost32(r, loss, f_scale, naive):
    """1/2 f_scale^2 sum rho, the terms formed in float32 from the float32-rounded residuals, summed in fp64."""
    r = np.asarray(r, np.float32)
    z = r * r * np.float32(1.0 / (f_scale * f_scale))
    t = rho32(z, loss, naive)
    assert t.dtype == np.float32
    return 0.5 * f_scale ** 2 * float(np.sum(t.astype(np.float64)))


# ------------------------------------------------------------------------------------------------
# the crafted K1 problems (k1_cases' tuple form)
# ------------------------------------------------------------------------------------------------
def residual(problem, ptz=None, rays=None):
    u, v, ptz0, rays0, frame, landmark, xy, weight = problem
    ptz = ptz0 if ptz is None else ptz
    rays = rays0 if rays is None else rays
    return orc.compute_residual_records(np.concatenate([ptz.reshape(-1), rays.reshape(-1)]), len(ptz), u, v,
                                        frame.astype(np.int64), landmark.astype(np.int64), xy)


def cost_at(problem, ptz, rays, loss, f_scale):
    """k1_cases.cost_at for every loss."""
    r = residual(problem, ptz, rays)
    weight = problem[7]
    w = np.ones(len(r)) if weight is None else np.repeat(weight, 2)
    return 0.5 * f_scale ** 2 * float(np.sum(w * weights(r, loss, 1.0, f_scale)[1]))


def linearise(problem, loss, hcurv, f_scale, ptz=None, rays=None, round32=False):
    """k1_cases.linearise for every loss (the same dict; k1_cases.reference(lin=...) takes it)."""
    u, v, ptz0, rays0, frame, landmark, xy, weight = problem
    ptz = ptz0 if ptz is None else ptz
    rays = rays0 if rays is None else rays
    n_pose, n_lm = len(ptz), len(rays)
    fr, lm = frame.astype(np.int64), landmark.astype(np.int64)
    x = np.concatenate([ptz[1:].reshape(-1), rays.reshape(-1)])
    J = orc.ba_jacobian(x, n_pose, n_lm, u, v, ptz[0], fr, lm).tocsr()
    r = orc.compute_residual_records(np.concatenate([ptz[0], x]), n_pose, u, v, fr, lm, xy)
    w = np.ones(len(r)) if weight is None else np.repeat(weight, 2)
    z, rho, w1, w2 = weights(r, loss, hcurv, f_scale)
    cost = 0.5 * f_scale ** 2 * float(np.sum(w * rho))
    if round32:
        J = J.astype(np.float32).astype(np.float64)
        r = r.astype(np.float32).astype(np.float64)
    H = (J.T @ J.multiply((w * w2)[:, None])).toarray()
    g = J.T @ (w * w1 * r)
    return dict(cost=cost, H=H, g=g, z=z, gmax=float(np.abs(g).max()), n_free_pose=n_pose - 1)


def negative_curvature_share(problem, loss, f_scale):
    """Share of the scalar residuals at x0 whose Newton curvature is negative (w2 takes the hc rho' branch)."""
    r = residual(problem)
    return float(np.mean(rho_all((r / f_scale) ** 2, loss)[2] < 0.0))


@functools.lru_cache(maxsize=None)
def small_residual_case(weighted=False, sigma=0.005, seed=11):
    """k1_cases.craft() with the observations replaced by the projection at (ptz0, rays0) plus N(0, sigma px) noise:
    every z << 1 at f_scale 2.5, where log(1 + z) and sqrt(1 + z) - 1 lose their digits in float32."""
    u, v, ptz0, rays0, frame, landmark, xy, weight = kc.craft(weighted=weighted)
    px, py = orc.from_ray_to_image(u, v, ptz0[frame, 2], ptz0[frame, 0], ptz0[frame, 1], rays0[landmark, 0],
                                   rays0[landmark, 1])
    rng = np.random.default_rng(seed)
    xy = np.stack([px, py], -1) + rng.normal(0.0, sigma, (len(frame), 2))
    return u, v, ptz0, rays0, frame, landmark, xy, weight


# ------------------------------------------------------------------------------------------------
# synthetic problems (synthetic.make_problem's object form): contaminated records, stationary points
# ------------------------------------------------------------------------------------------------
class Problem:
    """The fields of a synthetic problem the references read, with its own xy."""

    def __init__(self, p, xy):
        self.n_pose, self.n_landmark, self.u, self.v = p.n_pose, p.n_landmark, p.u, p.v
        self.frame, self.landmark, self.xy = p.frame, p.landmark, xy
        self.init_ptz, self.init_rays = p.init_ptz, p.init_rays


@functools.lru_cache(maxsize=None)
def contaminated(cfg, share=0.1, offset=8.0, seed=3):
    """synthetic.make_problem(cfg, seed=0) with `share` of its records (seeded) moved `offset` px off in x and y."""
    import synthetic
    p = synthetic.make_problem(cfg, seed=0)
    rng = np.random.default_rng(seed)
    xy = np.array(p.xy, np.float64)
    out = rng.random(len(xy)) < share
    xy[out] += offset * rng.choice([-1.0, 1.0], (int(out.sum()), 2))
    xy.setflags(write=False)
    return Problem(p, xy)


def records(p, ptz, rays, loss, f_scale, hcurv=1.0):
    """(J sparse over the free parameters, r, rho, w1, w2) of problem p at (ptz, rays)."""
    ptz = np.asarray(ptz, np.float64)
    rays = np.asarray(rays, np.float64)
    fr, lm = p.frame.astype(np.int64), p.landmark.astype(np.int64)
    x = np.concatenate([ptz[1:].reshape(-1), rays.reshape(-1)])
    J = orc.ba_jacobian(x, p.n_pose, p.n_landmark, p.u, p.v, ptz[0], fr, lm).tocsr()
    r = orc.compute_residual_records(np.concatenate([ptz[0], x]), p.n_pose, p.u, p.v, fr, lm, p.xy)
    _, rho, w1, w2 = weights(r, loss, hcurv, f_scale)
    return J, r, rho, w1, w2


def cost(p, ptz, rays, loss, f_scale):
    ptz = np.asarray(ptz, np.float64)
    rays = np.asarray(rays, np.float64)
    r = orc.compute_residual_records(np.concatenate([ptz.reshape(-1), rays.reshape(-1)]), p.n_pose, p.u, p.v,
                                     p.frame.astype(np.int64), p.landmark.astype(np.int64), p.xy)
    return 0.5 * f_scale ** 2 * float(np.sum(weights(r, loss, 1.0, f_scale)[1]))


def normal_matrix(p, ptz, rays, loss, f_scale):
    """Dense J^T diag(rho') J over [free poses | rays] (cov_ref.normal_matrix for every loss)."""
    import scipy.sparse as sp
    J, _, _, w1, _ = records(p, ptz, rays, loss, f_scale)
    Jw = sp.diags(np.sqrt(w1)) @ J
    return np.asarray((Jw.T @ Jw).todense())


def stationarity(p, ptz, rays, loss, f_scale):
    """max over the free parameters of |gradient entry| / (the magnitude of the terms it sums)."""
    J, r, _, w1, _ = records(p, ptz, rays, loss, f_scale)
    g = np.asarray(J.T @ (w1 * r)).reshape(-1)
    mag = np.asarray(abs(J).T @ np.abs(w1 * r)).reshape(-1) + 1e-300
    return float(np.max(np.abs(g) / mag))


def split(p, x):
    k = 3 * (p.n_pose - 1)
    return np.concatenate([np.zeros((1, 3)), x[:k].reshape(-1, 3)]), x[k:].reshape(-1, 2)


def solve(p, ptz0, rays0, loss, f_scale, max_iter=200, hcurv=0.1, gtol=1e-9):
    """Floored-Newton iteration (w2 = max(wn, hcurv rho'), a sparse solve per step) with step halving to the
    stationary point: stops after a full step below 1e-10 (deg; 1e-7 px of focal length) and checks the gradient there.
    Returns (ptz, rays, cost)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    ptz = np.array(ptz0, np.float64)
    rays = np.array(rays0, np.float64)
    c = cost(p, ptz, rays, loss, f_scale)
    for _ in range(max_iter):
        J, r, _, w1, w2 = records(p, ptz, rays, loss, f_scale, hcurv)
        Jw = sp.diags(np.sqrt(w2)) @ J
        dx = spla.spsolve((Jw.T @ Jw).tocsc(), -np.asarray(J.T @ (w1 * r)).reshape(-1))
        dptz, drays = split(p, dx)
        t = 1.0
        while True:
            c1 = cost(p, ptz + t * dptz, rays + t * drays, loss, f_scale)
            if c1 <= c + 1e-12 * abs(c) or t < 1e-6:
                break
            t *= 0.5
        ptz, rays, c = ptz + t * dptz, rays + t * drays, min(c, c1)
        if t == 1.0 and np.abs(dptz / np.array([1.0, 1.0, 1e3])).max() < 1e-10 and np.abs(drays).max() < 1e-10:
            break
    s = stationarity(p, ptz, rays, loss, f_scale)
    assert s < gtol, s
    return ptz, rays, c


class DenseHandle:
    """The handle protocol of ptzba.LMSolver's host loop (linearize / build_reduced / solve_reduced / read_scalars /
    accept / set_huber_curvature) in sparse fp64 numpy for every loss: H = J^T diag(w2) J, g = J^T (w1 r),
    D = max(D, diag H, 1e-12) remembered across steps, dx = solve(H + lam diag D, -g).  LMSolver(DenseHandle(...),
    device_loop=False) is the library's own LM -- its acceptance, damping and curvature-switch rules -- on the
    reference's numbers."""

    def __init__(self, p, loss, f_scale):
        self.p, self.loss_name, self.f_scale, self.hcurv = p, loss, f_scale, 1.0
        self.loss = 0 if loss == "linear" else 1  # (LMSolver: any non-linear id is a robust loss)
        assert len(np.unique(p.landmark)) == p.n_landmark and len(np.unique(p.frame)) == p.n_pose

    def set_huber_curvature(self, hc):
        self.hcurv = float(hc)

    def set_state(self, ptz, rays):
        self.ptz, self.rays = np.array(ptz, np.float64), np.array(rays, np.float64)
        self.D = np.zeros(3 * (self.p.n_pose - 1) + 2 * self.p.n_landmark)

    def get_state(self):
        return self.ptz.copy(), self.rays.copy()

    def _lin(self, ptz, rays):
        import scipy.sparse as sp
        J, r, rho, w1, w2 = records(self.p, ptz, rays, self.loss_name, self.f_scale, self.hcurv)
        Jw = sp.diags(np.sqrt(w2)) @ J
        return dict(cost=0.5 * self.f_scale ** 2 * float(np.sum(rho)), H=(Jw.T @ Jw).tocsc(),
                    g=np.asarray(J.T @ (w1 * r)).reshape(-1))

    def linearize(self):
        self.cur = self._lin(self.ptz, self.rays)
        self.s = np.zeros(8)
        self.s[0] = self.cur["cost"]

    def build_reduced(self, lam):
        self.lam = float(lam)

    def solve_reduced(self):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        H, g = self.cur["H"], self.cur["g"]
        self.D = np.maximum(self.D, np.maximum(H.diagonal(), 1e-12))
        dx = spla.spsolve((H + self.lam * sp.diags(self.D)).tocsc(), -g)
        dptz, drays = split(self.p, dx)
        self.trial_state = (self.ptz + dptz, self.rays + drays)
        self.trial = self._lin(*self.trial_state)
        ok = np.all(np.isfinite(dx))
        self.s = np.array([self.cur["cost"], self.trial["cost"],
                           -0.5 * float(g @ dx) + 0.5 * self.lam * float(dx @ (self.D * dx)), float(dx @ dx),
                           float(np.sum(self.ptz ** 2) + np.sum(self.rays ** 2)), 0.0 if ok else 1.0,
                           float(np.abs(g).max()), 0.0])

    def read_scalars(self):
        return self.s.copy()

    def accept(self, ok):
        if ok:
            (self.ptz, self.rays), self.cur = self.trial_state, self.trial

    def sync(self):
        pass


def lm_solve(p, loss, f_scale, huber_curvature=0.1, max_iter=300):
    """The library's LM (ptzba.LMSolver's host loop with its defaults: Gauss-Newton start, IRLS curvature until the
    switch, then huber_curvature) on a DenseHandle from the problem's x0 with tight tolerances, then solve()'s
    floored-Newton polish to the stationary point of that basin.  Returns (ptz, rays, cost, LMResult, how far the
    polish moved the LM's poses and rays)."""
    import ptzba
    h = DenseHandle(p, loss, f_scale)
    h.set_state(p.init_ptz, p.init_rays)
    res = ptzba.LMSolver(h, ftol=1e-14, xtol=1e-14, max_iter=max_iter, device_loop=False,
                         huber_curvature=huber_curvature).run()
    ptz, rays = h.get_state()
    ptz1, rays1, c = solve(p, ptz, rays, loss, f_scale)
    return ptz1, rays1, c, res, (float(np.abs(ptz1 - ptz).max()), float(np.abs(rays1 - rays).max()))


def scipy_solve(p, ptz0, rays0, loss, f_scale, max_nfev=300):
    """scipy's trf with the loss from the same start (tight tolerances, analytic Jacobian).  Returns (ptz, rays, cost)."""
    x0 = np.concatenate([np.asarray(ptz0)[1:].reshape(-1), np.asarray(rays0).reshape(-1)])
    res = orc.solve_scipy(x0, p.n_pose, p.n_landmark, p.u, p.v, np.asarray(ptz0)[0], p.frame.astype(np.int64),
                          p.landmark.astype(np.int64), p.xy, ftol=1e-15, xtol=1e-15, gtol=1e-15, analytic=True,
                          loss=loss, f_scale=f_scale, max_nfev=max_nfev)
    dptz, rays = split(p, res.x)
    dptz[0] = np.asarray(ptz0)[0]
    return dptz, rays, float(res.cost)


# the recorded stationary points of the GPU solve tests: (config, loss, f_scale, curvature setting of the LM that
# found the basin -- config 1: the default 0.1 after the switch, config 2: plain IRLS, as the GPU tests run them)
POINTS = {"c1_linear": ("config1", "linear", 1.0, 0.1), "c1_cauchy": ("config1", "cauchy", 1.0, 0.1),
          "c1_soft_l1": ("config1", "soft_l1", 1.0, 0.1), "c2_cauchy": ("config2", "cauchy", 1.0, 1.0),
          "c2_huber": ("config2", "huber", 1.0, 1.0), "c2_linear": ("config2", "linear", 1.0, 1.0)}


def point(name, path=None):
    """(problem, ptz, rays, cost) of a recorded stationary point (tests/golden/loss_points.npz, written by
    `python tests/loss_ref.py`): the cost is recomputed here against the problem as it is now.  scipy_record(name) has
    the recorded result of scipy's trf from the same start."""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    d = np.load(path, allow_pickle=False)
    cfg, loss, fs, _ = POINTS[name]
    p = contaminated(cfg)
    ptz, rays = d[name + "_ptz"], d[name + "_rays"]
    c = cost(p, ptz, rays, loss, fs)
    assert abs(c - float(d[name + "_cost"])) <= 1e-12 * c
    return p, ptz, rays, c


def scipy_record(name, path=None):
    """(cost, evaluations, status) of scipy's trf from the problem's x0 after at most SCIPY_NFEV evaluations, as
    `python tests/loss_ref.py` recorded it."""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    d = np.load(path, allow_pickle=False)
    return float(d[name + "_scipy_cost"]), int(d[name + "_scipy_nfev"]), int(d[name + "_scipy_status"])


def marginal(p, ptz, rays, E, loss, f_scale):
    """The dense formula of include/ptzba.h's ptzba_marginal_prior for free leaving frames E and no prior factors, rows
    scaled by sqrt(rho'): the dropped records' normal system, their landmarks eliminated, then E; offset
    1/2 f_scale^2 sum rho over the dropped records.  Returns a ptzba.Marginal."""
    import ptzba
    ptz = np.asarray(ptz, np.float64)
    E = [int(f) for f in E]
    assert all(f >= 1 for f in E)
    rec = ptzba.drop_mask(p.frame, E) != 0
    rows = np.repeat(rec, 2)
    J, r, rho, w1, _ = records(p, ptz, rays, loss, f_scale)
    k = 3 * (p.n_pose - 1)
    Jd = np.asarray(J[rows].todense()) * np.sqrt(w1[rows])[:, None]
    H = Jd.T @ Jd
    g = Jd.T @ (np.sqrt(w1[rows]) * r[rows])
    S, b = H[:k, :k].copy(), g[:k].copy()
    for l in np.unique(p.landmark[rec]).astype(np.int64):
        c = slice(k + 2 * l, k + 2 * l + 2)
        Y = H[:k, c] @ np.linalg.inv(H[c, c])
        S -= Y @ H[:k, c].T
        b -= Y @ g[c]
    rows3 = lambda fr: (3 * (np.asarray(fr, np.int64)[:, None] - 1) + np.arange(3)[None, :]).reshape(-1)  # noqa: E731
    K = np.array(sorted(int(f) for f in np.unique(p.frame[rec]) if f >= 1 and f not in E), np.int64)
    iK, iE = rows3(K), rows3(E)
    X = np.linalg.solve(S[np.ix_(iE, iE)], S[np.ix_(iK, iE)].T).T
    Lam = S[np.ix_(iK, iK)] - X @ S[np.ix_(iK, iE)].T
    eta = b[iK] - X @ b[iE]
    off = 0.5 * f_scale ** 2 * float(np.sum(rho[rows]))
    return ptzba.Marginal(K, ptz[K], 0.5 * (Lam + Lam.T), eta, off)


# ------------------------------------------------------------------------------------------------
# pose-only refinement (relocalisation): 3-parameter IRLS polish
# ------------------------------------------------------------------------------------------------
def reloc_cost(pose, rays, points, u, v, loss, f_scale):
    r = orc.reloc_residual(pose, rays, points, u, v)
    return 0.5 * f_scale ** 2 * float(np.sum(weights(r, loss, 1.0, f_scale)[1]))


def reloc_polish(pose, rays, points, u, v, loss, f_scale, max_iter=200):
    """Floored-Newton iteration on (pan, tilt, f) with step halving from `pose` until the step is below 1e-12 deg /
    1e-9 px.  Returns (pose, cost, relative gradient)."""
    pose = np.array(pose, np.float64)
    rays = np.asarray(rays, np.float64).reshape(-1, 2)
    c = reloc_cost(pose, rays, points, u, v, loss, f_scale)
    for _ in range(max_iter):
        J = orc.record_jacobian(u, v, np.repeat(pose[None], len(rays), 0), rays)[:, :, :3].reshape(-1, 3)
        r = orc.reloc_residual(pose, rays, points, u, v)
        _, _, w1, w2 = weights(r, loss, 0.1, f_scale)
        d = np.linalg.solve(J.T @ (w2[:, None] * J), -J.T @ (w1 * r))
        t = 1.0
        while True:
            c1 = reloc_cost(pose + t * d, rays, points, u, v, loss, f_scale)
            if c1 <= c + 1e-13 * abs(c) or t < 1e-6:
                break
            t *= 0.5
        pose, c = pose + t * d, min(c, c1)
        if t == 1.0 and np.abs(d / np.array([1.0, 1.0, 1e3])).max() < 1e-12:
            break
    J = orc.record_jacobian(u, v, np.repeat(pose[None], len(rays), 0), rays)[:, :, :3].reshape(-1, 3)
    r = orc.reloc_residual(pose, rays, points, u, v)
    w1 = weights(r, loss, 1.0, f_scale)[2]
    g = J.T @ (w1 * r)
    return pose, c, float(np.max(np.abs(g) / (np.abs(J).T @ np.abs(w1 * r))))


SCIPY_NFEV = 300  # evaluations given to scipy's trf for the recorded comparison cost


def _record(name):
    """One recorded point: the LM's stationary point and scipy's trf result from the same start after SCIPY_NFEV
    evaluations (its cost, evaluations used and status)."""
    from scipy.optimize import least_squares  # noqa: F401  (fail early without scipy)
    cfg, loss, fs, hc = POINTS[name]
    p = contaminated(cfg)
    ptz, rays, c, res, moved = lm_solve(p, loss, fs, hc)
    x0 = np.concatenate([p.init_ptz[1:].reshape(-1), p.init_rays.reshape(-1)])
    sc = orc.solve_scipy(x0, p.n_pose, p.n_landmark, p.u, p.v, p.init_ptz[0], p.frame.astype(np.int64),
                         p.landmark.astype(np.int64), p.xy, ftol=1e-15, xtol=1e-15, gtol=1e-15, analytic=True,
                         loss=loss, f_scale=fs, max_nfev=SCIPY_NFEV)
    print(name, res, "polish moved", moved, "cost", c, "stationarity", stationarity(p, ptz, rays, loss, fs),
          "scipy cost", sc.cost, "nfev", sc.nfev, "status", sc.status, flush=True)
    return {name + "_ptz": ptz, name + "_rays": rays, name + "_cost": c, name + "_scipy_cost": float(sc.cost),
            name + "_scipy_nfev": int(sc.nfev), name + "_scipy_status": int(sc.status)}


if __name__ == "__main__":
    from concurrent.futures import ProcessPoolExecutor
    out = {}
    with ProcessPoolExecutor(len(POINTS)) as ex:
        for d in ex.map(_record, list(POINTS)):
            out.update(d)
    np.savez(os.path.join(_ROOT, "tests", "golden", GOLDEN), **out)
    print("wrote", GOLDEN)
