"""fp64 NumPy restatement of relocalisation under the displaced camera K (R p + d(f)): the exact
inverse projection (`ptz_back_project_rays_exact`), the displaced two-point minimal solver of `ptz_pose_ransac_disp`
(the kernel's Newton steps one for one), the scored candidate list, and the scene generator of the tests (test
infrastructure; used by test_reloc_disp_cpu.py and test_gpu_reloc_disp.py).

Model (disp_ref.project): r = R_x(tilt) R_y(pan) p, q = r + d(f), d(f) = (l0 + l3 f, l1 + l4 f, l2 + l5 f),
x = u + f q0 / q2, y = v + f q1 / |q2|.

Minimal solver: a pixel a = (x - u, y - v) at focal length f sees q = t nh, nh = (a0, a1, f); r = q - d(f) has
|r|^2 = |p|^2 =: m, so t is the positive root of t^2 |nh|^2 - 2 t (nh . d) + |d|^2 - m = 0, and the rotation keeps
r_i . r_j = p_i . p_j =: g(f) = 0.  NEWTON steps of Newton's iteration in f with the analytic dg/df, from each accepted
root of pose_ransac_ref.minimal_solver's closed form; the slot is 2 * (that root) + branch."""
import numpy as np

import disp_ref
import pose_ransac_ref as pr

D2R = np.pi / 180.0
NEWTON = 6  # csrc/pose_ransac.hip PR_NEWTON


def rotation(pan, tilt):
    """R_x(tilt) R_y(pan) (csrc/camera_model.h rot_tp)."""
    a, b = pan * D2R, tilt * D2R
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return np.array([[ca, 0.0, -sa], [sb * sa, cb, sb * ca], [cb * sa, -sb, cb * ca]])


def back_project_exact(u, v, f, pan, tilt, points, lam):
    """The exact inverse of the displaced projection: (rays [n, 2] in degrees, valid [n] bool).  With
    n = ((x - u) / f, (y - v) / f, 1) the direction p = (p0, p1, 1) solves R p + d = t n:
    t = (1 + (R^T d)_z) / (R^T n)_z, p = t R^T n - R^T d.  Not valid ((R^T n)_z <= 0, t <= 0 or a non-finite result):
    the ray is NaN."""
    points = np.asarray(points, np.float64).reshape(-1, 2)
    lam = np.asarray(lam, np.float64)
    R = rotation(pan, tilt)
    n = np.stack([(points[:, 0] - u) / f, (points[:, 1] - v) / f, np.ones(len(points))], 1)
    d = lam[:3] + lam[3:] * f
    rn = n @ R  # rows: R^T n
    rd = R.T @ d
    with np.errstate(all="ignore"):
        t = (1.0 + rd[2]) / rn[:, 2]
        p0 = t * rn[:, 0] - rd[0]
        p1 = t * rn[:, 1] - rd[1]
        th = np.arctan(p0) / D2R
        ph = np.arctan(-p1 / np.sqrt(p0 * p0 + 1.0)) / D2R
        valid = (rn[:, 2] > 0.0) & (t > 0.0) & np.isfinite(th) & np.isfinite(ph)
    rays = np.stack([th, ph], 1)
    rays[~valid] = np.nan
    return rays, valid


def disp_ray(a0, a1, m, f, lam):
    """(r [3], dr/df [3], ok) of pixel (a0, a1) at focal length f (csrc/pose_ransac.hip pr_disp_ray)."""
    c, k = lam[:3], lam[3:]
    d0, d1, d2 = c[0] + k[0] * f, c[1] + k[1] * f, c[2] + k[2] * f
    N = a0 * a0 + a1 * a1 + f * f
    b = a0 * d0 + a1 * d1 + f * d2
    dd = d0 * d0 + d1 * d1 + d2 * d2
    disc = b * b - N * (dd - m)
    with np.errstate(all="ignore"):
        S = np.sqrt(disc)
        t = (b + S) / N
        bp = d2 + a0 * k[0] + a1 * k[1] + f * k[2]
        dkd = d0 * k[0] + d1 * k[1] + d2 * k[2]
        tp = -(t * t * f - t * bp + dkd) / S
    r = np.array([t * a0 - d0, t * a1 - d1, t * f - d2])
    dr = np.array([tp * a0 - k[0], tp * a1 - k[1], tp * f + t - k[2]])
    return r, dr, bool(disc >= 0.0)


def g_and_slope(pi, pj, ai, aj, f, lam):
    """g(f) = r_i . r_j - p_i . p_j and its analytic derivative."""
    mi = pi[0] * pi[0] + pi[1] * pi[1] + 1.0
    mj = pj[0] * pj[0] + pj[1] * pj[1] + 1.0
    d = pi[0] * pj[0] + pi[1] * pj[1] + 1.0
    ri, dri, _ = disp_ray(ai[0], ai[1], mi, f, lam)
    rj, drj, _ = disp_ray(aj[0], aj[1], mj, f, lam)
    return float(ri @ rj - d), float(dri @ rj + ri @ drj)


def minimal_solver_disp(pi, pj, ai, aj, lam, steps=NEWTON, trace=None):
    """Candidates of one sample under the displacement lam: a list of (slot, (ca, sa, cb, sb, f)).  trace (a list)
    receives, per started root, the f after every Newton step."""
    lam = np.asarray(lam, np.float64)
    out = []
    mi = pi[0] * pi[0] + pi[1] * pi[1] + 1.0
    mj = pj[0] * pj[0] + pj[1] * pj[1] + 1.0
    d = pi[0] * pj[0] + pi[1] * pj[1] + 1.0
    cx, cy, cz = pi[1] - pj[1], pj[0] - pi[0], pi[0] * pj[1] - pi[1] * pj[0]
    M = mi * mj
    c2 = d * d / M
    omc2 = (cx * cx + cy * cy + cz * cz) / M
    if not omc2 > 1e-14:
        return out
    s = ai[0] * aj[0] + ai[1] * aj[1]
    ni = ai[0] * ai[0] + ai[1] * ai[1]
    nj = aj[0] * aj[0] + aj[1] * aj[1]
    A = omc2
    B = 2.0 * s - c2 * (ni + nj)
    C = s * s - c2 * ni * nj
    disc = B * B - 4.0 * A * C
    if not disc > 0.0:
        return out
    qq = -0.5 * (B + (np.sqrt(disc) if B >= 0 else -np.sqrt(disc)))
    for root, F in enumerate((qq / A, C / qq if qq != 0 else -1.0)):
        if not (F > 0.0 and (s + F) * d > 0.0):
            continue
        f = np.sqrt(F)
        ok = True
        fs = [float(f)]
        with np.errstate(all="ignore"):
            for _ in range(steps):
                ri, dri, oi = disp_ray(ai[0], ai[1], mi, f, lam)
                rj, drj, oj = disp_ray(aj[0], aj[1], mj, f, lam)
                ok = ok and oi and oj
                g = ri[0] * rj[0] + ri[1] * rj[1] + ri[2] * rj[2] - d
                gp = (dri[0] * rj[0] + dri[1] * rj[1] + dri[2] * rj[2] + ri[0] * drj[0] + ri[1] * drj[1] +
                      ri[2] * drj[2])
                f = f - g / gp
                fs.append(float(f))
            ri, _, oi = disp_ray(ai[0], ai[1], mi, f, lam)
        if trace is not None:
            trace.append(fs)
        if not (ok and oi and np.isfinite(f) and f > 0.0):
            continue
        q0, q1, q2 = ri
        p0, p1 = pi
        r2 = 1.0 + p0 * p0 - q0 * q0
        if not r2 >= 0.0:
            continue
        r = np.sqrt(r2)
        for branch, sg in enumerate((1.0, -1.0)):
            ca = (p0 * q0 + sg * r) / (1.0 + p0 * p0)
            sa = (-q0 + sg * p0 * r) / (1.0 + p0 * p0)
            w2 = sa * p0 + ca
            cbn = q1 * p1 + q2 * w2
            sbn = q1 * w2 - q2 * p1
            nb = np.sqrt(cbn * cbn + sbn * sbn)
            if not nb > 0.0:
                continue
            out.append((2 * root + branch, (ca, sa, cbn / nb, sbn / nb, float(f))))
    return out


def residual(pose, rays, points, u, v, lam):
    """Interleaved reprojection residuals [2 n] of the displaced model (what scipy's least_squares minimises)."""
    rays = np.asarray(rays, np.float64).reshape(-1, 2)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    xy, _ = disp_ref.project(u, v, np.tile(np.asarray(pose, np.float64), (len(rays), 1)), rays, lam)
    return (xy - points).reshape(-1)


def errors_disp(ptz, rays, points, u, v, lam):
    """Reprojection error [n] in px at pose ptz under lam (disp_ref.project) and the q2 > 0 flags."""
    rays = np.asarray(rays, np.float64).reshape(-1, 2)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    xy, q2 = disp_ref.project(u, v, np.tile(np.asarray(ptz, np.float64), (len(rays), 1)), rays, lam)
    e = xy - points
    return np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2), q2 > 0


def inlier_mask_disp(ptz, rays, points, u, v, lam, threshold):
    e, front = errors_disp(ptz, rays, points, u, v, lam)
    return front & (e < threshold)


def pose_ransac_ref_disp(u, v, rays, points, lam, threshold=3.0, n_hyp=1024, seed=0, steps=NEWTON):
    """pose_ransac_ref.pose_ransac_ref under the displacement lam: the same dict (cands, best, margin)."""
    rays = np.asarray(rays, np.float64).reshape(-1, 2)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    n = len(rays)
    p0, p1 = pr.ray_dirs(rays)
    ax, ay = points[:, 0] - u, points[:, 1] - v
    cands = []
    margin = np.inf
    for h in range(n_hyp):
        i, j = pr.sample(seed, h, n)
        if i == j:
            continue
        for slot, c in minimal_solver_disp((p0[i], p1[i]), (p0[j], p1[j]), (ax[i], ay[i]), (ax[j], ay[j]), lam, steps):
            ptz = pr.cand_to_ptz(c)
            e, front = errors_disp(ptz, rays, points, u, v, lam)
            margin = min(margin, float(np.min(np.abs(e - threshold))))
            cands.append((h, slot, c, ptz, int(np.count_nonzero(front & (e < threshold)))))
    best = None
    for k, c in enumerate(cands):
        if best is None or c[4] > cands[best][4]:
            best = k
    return {"cands": cands, "best": best, "margin": margin}


def make_scene_disp(scene_seed, n, outlier_frac, noise, u=640.0, v=360.0, lam=disp_ref.LAMBDA):
    """pose_ransac_ref.make_scene seen through the displaced camera: the same draws in the same order, but pan from
    40..65 degrees (every pixel of 1280 x 720 then has a valid ray) and the rays from the exact inverse at the ground
    truth under lam.  Returns (gt [3], rays [n, 2], points [n, 2], inlier mask [n] bool)."""
    rng = np.random.default_rng(scene_seed)
    gt = np.array([rng.uniform(40, 65), rng.uniform(-14, -4), rng.uniform(1800, 4300)])
    pix = rng.uniform(0.0, [1280.0, 720.0], (n, 2))
    rays, valid = back_project_exact(u, v, gt[2], gt[0], gt[1], pix, lam)
    assert valid.all()
    obs = pix + rng.normal(0.0, noise, (n, 2))
    n_out = int(round(n * outlier_frac))
    out = rng.choice(n, n_out, replace=False)
    obs[out] = rng.uniform(0.0, [1280.0, 720.0], (n_out, 2))
    truth = np.ones(n, bool)
    truth[out] = False
    return gt, rays, obs, truth


def scipy_optimum(x0, rays, points, u, v, lam, loss="linear", f_scale=1.0):
    """scipy's least_squares on the displaced residual, tolerances 1e-15."""
    from scipy.optimize import least_squares
    return least_squares(residual, np.asarray(x0, np.float64), x_scale='jac', ftol=1e-15, xtol=1e-15, gtol=1e-15,
                         method='trf', loss=loss, f_scale=f_scale, args=(rays, points, u, v, lam))
