"""fp64 NumPy restatement of libptzba's two-point PTZ pose RANSAC (csrc/pose_ransac.hip, `ptz_pose_ransac`):
the minimal solver, the counter-keyed sampling, the scoring and the tie rule, plus the deterministic scene
generator of the pose-RANSAC tests (test infrastructure; used by test_pose_ransac_ref.py, test_gpu_pose_ransac.py,
test_gpu_nn_map.py and tools/pose_ransac_time.py).

Camera model (oracle.from_ray_to_image, q form): p = [tan th, -tan ph sqrt(tan^2 th + 1), 1],
q = R_x(tilt) R_y(pan) p, x = u + f q0/q2, y = v + f q1/|q2|; for q2 > 0 a pixel sees the direction [x-u, y-v, f].

A candidate is (ca, sa, cb, sb, f) = (cos pan, sin pan, cos tilt, sin tilt, f).  Sample h draws i = draw(h, 0) and
j = draw(h, 1) (redrawn while equal to i, at most 64 attempts) and owns four candidate slots, in this order:
    slot = 2 * root + branch,   root 0: F = qq / A, root 1: F = C / qq   (the cancellation-free quadratic formula),
                                branch 0: the '+' square root of the pan equation, branch 1: the '-' one.
The winner is the candidate with the most inliers; ties go to the lowest 4 * h + slot."""
import numpy as np

from oracle import ptz_oracle as orc

D2R = np.pi / 180.0


def ray_dirs(rays):
    """[n, 2] rays (theta, phi in degrees) -> p0, p1 of p = [p0, p1, 1]."""
    rays = np.asarray(rays, np.float64).reshape(-1, 2)
    tt = np.tan(rays[:, 0] * D2R)
    return tt, -np.tan(rays[:, 1] * D2R) * np.sqrt(tt * tt + 1.0)


def sample(seed, h, n):
    """The two draws of sample h: (i, j); i == j when 64 attempts did not give a second index."""
    i = orc._ransac_draw(seed, h, 0, 0, n)
    att = 0
    while True:
        j = orc._ransac_draw(seed, h, 1, att, n)
        att += 1
        if j != i or att >= 64:
            break
    return int(i), int(j)


def minimal_solver(pi, pj, ai, aj):
    """Candidates of one sample: pi, pj = (p0, p1) of the two rays, ai, aj = (x - u, y - v) of the two pixels.
    Returns a list of (slot, (ca, sa, cb, sb, f))."""
    out = []
    mi = pi[0] * pi[0] + pi[1] * pi[1] + 1.0
    mj = pj[0] * pj[0] + pj[1] * pj[1] + 1.0
    d = pi[0] * pj[0] + pi[1] * pj[1] + 1.0
    cx, cy, cz = pi[1] - pj[1], pj[0] - pi[0], pi[0] * pj[1] - pi[1] * pj[0]  # p_i x p_j
    M = mi * mj
    c2 = d * d / M
    omc2 = (cx * cx + cy * cy + cz * cz) / M  # 1 - c^2 without the cancellation
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
        lam = np.sqrt(mi / (ni + F))
        q0, q1, q2 = lam * ai[0], lam * ai[1], lam * f
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
            out.append((2 * root + branch, (ca, sa, cbn / nb, sbn / nb, f)))
    return out


def cand_to_ptz(c):
    return np.array([np.degrees(np.arctan2(c[1], c[0])), np.degrees(np.arctan2(c[3], c[2])), c[4]])


def errors(ptz, rays, points, u, v):
    """Reprojection error [n] in px at pose ptz (oracle.from_ray_to_image) and the q2 > 0 flags."""
    rays = np.asarray(rays, np.float64).reshape(-1, 2)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    r = orc.reloc_residual(ptz, rays, points, u, v).reshape(-1, 2)
    p0, p1 = ray_dirs(rays)
    a, b = ptz[0] * D2R, ptz[1] * D2R
    w2 = np.sin(a) * p0 + np.cos(a)
    q2 = -np.sin(b) * p1 + np.cos(b) * w2
    return np.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2), q2 > 0


def inlier_mask(ptz, rays, points, u, v, threshold):
    e, front = errors(ptz, rays, points, u, v)
    return front & (e < threshold)


def pose_ransac_ref(u, v, rays, points, threshold=3.0, n_hyp=1024, seed=0):
    """All candidates of all samples, scored.  Returns a dict:
    cands      list of (h, slot, (ca, sa, cb, sb, f), ptz [3], count)
    best       index into cands of the winner (most inliers, then lowest 4 h + slot), or None
    margin     min over candidates and correspondences of | error - threshold | (px)"""
    rays = np.asarray(rays, np.float64).reshape(-1, 2)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    n = len(rays)
    p0, p1 = ray_dirs(rays)
    ax, ay = points[:, 0] - u, points[:, 1] - v
    cands = []
    margin = np.inf
    for h in range(n_hyp):
        i, j = sample(seed, h, n)
        if i == j:
            continue
        for slot, c in minimal_solver((p0[i], p1[i]), (p0[j], p1[j]), (ax[i], ay[i]), (ax[j], ay[j])):
            ptz = cand_to_ptz(c)
            e, front = errors(ptz, rays, points, u, v)
            margin = min(margin, float(np.min(np.abs(e - threshold))))
            cands.append((h, slot, c, ptz, int(np.count_nonzero(front & (e < threshold)))))
    best = None
    for k, c in enumerate(cands):  # cands are in ascending 4 h + slot: the first maximum wins
        if best is None or c[4] > cands[best][4]:
            best = k
    return {"cands": cands, "best": best, "margin": margin}


def make_scene(scene_seed, n, outlier_frac, noise, u=640.0, v=360.0):
    """The deterministic scene of the pose-RANSAC tests: a pose gt, n pixels uniform in 1280 x 720, their rays at gt
    (oracle.from_image_to_ray), observations = pixels + N(0, noise), and round(n * outlier_frac) of them replaced by
    uniform-random pixels.  Returns (gt [3], rays [n, 2], points [n, 2], inlier mask [n] bool)."""
    rng = np.random.default_rng(scene_seed)
    gt = np.array([rng.uniform(40, 75), rng.uniform(-14, -4), rng.uniform(1800, 4300)])
    pix = rng.uniform(0.0, [1280.0, 720.0], (n, 2))
    th, ph = orc.from_image_to_ray(u, v, gt[2], gt[0], gt[1], pix[:, 0], pix[:, 1])
    rays = np.stack([th, ph], 1)
    obs = pix + rng.normal(0.0, noise, (n, 2))
    n_out = int(round(n * outlier_frac))
    out = rng.choice(n, n_out, replace=False)
    obs[out] = rng.uniform(0.0, [1280.0, 720.0], (n_out, 2))
    truth = np.ones(n, bool)
    truth[out] = False
    return gt, rays, obs, truth
