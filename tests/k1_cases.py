"""Crafted bundle-adjustment problems that reach every path of the linearisation kernel K1 (k_linearize,
csrc/ba_kernels.hip) at ~5,500 records, and a dense fp64 reference of one damped step (test infrastructure; used by
tests/test_k1_cases.py on the CPU and tests/test_gpu_k1_paths.py on the GPU).

The records are arbitrary (frame, landmark, xy) triples, not pair form: ptzba_set_problem accepts them."""
import numpy as np

from oracle import ptz_oracle as orc

K1_SEGW = 128  # csrc/ptzba_kernels.h: segments per K1 window
F_SCALES = (1.0, 2.5)  # the Huber scales the tests use: no |r| / f_scale of a crafted case lies near the unit for either


def _structure(n_pose, extra, rng):
    """[(landmark, frame, records)] per segment; landmark ids in the order that puts every record-group alignment
    (first record & 3) at a window boundary inside the long landmarks (layout(): checked by test_k1_cases.py)."""
    segs = []
    lm = 0

    def add(frames, counts):
        nonlocal lm
        segs.extend((lm, int(f), int(c)) for f, c in zip(frames, counts))
        lm += 1

    allf = np.arange(n_pose)
    far_starts = [0, 1, 2, n_pose - 5, n_pose - 4, n_pose - 3]
    # long: every frame (ceil(n_pose / 128) windows, an own frame range beyond the LDS table)
    add(allf, np.ones(n_pose, int))
    add(allf, 1 + allf % 3)
    add(np.arange(far_starts[0], far_starts[0] + 3), (3, 2, 2))  # (a far landmark here: 7 records shift the next one)
    c = np.ones(n_pose, int)
    c[n_pose // 2] = 700  # one run over three 256-record batches
    add(allf, c)
    # far: one size class (7 records), sorted by first frame: a workgroup that holds both ends falls back
    for s in far_starts[1:]:
        add(np.arange(s, s + 3), (3, 2, 2))
    # local: 12 consecutive frames, starting every 3 frames, and one over the last 12 frames
    for s in list(range(0, n_pose - 11, 3)) + [n_pose - 12]:
        add(np.arange(s, s + 12), rng.integers(1, 4, 12))
    # tiny: one record; one 5-record segment.  With the `extra` two-record landmarks they end the work order (the
    # smallest size classes) in neighbouring frames, so the last workgroup stages its tables in LDS whatever the table size
    t0 = n_pose // 4
    add([t0], [1])
    add([t0 + 4], [5])
    for e in range(extra):
        add([t0 + 1 + e, t0 + 2 + e], [1, 1])
    return segs, lm


def craft(n_pose=400, extra=0, weighted=False, seed=7):
    """(u, v, ptz0, rays0, frame, landmark, xy, weight): see the module docstring and _structure.
    Poses on a narrow arc (pan 48-56 deg, tilt ~ -10 deg, f ~ 3000), rays at theta in [50, 54], phi in [-12, -8];
    observations = projection of the true state + 0.5 px noise, ~15 % of the records 8 px further off (both Huber
    branches populated); (ptz0, rays0) = the truth perturbed (frame 0 exact).  weighted: every record carries an integer
    multiplicity from {1, 2, 3, 5} (the rec_w instantiation of K1), else weight is None.  Record order shuffled."""
    assert 0 <= extra <= 3 and n_pose >= 64
    rng = np.random.default_rng(seed)
    u, v = 640.0, 360.0
    segs, n_lm = _structure(n_pose, extra, rng)
    seg_lm = np.array([s[0] for s in segs])
    seg_fr = np.array([s[1] for s in segs])
    cnt = np.array([s[2] for s in segs])
    landmark = np.repeat(seg_lm, cnt).astype(np.int32)
    frame = np.repeat(seg_fr, cnt).astype(np.int32)
    n = len(frame)
    ptz = np.stack([np.linspace(48.0, 56.0, n_pose) + rng.normal(0, 0.05, n_pose),
                    -10.0 + rng.normal(0, 0.2, n_pose), 3000.0 + rng.normal(0, 40.0, n_pose)], -1)
    rays = np.stack([rng.uniform(50.0, 54.0, n_lm), rng.uniform(-12.0, -8.0, n_lm)], -1)
    px, py = orc.from_ray_to_image(u, v, ptz[frame, 2], ptz[frame, 0], ptz[frame, 1], rays[landmark, 0], rays[landmark, 1])
    xy = np.stack([px, py], -1) + rng.normal(0, 0.5, (n, 2))
    out = rng.random(n) < 0.15
    xy[out] += 8.0 * rng.choice([-1.0, 1.0], (int(out.sum()), 2))
    ptz0 = ptz + rng.normal(0, 1.0, (n_pose, 3)) * np.array([0.015, 0.01, 5.0])
    ptz0[0] = ptz[0]
    rays0 = rays + rng.normal(0, 0.01, (n_lm, 2))
    weight = rng.choice([1.0, 2.0, 3.0, 5.0], n) if weighted else None
    perm = rng.permutation(n)
    frame, landmark, xy = frame[perm], landmark[perm], xy[perm]
    # no residual within 1e-3 (in z = (r / f_scale)^2) of the Huber unit at x0, for either scale: fp32 records must not
    # flip a branch.  Offending observations move 0.02 px away from the threshold.
    for _ in range(8):
        r = orc.compute_residual_records(np.concatenate([ptz0.reshape(-1), rays0.reshape(-1)]), n_pose, u, v,
                                         frame.astype(np.int64), landmark.astype(np.int64), xy).reshape(-1, 2)
        bad = np.zeros(r.shape, bool)
        for fs in F_SCALES:
            bad |= np.abs((r / fs) ** 2 - 1.0) < 2e-3
        if not bad.any():
            break
        # r = projection - xy: a larger |r| needs xy further from the projection
        grow = np.zeros(r.shape, bool)
        for fs in F_SCALES:
            grow |= (np.abs((r / fs) ** 2 - 1.0) < 2e-3) & (np.abs(r) >= fs)
        step = np.where(grow, 1.0, -1.0) * np.sign(r) * 0.02
        xy = xy - np.where(bad, step, 0.0)
    return u, v, ptz0, rays0, frame, landmark, xy, weight


def expand(problem):
    """The same cost with every record repeated `weight` times (integer multiplicities) and no weights: the form the
    oracle's own cost and block functions take."""
    u, v, ptz0, rays0, frame, landmark, xy, weight = problem
    if weight is None:
        return problem
    k = weight.astype(np.int64)
    return u, v, ptz0, rays0, np.repeat(frame, k), np.repeat(landmark, k), np.repeat(xy, k, axis=0), None


def layout(problem):
    """The sorted record layout ptzba_set_problem builds (records by landmark, then frame): per landmark its segment
    count and first record, and the set of (first record & 3) over the window boundaries INSIDE landmarks (segment
    128, 256, ... of a landmark), where K1 masks the neighbouring window's records in a shared 4-record group."""
    frame, landmark = problem[4].astype(np.int64), problem[5].astype(np.int64)
    n_pose = len(problem[2])
    key, cnt = np.unique(landmark * n_pose + frame, return_counts=True)
    seg_lm = key // n_pose
    rec_begin = np.concatenate([[0], np.cumsum(cnt)])
    align = set()
    windows = 0
    for l in np.unique(seg_lm):
        s = np.flatnonzero(seg_lm == l)
        windows = max(windows, -(-len(s) // K1_SEGW))
        for w in range(K1_SEGW, len(s), K1_SEGW):
            align.add(int(rec_begin[s[w]]) & 3)
    return dict(n_segments=len(key), n_records=len(frame), max_windows=windows, boundary_alignments=align,
                max_run=int(cnt.max()), frames_seen=[len(np.unique(seg_lm[key % n_pose == f])) for f in range(n_pose)])


def _weights(r, loss, hcurv, f_scale):
    z = (r / f_scale) ** 2
    if loss == "huber":
        inl = z <= 1.0
        sq = np.sqrt(np.maximum(z, 1.0))
        rho = np.where(inl, z, 2.0 * sq - 1.0)
        w1 = np.where(inl, 1.0, 1.0 / sq)
        w2 = np.where(inl, 1.0, hcurv * w1)
        return z, rho, w1, w2
    assert loss == "linear"
    one = np.ones_like(r)
    return z, z, one, one


def cost_at(problem, ptz, rays, loss="linear", f_scale=1.0):
    """0.5 f_scale^2 sum w rho((r / f_scale)^2) over the scalar residuals at (ptz, rays), fp64."""
    u, v, _, _, frame, landmark, xy, weight = problem
    r = orc.compute_residual_records(np.concatenate([ptz.reshape(-1), rays.reshape(-1)]), len(ptz), u, v,
                                     frame.astype(np.int64), landmark.astype(np.int64), xy)
    w = np.ones(len(r)) if weight is None else np.repeat(weight, 2)
    return 0.5 * f_scale ** 2 * float(np.sum(w * _weights(r, loss, 1.0, f_scale)[1]))


def linearise(problem, loss="linear", hcurv=1.0, f_scale=1.0, ptz=None, rays=None, round32=False):
    """cost, H, g (and z) of reference() at (ptz, rays): the part of a step that does not depend on the damping."""
    u, v, ptz0, rays0, frame, landmark, xy, weight = problem
    ptz = ptz0 if ptz is None else ptz
    rays = rays0 if rays is None else rays
    n_pose, n_lm = len(ptz), len(rays)
    fr, lm = frame.astype(np.int64), landmark.astype(np.int64)
    x = np.concatenate([ptz[1:].reshape(-1), rays.reshape(-1)])
    J = orc.ba_jacobian(x, n_pose, n_lm, u, v, ptz[0], fr, lm).tocsr()
    r = orc.compute_residual_records(np.concatenate([ptz[0], x]), n_pose, u, v, fr, lm, xy)
    w = np.ones(len(r)) if weight is None else np.repeat(weight, 2)
    z, rho, w1, w2 = _weights(r, loss, hcurv, f_scale)
    cost = 0.5 * f_scale ** 2 * float(np.sum(w * rho))
    if round32:
        J = J.astype(np.float32).astype(np.float64)
        r = r.astype(np.float32).astype(np.float64)
    H = (J.T @ J.multiply((w * w2)[:, None])).toarray()
    g = J.T @ (w * w1 * r)
    return dict(cost=cost, H=H, g=g, z=z, gmax=float(np.abs(g).max()), n_free_pose=n_pose - 1)


def reference(problem, lam, loss="linear", hcurv=1.0, f_scale=1.0, D_prev=None, ptz=None, rays=None, lin=None):
    """One damped Gauss-Newton / Levenberg-Marquardt step of the library's host-step API in dense fp64, at
    (ptz, rays) (default: the problem's ptz0, rays0), frame 0 fixed:

      J = orc.ba_jacobian, r = orc.compute_residual_records; per scalar residual z = (r / f_scale)^2,
      huber: rho = z | 2 sqrt(z) - 1, w1 = 1 | 1 / sqrt(z), w2 = 1 | hcurv w1 (inside | beyond the unit), w = record weight
      cost = 1/2 f_scale^2 sum w rho;  H = J^T diag(w w2) J;  g = J^T (w w1 r)
      D = max(D_prev, diag H, 1e-12);  dx = solve(H + lam diag(D), -g)
      pred = -1/2 g.dx + 1/2 lam dx^T D dx;  |dx|^2;  max |g|

    What it mirrors in the kernels: the Hessian weight hx / hy = w w2 and the gradient weight wx / wy = w w1 of
    k_linearize (csrc/ba_kernels.hip); the damping rule D = max(D, diag, 1e-12) with its memory across steps in
    k_build_prologue (rays, ba_kernels.hip) and in k_schur_reduce's fused prepare / k_chol_prepare (poses, diag U:
    schur_kernels.hip, chol_kernels.hip); the predicted reduction, |delta|^2 and max |gradient| of k_trial
    (ba_kernels.hip) summed by k_reduce_cols; ptzba_set_state zeroes D (D_prev = None).
    lin: a linearise() result at the same point to reuse (several dampings of one linearisation).
    Returns a dict: cost, dx, g, D, H, pred, dx2, gmax, z, n_free_pose (dx / g / D order: free poses, then rays)."""
    if lin is None:
        lin = linearise(problem, loss, hcurv, f_scale, ptz, rays)
    H, g = lin["H"], lin["g"]
    D = np.maximum(np.diag(H), 1e-12)
    if D_prev is not None:
        D = np.maximum(D, D_prev)
    dx = np.linalg.solve(H + lam * np.diag(D), -g)
    pred = -0.5 * float(g @ dx) + 0.5 * lam * float(dx @ (D * dx))
    return dict(lin, dx=dx, D=D, pred=pred, dx2=float(dx @ dx))


def split_kinds(d, n_free_pose):
    """A free-parameter vector (free poses, then rays) by kind: pan and tilt (deg), f (px), rays (deg)."""
    p = d[:3 * n_free_pose].reshape(-1, 3)
    return {"pan_tilt": p[:, :2].reshape(-1), "f": p[:, 2], "rays": d[3 * n_free_pose:]}
