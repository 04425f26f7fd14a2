"""CPU reference of bundle adjustment with Gaussian pose priors (shared by test_priors_cpu.py and
test_gpu_priors.py).  A prior is a list of factors (frames, mean, info); the objective is

    cost = 1/2 sum rho(r^2) + 1/2 sum_k e_k^T info_k e_k,     e_k = x[frames_k] - mean_k

with the oracle's residual and analytic Jacobian for the first term (cov_ref.normal_matrix's ingredients).  Gives the
dense normal matrix H + P, the gradient, the cost, one Gauss-Newton step and a Gauss-Newton / IRLS iteration to the
stationary point.  Frame 0 is the gauge (n_fixed = 1), as in the oracle's Jacobian."""
import functools

import numpy as np


def prior_terms(factors, ptz, n_pose):
    """(P [3 (n_pose - 1)]^2 dense, P e [3 (n_pose - 1)], prior cost) at the poses ptz [n_pose, 3]."""
    k = 3 * (n_pose - 1)
    P = np.zeros((k, k))
    g = np.zeros(k)
    c = 0.0
    x = np.asarray(ptz, np.float64).reshape(-1)
    for frames, mean, info in factors:
        frames = np.atleast_1d(np.asarray(frames, np.int64))
        assert frames.min() >= 1 and frames.max() < n_pose
        idx = (3 * frames[:, None] + np.arange(3)[None, :]).reshape(-1)
        L = np.asarray(info, np.float64)
        e = x[idx] - np.asarray(mean, np.float64).reshape(-1)
        Le = L @ e
        P[np.ix_(idx - 3, idx - 3)] += L
        g[idx - 3] += Le
        c += 0.5 * float(e @ Le)
    return P, g, c


def prior_cost(factors, ptz):
    ptz = np.asarray(ptz, np.float64)
    return prior_terms(factors, ptz, len(ptz))[2]


def _records(p, ptz, rays, loss, f_scale):
    """(J sparse over the free parameters, r, per-residual cost, gradient weight, curvature weight)."""
    from oracle import ptz_oracle as orc
    ptz = np.asarray(ptz, np.float64)
    rays = np.asarray(rays, np.float64)
    fr, lm = p.frame.astype(np.int64), p.landmark.astype(np.int64)
    x = np.concatenate([ptz[1:].reshape(-1), rays.reshape(-1)])
    J = orc.ba_jacobian(x, p.n_pose, p.n_landmark, p.u, p.v, ptz[0], fr, lm).tocsr()
    r = orc.compute_residual_records(np.concatenate([ptz[0], x]), p.n_pose, p.u, p.v, fr, lm, p.xy)
    c, w1, w2 = orc._loss_weights(r, loss, f_scale)
    return J, r, c, w1, w2


def cost(p, ptz, rays, factors, loss="linear", f_scale=1.0):
    return float(np.sum(_records(p, ptz, rays, loss, f_scale)[2])) + prior_cost(factors, ptz)


def gradient(p, ptz, rays, factors, loss="linear", f_scale=1.0):
    """d cost / d [free poses | rays]."""
    J, r, _, w1, _ = _records(p, ptz, rays, loss, f_scale)
    g = np.asarray(J.T @ (w1 * r)).reshape(-1)
    g[:3 * (p.n_pose - 1)] += prior_terms(factors, ptz, p.n_pose)[1]
    return g


def normal_matrix(p, ptz, rays, factors, loss="linear", f_scale=1.0):
    """Dense H + P, H = cov_ref.normal_matrix (J^T diag(rho') J: the IRLS weights for the Huber loss)."""
    import cov_ref
    H = cov_ref.normal_matrix(p, ptz, rays, loss, f_scale)
    k = 3 * (p.n_pose - 1)
    H[:k, :k] += prior_terms(factors, ptz, p.n_pose)[0]
    return H


def gn_step(p, ptz, rays, factors, loss="linear", f_scale=1.0, curvature=False):
    """dx of (H + P) dx = -(g + P e) (sparse solve); curvature=True weights H by the loss's floored Newton curvature
    instead of the IRLS weights (the same stationary point, fewer iterations)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    J, r, _, w1, w2 = _records(p, ptz, rays, loss, f_scale)
    P, gp, _ = prior_terms(factors, ptz, p.n_pose)
    k = 3 * (p.n_pose - 1)
    n = J.shape[1]
    Jw = sp.diags(np.sqrt(w2 if curvature else w1)) @ J
    H = (Jw.T @ Jw).tolil()
    H[:k, :k] = H[:k, :k] + sp.lil_matrix(P)
    g = np.asarray(J.T @ (w1 * r)).reshape(-1)
    g[:k] += gp
    dx = spla.spsolve(H.tocsc(), -g)
    assert dx.shape == (n,)
    return dx, g


def split(p, dx):
    k = 3 * (p.n_pose - 1)
    dptz = np.concatenate([np.zeros((1, 3)), dx[:k].reshape(-1, 3)])
    return dptz, dx[k:].reshape(-1, 2)


def solve(p, ptz0, rays0, factors, loss="linear", f_scale=1.0, max_iter=100, gtol=1e-9):
    """Gauss-Newton (linear) / floored-Newton IRLS (huber) with step halving to the stationary point: stops after a
    full step below 1e-10 (deg; 1e-7 px of focal length), and checks the gradient there.  Returns
    (ptz, rays, cost)."""
    ptz = np.array(ptz0, np.float64)
    rays = np.array(rays0, np.float64)
    c = cost(p, ptz, rays, factors, loss, f_scale)
    for _ in range(max_iter):
        dx, _ = gn_step(p, ptz, rays, factors, loss, f_scale, curvature=loss == "huber")
        dptz, drays = split(p, dx)
        t = 1.0
        while True:
            c1 = cost(p, ptz + t * dptz, rays + t * drays, factors, loss, f_scale)
            if c1 <= c + 1e-12 * abs(c) or t < 1e-6:  # (equal up to the cost's rounding near the optimum)
                break
            t *= 0.5
        ptz, rays, c = ptz + t * dptz, rays + t * drays, min(c, c1)
        scale = np.array([1.0, 1.0, 1e3])
        if t == 1.0 and np.abs(dptz / scale).max() < 1e-10 and np.abs(drays).max() < 1e-10:
            break
    assert_stationary(p, ptz, rays, factors, loss, f_scale, gtol)
    return ptz, rays, c


def assert_stationary(p, ptz, rays, factors, loss="linear", f_scale=1.0, gtol=1e-9):
    """Every gradient entry at (ptz, rays) is rounding noise (gtol) against the magnitude of the terms it sums."""
    ptz = np.asarray(ptz, np.float64)
    J, r, _, w1, _ = _records(p, ptz, rays, loss, f_scale)
    g = gradient(p, ptz, rays, factors, loss, f_scale)
    mag = np.asarray(abs(J).T @ np.abs(w1 * r)).reshape(-1) + 1e-300
    for frames, mean, info in factors:
        idx = (3 * np.atleast_1d(np.asarray(frames, np.int64))[:, None] + np.arange(3)[None, :]).reshape(-1)
        mag[idx - 3] += np.abs(info) @ np.abs(ptz.reshape(-1)[idx] - np.asarray(mean, np.float64).reshape(-1))
    assert np.max(np.abs(g) / mag) < gtol, np.max(np.abs(g) / mag)


# ------------------------------------------------------------------------------------------------
# the factor set of the GPU tests
# ------------------------------------------------------------------------------------------------
SIGMA = np.array([0.02, 0.02, 2.0])  # deg, deg, px: an encoder-grade prior


def _spd(rng, frames):
    """A dense SPD information matrix over the frames' 3 G parameters with standard deviations ~ SIGMA."""
    n = 3 * len(frames)
    A = rng.standard_normal((n, n))
    C = A @ A.T / n + np.eye(n)  # correlation-like, eigenvalues >= 1
    s = 1.0 / np.tile(SIGMA, len(frames))
    L = C * np.outer(s, s)
    return 0.5 * (L + L.T)


def factor_set(p, extra_pairs=(), far_pair=None, seed=0):
    """The factor set of test_gpu_priors.py over problem p: a unary prior on the first free frame and on the last
    frame, the adjacent pairs `extra_pairs` (whose system rows straddle a tile boundary at config 2), an adjacent
    pair and a dense G = 3 factor, two of them sharing a frame, and `far_pair` (config 2: (1, 45), outside the
    records' coupling window).  Means sit up to 10 sigma off the problem's initial poses, so the priors pull."""
    rng = np.random.default_rng(seed)
    n = p.n_pose
    groups = [[1], [n - 1], [n // 2, n // 2 + 1], [n // 2 + 1, n // 2 + 3, n // 2 + 2]]
    groups += [list(q) for q in extra_pairs]
    if far_pair is not None:
        groups.append(list(far_pair))
    out = []
    for fr in groups:
        mean = (p.init_ptz[fr] + rng.uniform(-10.0, 10.0, (len(fr), 3)) * SIGMA).reshape(-1)
        out.append((np.array(fr, np.int32), mean, _spd(rng, fr)))
    return out


@functools.lru_cache(maxsize=None)
def problem(cfg, seed=0):
    import synthetic
    return synthetic.make_problem(cfg, seed=seed)


CONFIG2_PAIRS = ((11, 12), (15, 16), (47, 48))  # see test_gpu_priors.py
CONFIG2_FAR = (1, 45)
CONFIG2_HUBER = "priors_config2_huber.npz"


def config2_factors():
    return factor_set(problem("config2"), CONFIG2_PAIRS, CONFIG2_FAR)


def config2_huber_point(path):
    """The recorded stationary point (ptz, rays, cost) of config 2's Huber objective (f_scale 1) with
    config2_factors(), made by `python tests/prior_ref.py` (solve() from the no-prior optimum of
    config2_optimum.npz takes ~20 s of Jacobians: recorded once).  Its stationarity is checked here on every load,
    against the factor set and problem as they are now."""
    d = np.load(path, allow_pickle=False)
    p = problem("config2")
    factors = config2_factors()
    assert_stationary(p, d["ptz"], d["rays"], factors, "huber", 1.0)
    c = cost(p, d["ptz"], d["rays"], factors, "huber", 1.0)
    assert abs(c - float(d["cost"])) <= 1e-12 * c
    return d["ptz"], d["rays"], c


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "pan-tilt-zoom-slam_amd"), root]
    gold = os.path.join(root, "tests", "golden")
    p2 = problem("config2")
    xt = np.load(os.path.join(gold, "config2_optimum.npz"))["x_tight_huber"]
    k2 = 3 * (p2.n_pose - 1)
    ptz2, rays2, c2 = solve(p2, np.concatenate([p2.init_ptz[0], xt[:k2]]).reshape(-1, 3), xt[k2:].reshape(-1, 2),
                            config2_factors(), "huber", 1.0)
    np.savez(os.path.join(gold, CONFIG2_HUBER), ptz=ptz2, rays=rays2, cost=c2)
    print("wrote", CONFIG2_HUBER, "cost", c2)
