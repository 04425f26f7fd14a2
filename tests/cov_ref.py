"""CPU reference of the BA posterior covariance blocks (shared by test_covariance_cpu.py and
test_gpu_covariance.py): the oracle's analytic Jacobian at a state, rows scaled by sqrt(rho') for the Huber loss,
H = J^T J densified and inverted whole; the pose and ray blocks are cut out of that inverse.  A second route through
the Schur complement (numpy) checks the first."""
import functools

import numpy as np


def normal_matrix(p, ptz, rays, loss="linear", f_scale=1.0, n_fixed=1):
    """Dense H = J^T diag(rho') J over [3 (n_pose - n_fixed) poses | 2 M rays] at (ptz, rays)."""
    import scipy.sparse as sp
    from oracle import ptz_oracle as orc
    ptz = np.asarray(ptz, np.float64)
    rays = np.asarray(rays, np.float64)
    fr, lm = p.frame.astype(np.int64), p.landmark.astype(np.int64)
    x = np.concatenate([ptz[1:].reshape(-1), rays.reshape(-1)])
    J = orc.ba_jacobian(x, p.n_pose, p.n_landmark, p.u, p.v, ptz[0], fr, lm).tocsr()
    if loss == "huber":
        r = orc.compute_residual_records(np.concatenate([ptz[0], x]), p.n_pose, p.u, p.v, fr, lm, p.xy)
        w1 = orc._loss_weights(r, "huber", f_scale)[1]
        J = sp.diags(np.sqrt(w1)) @ J
    J = J.tocsc()[:, 3 * (n_fixed - 1):]
    return np.asarray((J.T @ J).todense())


def _cut(C, n_pose, n_landmark, n_fixed):
    pose = np.zeros((n_pose, 3, 3))
    for f in range(n_fixed, n_pose):
        o = 3 * (f - n_fixed)
        pose[f] = C[o:o + 3, o:o + 3]
    o = 3 * (n_pose - n_fixed)
    ray = np.stack([C[o + 2 * l:o + 2 * l + 2, o + 2 * l:o + 2 * l + 2] for l in range(n_landmark)])
    return pose, ray


def dense_blocks(p, ptz, rays, loss="linear", f_scale=1.0, n_fixed=1):
    """(pose_cov [n_pose,3,3] with the fixed frames zero, ray_cov [M,2,2]) from np.linalg.inv(H)."""
    H = normal_matrix(p, ptz, rays, loss, f_scale, n_fixed)
    return _cut(np.linalg.inv(H), p.n_pose, p.n_landmark, n_fixed)


def schur_blocks(p, ptz, rays, loss="linear", f_scale=1.0, n_fixed=1):
    """The same blocks through S = U - W V^-1 W^T: pose blocks from inv(S), ray blocks V^-1 + Y^T S^-1 Y."""
    H = normal_matrix(p, ptz, rays, loss, f_scale, n_fixed)
    k = 3 * (p.n_pose - n_fixed)
    U, W = H[:k, :k], H[:k, k:]
    Vi = np.zeros((p.n_landmark, 2, 2))
    for l in range(p.n_landmark):
        Vi[l] = np.linalg.inv(H[k + 2 * l:k + 2 * l + 2, k + 2 * l:k + 2 * l + 2])
    Y = np.concatenate([W[:, 2 * l:2 * l + 2] @ Vi[l] for l in range(p.n_landmark)], 1)
    Si = np.linalg.inv(U - Y @ W.T)
    pose = np.zeros((p.n_pose, 3, 3))
    for f in range(n_fixed, p.n_pose):
        o = 3 * (f - n_fixed)
        pose[f] = Si[o:o + 3, o:o + 3]
    ray = np.stack([Vi[l] + Y[:, 2 * l:2 * l + 2].T @ Si @ Y[:, 2 * l:2 * l + 2] for l in range(p.n_landmark)])
    return pose, ray


def block_err(got, ref):
    """Correlation-scaled block error: max over blocks and entries of |got - ref| / sqrt(ref_ii ref_jj); blocks whose
    reference is all zero (fixed frames) must be zero exactly."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    worst = 0.0
    for g, r in zip(got, ref):
        if not r.any():
            assert not g.any()
            continue
        d = np.sqrt(np.diag(r))
        worst = max(worst, float(np.max(np.abs(g - r) / np.outer(d, d))))
    return worst


@functools.lru_cache(maxsize=None)
def synthetic_reference(cfg, loss="linear", f_scale=1.0, n_fixed=1):
    """The dense-inverse blocks of synthetic.make_problem(cfg, seed=0) at its initial state, computed once per
    session (config 2: a 3,365-parameter inverse) and never modified by its users."""
    import synthetic
    p = synthetic.make_problem(cfg, seed=0)
    pose, ray = dense_blocks(p, p.init_ptz, p.init_rays, loss, f_scale, n_fixed)
    pose.setflags(write=False)
    ray.setflags(write=False)
    return p, pose, ray
