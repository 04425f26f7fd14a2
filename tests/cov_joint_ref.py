"""CPU reference of the joint posterior covariance (shared by test_cov_joint_cpu.py and test_gpu_cov_joint.py): the
sub-matrix of np.linalg.inv(H) cut at chosen parameters in the chosen order, H from cov_ref.normal_matrix (or
ray_prior_ref.normal_matrix with priors); the same matrix through the Schur form scale * (D + Z^T Z), L Z = [E | -Y];
and the metric max |got_ij - ref_ij| / sqrt(ref_ii ref_jj) over the whole matrix."""
import functools

import numpy as np


def param_index(p, frames, landmarks, n_fixed=1, dead=()):
    """H's parameter index of every chosen parameter, frames first (3 each), then landmarks (2 each); -1 for the
    parameters of a fixed frame and of a landmark in `dead` (no records: not part of H's live part)."""
    k = 3 * (p.n_pose - n_fixed)
    idx = []
    for f in np.asarray(frames, np.int64).reshape(-1):
        idx += [3 * (f - n_fixed) + x if f >= n_fixed else -1 for x in range(3)]
    for l in np.asarray(landmarks, np.int64).reshape(-1):
        idx += [k + 2 * l + x if l not in dead else -1 for x in range(2)]
    return np.array(idx, np.int64)


def cut(C, idx):
    """C[idx][:, idx] with all-zero rows and columns where idx < 0."""
    idx = np.asarray(idx)
    live = idx >= 0
    out = np.zeros((len(idx), len(idx)))
    out[np.ix_(live, live)] = C[np.ix_(idx[live], idx[live])]
    return out


def joint_err(got, ref):
    """max |got_ij - ref_ij| / sqrt(ref_ii ref_jj); rows and columns whose reference diagonal is zero (a fixed frame, a
    landmark without records) must be zero exactly."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.ndim == 2 and got.shape[0] == got.shape[1], (got.shape, ref.shape)
    d = np.diag(ref)
    live = d > 0
    assert not got[~live].any() and not got[:, ~live].any()
    assert not ref[~live].any() and not ref[:, ~live].any()
    if not live.any():
        return 0.0
    s = np.sqrt(d[live])
    return float(np.max(np.abs(got - ref)[np.ix_(live, live)] / np.outer(s, s)))


def schur_joint(H, p, frames, landmarks, n_fixed=1, sign=-1.0):
    """The joint covariance through the reduced system: S = U - sum_l W_l V_l^-1 W_l^T = L L^T (numpy's Cholesky),
    B = [E_F | sign Y_L], Cov = D + Z^T Z with L Z = B and D = blockdiag(0, V_l^-1).  sign = -1 is the formula;
    +1 is the variant that flips every pose-ray entry."""
    k = 3 * (p.n_pose - n_fixed)
    U, W = H[:k, :k], H[:k, k:]
    M = p.n_landmark
    Vi = np.zeros((M, 2, 2))
    for l in range(M):
        Vi[l] = np.linalg.inv(H[k + 2 * l:k + 2 * l + 2, k + 2 * l:k + 2 * l + 2])
    Y = np.concatenate([W[:, 2 * l:2 * l + 2] @ Vi[l] for l in range(M)], 1)
    L = np.linalg.cholesky(U - Y @ W.T)
    frames = np.asarray(frames, np.int64).reshape(-1)
    landmarks = np.asarray(landmarks, np.int64).reshape(-1)
    n = 3 * len(frames) + 2 * len(landmarks)
    B = np.zeros((k, n))
    D = np.zeros((n, n))
    for q, f in enumerate(frames):
        if f >= n_fixed:
            for x in range(3):
                B[3 * (f - n_fixed) + x, 3 * q + x] = 1.0
    o = 3 * len(frames)
    for q, l in enumerate(landmarks):
        B[:, o + 2 * q:o + 2 * q + 2] = sign * Y[:, 2 * l:2 * l + 2]
        D[o + 2 * q:o + 2 * q + 2, o + 2 * q:o + 2 * q + 2] = Vi[l]
    Z = np.linalg.solve(L, B)  # (dense solve against the triangular factor)
    return D + Z.T @ Z


@functools.lru_cache(maxsize=None)
def synthetic_inverse(cfg, loss="linear", f_scale=1.0, n_fixed=1):
    """(problem, np.linalg.inv(H)) of synthetic.make_problem(cfg, seed=0) at its initial state, computed once per
    session (config 2: a 3,365-parameter inverse, ~5 s) and never modified by its users."""
    import synthetic
    import cov_ref
    p = synthetic.make_problem(cfg, seed=0)
    C = np.linalg.inv(cov_ref.normal_matrix(p, p.init_ptz, p.init_rays, loss, f_scale, n_fixed))
    C.setflags(write=False)
    return p, C
