"""The crafted systems the covariance kernels (csrc/cov_kernels.hip: k_cov_tile_inv, k_cov_gram, k_cov_cross,
k_cov_resid_part; host side csrc/api_cov.hip) are pinned on in tests/test_cov_cases.py (CPU) and
tests/test_gpu_cov_reference.py (GPU): the real problems of tests/k3_cases.py, whose plans have the shapes the synthetic
configs 1 and 2 lack -- many row tiles, a sparse tile pattern, padding rows, frames straddling a tile edge, the
augmented row alone in the last visited tile (n_aug % 32 == 1) or opening a tile of its own (n_aug % 32 == 0).

  problem(config)       the namespace cov_ref / cov_joint_ref / loss_ref.records take
  inverse(struct)       C = inv(H), H = cov_ref.normal_matrix at the problem's own (ptz0, rays0); read-only, once per session
  inverse32(struct)     the same from the Jacobian rounded to float32 (what fp32 records can at best deliver): e_round
  ref_pivot(pl, struct) the smallest diagonal entry of the Cholesky factor of S = U - W V^-1 W^T in the plan's system order,
                        padding rows left out, in float64 (numpy) and in np.longdouble (k3_ref.chol_ref)
  blocks / groups       a host-side model of ptzba_covariance's packing (cov_prepare, k_cov_gram's first tile)
  strided_selection     a landmark index list with repeats that makes k_cov_gram's grid-stride loop take second blocks
                        whose first tile lies above and below the first block's

Formulas live in cov_ref / cov_joint_ref / loss_ref / k3_ref; nothing is restated here."""
import types

import numpy as np

import cov_ref
import k3_cases as kc
import k3_ref as k3

NB = 32
COV_POSE_F = 10                  # csrc/ptzba_kernels.h: frames of a pose block
COV_RAY_L = NB // 2              # landmarks of a ray block
COV_WG_PER_CU = 2                # csrc/api_cov.hip
COV_WORK_BYTES = 192 << 20       # csrc/api_cov.hip: cap of the Z workspace
RESID_PARTS, RESID_WG = 1024, 256  # csrc/api_cov.hip: n_part = min(1024, ceil(n_rec / 256))

# the configurations of k3_cases the covariance tests use, and the facts each is named for (the issue's table):
# n_aug % 32, lower pattern tiles of the visited rows (count, of how many), padding rows, whether a frame straddles a tile
# edge, the live rows of the last visited tile
CONFIGS = ("one_tile", "chain", "nd2_small", "nd2", "nd2_nd1", "wide")
FACTS = {
    "one_tile": dict(n_aug=33, T=2, pattern=(1, 1), padding=0, straddle=1, last_live=1),
    "chain": dict(n_aug=117, T=4, pattern=(5, 6), padding=0, straddle=2, last_live=21),
    "nd2_small": dict(n_aug=224, T=7, pattern=(8, 21), padding=47, straddle=0, last_live=32),
    "nd2": dict(n_aug=448, T=14, pattern=(36, 91), padding=91, straddle=7, last_live=32),
    "nd2_nd1": dict(n_aug=416, T=13, pattern=(26, 78), padding=59, straddle=8, last_live=32),
    "wide": dict(n_aug=928, T=29, pattern=(308, 406), padding=31, straddle=18, last_live=32),
}


def struct_of(config):
    return kc.CONFIGS[config][0]


def problem(config):
    """The configuration's problem as cov_ref's namespace (the arrays are k3_cases' own: never modified)."""
    struct = struct_of(config)

    def make():
        (u, v, ptz0, rays0, frame, landmark, xy, weight), _ = kc.problem(struct)
        assert weight is None
        return types.SimpleNamespace(n_pose=len(ptz0), n_landmark=len(rays0), frame=frame, landmark=landmark, xy=xy, u=u,
                                     v=v, init_ptz=ptz0, init_rays=rays0)
    return kc._memo(("cov_problem", struct), make)


def normal_matrix(struct, loss="linear", f_scale=1.0):
    def make():
        p = problem(struct)
        H = cov_ref.normal_matrix(p, p.init_ptz, p.init_rays, loss, f_scale)
        H.setflags(write=False)
        return H
    return kc._memo(("cov_H", struct, loss, f_scale), make)


def inverse(struct, loss="linear", f_scale=1.0):
    """C = np.linalg.inv(H) over [3 (n_pose - 1) poses | 2 M rays]: once per session, read-only."""
    def make():
        C = np.linalg.inv(normal_matrix(struct, loss, f_scale))
        C.setflags(write=False)
        return C
    return kc._memo(("cov_C", struct, loss, f_scale), make)


def inverse32(struct):
    """inv(J32^T J32), J32 the oracle's Jacobian (loss_ref.records) rounded to float32 and back: what a linearisation
    from float32 records differs by at the least.  Read-only."""
    def make():
        import loss_ref
        p = problem(struct)
        J = loss_ref.records(p, p.init_ptz, p.init_rays, "linear", 1.0)[0]
        J = J.astype(np.float32).astype(np.float64).tocsc()
        C = np.linalg.inv(np.asarray((J.T @ J).todense()))
        C.setflags(write=False)
        return C
    return kc._memo(("cov_C32", struct), make)


def blocks_of(struct, C):
    p = problem(struct)
    return cov_ref._cut(C, p.n_pose, p.n_landmark, 1)


def reference_blocks(struct, loss="linear", f_scale=1.0):
    """(pose [n_pose, 3, 3], ray [M, 2, 2]) cut from inverse(): read-only."""
    def make():
        pose, ray = blocks_of(struct, inverse(struct, loss, f_scale))
        pose.setflags(write=False)
        ray.setflags(write=False)
        return pose, ray
    return kc._memo(("cov_blocks", struct, loss, f_scale), make)


def e_round(struct):
    """block_err of the float32-Jacobian blocks against the fp64 reference blocks: the rounding of the records alone."""
    def make():
        pose, ray = reference_blocks(struct)
        p32, r32 = blocks_of(struct, inverse32(struct))
        return max(cov_ref.block_err(p32, pose), cov_ref.block_err(r32, ray))
    return kc._memo(("cov_eround", struct), make)


def k2_model_error(struct):
    """block_err of the pose blocks of inv(S~), S~ the reduced system as the fp32 matrix-core K2 computes it
    (k2_ref.model_mf: float32 W | U slots, split-fp16 operands, float32 accumulators), against the fp64 reference.  A
    figure, not a gate: what fp32 records cost before any covariance kernel runs."""
    def make():
        import k2_ref
        p = problem(struct)
        Si = np.linalg.inv(k2_ref.model_mf(kc.problem(struct)[0], 0.0)["S"])
        pose = np.zeros((p.n_pose, 3, 3))
        for f in range(1, p.n_pose):
            pose[f] = Si[3 * f - 3:3 * f, 3 * f - 3:3 * f]
        return cov_ref.block_err(pose, reference_blocks(struct)[0])
    return kc._memo(("cov_k2_model", struct), make)


def fp32_gate(e):
    """max(2e-3, 10 e_round): the rule of tests/test_gpu_k1_paths.py for max |gradient| (2e-3: test_gpu_covariance.TOL[1])."""
    return max(2e-3, 10.0 * e)


# ------------------------------------------------------------------------------------------------
# the smallest pivot
# ------------------------------------------------------------------------------------------------
def reduced_system(struct, dtype=np.float64):
    """S = U - sum_l W_l V_l^-1 W_l^T in frame order from the dense H, formed in `dtype` (landmark by landmark over the
    rows of the frames that see it: W_l is zero elsewhere)."""
    p = problem(struct)
    H = np.asarray(normal_matrix(struct), dtype)
    k = 3 * (p.n_pose - 1)
    S = H[:k, :k].copy()
    for l in range(p.n_landmark):
        c = k + 2 * l
        W = H[:k, c:c + 2]
        rows = np.flatnonzero(np.abs(W).max(axis=1) > 0)
        V = H[c:c + 2, c:c + 2]
        det = V[0, 0] * V[1, 1] - V[0, 1] * V[1, 0]
        Vi = np.array([[V[1, 1], -V[0, 1]], [-V[1, 0], V[0, 0]]], dtype) / det
        Wr = W[rows]
        S[np.ix_(rows, rows)] -= Wr @ Vi @ Wr.T
    return S


def ref_pivot(pl, struct):
    """(float64, np.longdouble) smallest diagonal entry of the Cholesky factor of S permuted to the plan's system order
    with the padding rows left out (they are identity rows: pivot 1, coupled to nothing).  The factor's own diagonal,
    i.e. AFTER the square root -- what k_cov_tile_inv reads from Ldiag."""
    def make():
        rows = k3.frame_rows(pl["pos"])
        order = np.argsort(rows, kind="stable")          # frame-order index of every system row, padding skipped
        n = len(order)
        out = []
        for dtype in (np.float64, np.longdouble):
            S = reduced_system(struct, dtype)[np.ix_(order, order)]
            if dtype is np.float64:
                d = np.diag(np.linalg.cholesky(S))
            else:
                ld = (n + NB - 1) // NB * NB
                A = np.zeros((ld, ld), np.longdouble)
                A[:n, :n] = S
                A[np.arange(n, ld), np.arange(n, ld)] = 1.0
                d = np.diag(k3.chol_ref(A))[:n]
            out.append(d.min())
        return float(out[0]), out[1]
    return kc._memo(("cov_pivot", struct, pl["pos"].tobytes()), make)


def pivot_gate(p64, pld):
    """max(1e-7, 10 x the relative float64 - longdouble difference of the reference)."""
    return max(1e-7, 10.0 * float(abs(np.longdouble(p64) - pld) / pld))


# ------------------------------------------------------------------------------------------------
# shape facts of a plan
# ------------------------------------------------------------------------------------------------
def shape_facts(pl):
    """dict(n_aug, T, pattern=(lower pattern tiles of the visited rows, of how many), padding, straddle, last_live)."""
    n_aug = pl["n_aug"]
    T = (n_aug + NB - 1) // NB
    pos = np.asarray(pl["pos"], np.int64)[1:]
    fill = pl["fill"][:T, :T]
    return dict(n_aug=n_aug, T=T, pattern=(int(np.tril(fill, -1).sum()), T * (T - 1) // 2),
                padding=n_aug - 3 * len(pos), straddle=int(np.sum(pos % NB > NB - 3)),
                last_live=min(NB, n_aug - (T - 1) * NB))


# ------------------------------------------------------------------------------------------------
# the packing model of ptzba_covariance
# ------------------------------------------------------------------------------------------------
def landmark_t0(config, pl, span=True):
    """First non-zero row tile of every landmark's Y columns.  span=True is what k_cov_gram takes: the smallest
    pos[f] // 32 over the free frames between the landmark's first and last frame (lm_meta's range); span=False the
    smallest over the frames that see it.  The first is never later than the second."""
    p = problem(config)
    pos = np.asarray(pl["pos"], np.int64)
    tile = np.where(pos >= 0, pos // NB, np.iinfo(np.int64).max)
    T = (pl["n_aug"] + NB - 1) // NB
    out = np.full(p.n_landmark, T, np.int64)
    if span:
        lo = np.full(p.n_landmark, p.n_pose, np.int64)
        hi = np.full(p.n_landmark, -1, np.int64)
        np.minimum.at(lo, p.landmark, p.frame)
        np.maximum.at(hi, p.landmark, p.frame)
        for l in range(p.n_landmark):
            if hi[l] >= lo[l]:
                out[l] = min(T, tile[lo[l]:hi[l] + 1].min())
    else:
        np.minimum.at(out, p.landmark, np.minimum(tile[p.frame], T))
    return out


def blocks(config, pl, idx=None, poses=True, span=True):
    """The first tile t0 of every 32-column block of a covariance(idx) call in launch order: the pose blocks (free frames
    sorted by pos, 10 per block, t0 of the first), then the ray blocks (16 selected indices per block, the smallest t0 of
    their landmarks).  idx None: every landmark."""
    pos = np.asarray(pl["pos"], np.int64)
    t0 = []
    if poses:
        free = np.sort(pos[pos >= 0])
        t0 += [int(free[k] // NB) for k in range(0, len(free), COV_POSE_F)]
    lt = landmark_t0(config, pl, span)
    idx = np.arange(len(lt)) if idx is None else np.asarray(idx, np.int64)
    t0 += [int(lt[idx[k:k + COV_RAY_L]].min()) for k in range(0, len(idx), COV_RAY_L)]
    return np.array(t0, np.int64)


def max_groups(pl, cus, per_cu=COV_WG_PER_CU):
    """cov_prepare's bound on the workgroups in flight: min(CUs x per_cu, (192 << 20) // (T x 8192))."""
    T = (pl["n_aug"] + NB - 1) // NB
    return max(1, min(cus * per_cu, COV_WORK_BYTES // (T * NB * NB * 8)))


def groups(pl, cus, n_blocks, per_cu=COV_WG_PER_CU):
    return min(max_groups(pl, cus, per_cu), n_blocks)


def stride_jumps(t0, n_groups):
    """(largest rise, largest fall) of t0 between two consecutive blocks of one workgroup (blk, blk + n_groups, ...)."""
    d = t0[n_groups:] - t0[:-n_groups] if len(t0) > n_groups else np.zeros(0, np.int64)
    return (int(d.max()), int(-d.min())) if len(d) else (0, 0)


STRIDE_EXTRA = 8  # ray blocks of the second pass beyond those that follow a pose block


def strided_selection(config, pl, groups_bound):
    """A landmark index list (int32, with repeats) for covariance(idx) with poses: groups_bound + STRIDE_EXTRA ray blocks,
    the last ragged (11 of 16), so that blocks = pose blocks + ray blocks > groups_bound and the workgroups
    0 .. pose blocks + STRIDE_EXTRA - 1 take a second block.  Block b runs in pass b // groups_bound on workgroup
    b % groups_bound; a ray block is filled with landmarks of the highest first tile where pass + workgroup is even and
    with landmarks of the lowest first tile where it is odd, so a workgroup that runs two ray blocks climbs or drops
    between them, and one that starts with a pose block does whichever its pose block leaves open.  The landmarks of a
    class are cycled through, so every block holds other columns."""
    lt = landmark_t0(config, pl, span=True)
    lo_t, hi_t = int(lt.min()), int(lt.max())
    assert hi_t - lo_t >= 2, (config, lo_t, hi_t)
    # (the kernel's first tile is never later than the one over the seeing frames: `high` holds under both)
    low = np.flatnonzero(landmark_t0(config, pl, span=False) == lo_t)
    high = np.flatnonzero(lt == hi_t)
    assert len(low) and len(high), config
    n_pose_blocks = len(blocks(config, pl, idx=[], poses=True))
    n_ray_blocks = groups_bound + STRIDE_EXTRA
    idx = []
    cur = {0: 0, 1: 0}
    for r in range(n_ray_blocks):
        b = n_pose_blocks + r
        odd = (b // groups_bound + b % groups_bound) & 1
        pool = low if odd else high
        n = COV_RAY_L if r + 1 < n_ray_blocks else COV_RAY_L - 5
        idx += [pool[(cur[odd] + q) % len(pool)] for q in range(n)]
        cur[odd] += n
    return np.array(idx, np.int32)


# ------------------------------------------------------------------------------------------------
# joint selections and the records of the residual-scale case
# ------------------------------------------------------------------------------------------------
def joint_selection(config, pl):
    """(frames, landmarks) of the joint case of `config` (the issue's item 5)."""
    p = problem(config)
    pos = np.asarray(pl["pos"], np.int64)
    rng = np.random.default_rng(17)
    if config == "nd2":  # all 119 free frames in reverse order, frame 0 after the first 60, 200 landmarks permuted
        frames = list(range(p.n_pose - 1, 0, -1))
        frames.insert(60, 0)
        landmarks = rng.permutation(p.n_landmark)[:200]
    elif config == "wide":  # 100 frames from both dissection parts and the separator (by pos), 300 landmarks permuted
        by_pos = np.argsort(pos[1:], kind="stable") + 1
        n = len(by_pos)
        take = np.concatenate([by_pos[:34], by_pos[n // 2 - 16:n // 2 + 17], by_pos[-33:]])
        frames = list(rng.permutation(take))
        landmarks = rng.permutation(p.n_landmark)[:300]
    elif config == "nd2_small":  # 5 frames and 5 landmarks whose blocks' first tiles differ
        by_pos = np.argsort(pos[1:], kind="stable") + 1
        frames = [int(by_pos[k]) for k in (len(by_pos) - 1, 0, len(by_pos) // 2, len(by_pos) // 4, 3 * len(by_pos) // 4)]
        lt = landmark_t0(config, pl)
        landmarks = np.argsort(-lt, kind="stable")[:5]  # the five that start latest; the frames start at tile 0
    else:
        raise KeyError(config)
    return np.array(frames, np.int32), np.asarray(landmarks, np.int32)


def joint_blocks(config, pl, frames, landmarks, span=True):
    """First tiles of ptzba_covariance_joint's blocks: the chosen free frames sorted by pos, 10 per block, then the
    landmarks, 16 per block."""
    pos = np.asarray(pl["pos"], np.int64)
    fp = np.sort(pos[np.asarray(frames, np.int64)])
    fp = fp[fp >= 0]
    t0 = [int(fp[k] // NB) for k in range(0, len(fp), COV_POSE_F)]
    lt = landmark_t0(config, pl, span)
    lm = np.asarray(landmarks, np.int64)
    t0 += [int(lt[lm[k:k + COV_RAY_L]].min()) for k in range(0, len(lm), COV_RAY_L)]
    return np.array(t0, np.int64)


SCALE_POSES, SCALE_LANDMARKS = 140, 1900


def scale_problem():
    """140 frames x 1,900 landmarks, every landmark seen once by every frame: 266,000 records -- more than
    1,024 x 256 = 262,144, so k_cov_resid_part's 1,024 workgroups stride to a second record -- no pair repeated (nothing
    merges).  As k2_cases.build: 0.5 px noise, 15 % of the records 8 px off.  Returns (namespace, integer multiplicities
    1..3 per record for the weighted run)."""
    def make():
        import k2_cases as k2c
        segs = [(l, f, 1) for l in range(SCALE_LANDMARKS) for f in range(SCALE_POSES)]
        u, v, ptz0, rays0, frame, landmark, xy, _ = k2c.build(SCALE_POSES, segs, 91)
        p = types.SimpleNamespace(n_pose=SCALE_POSES, n_landmark=SCALE_LANDMARKS, frame=frame, landmark=landmark, xy=xy,
                                  u=u, v=v, init_ptz=ptz0, init_rays=rays0)
        mult = np.random.default_rng(92).integers(1, 4, len(frame)).astype(np.float64)
        mult.setflags(write=False)
        return p, mult
    return kc._memo(("cov_scale_problem",), make)


def scale_residuals():
    """The scalar residuals r [2 R] of scale_problem() at its initial state (loss_ref.records): read-only."""
    def make():
        import loss_ref
        p, _ = scale_problem()
        r = loss_ref.records(p, p.init_ptz, p.init_rays, "linear", 1.0)[1]
        r.setflags(write=False)
        return r
    return kc._memo(("cov_scale_r",), make)


def residual_scale(r, loss, f_scale, n_free, weight=None):
    """sum w rho'(z) r^2 / (2 R - n_free), rho' from loss_ref.weights."""
    import loss_ref
    w = np.ones(len(r)) if weight is None else np.repeat(weight, 2)
    w1 = loss_ref.weights(r, loss, 1.0, f_scale)[2]
    return float(np.sum(w * w1 * r * r)) / (len(r) - n_free)
