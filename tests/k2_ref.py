"""A dense fp64 reference of K2's reduced camera system S | b | g_pose | diag U (k_schur*, k_schur_reduce:
csrc/schur_kernels.hip), the map from the exchange region back to frame order, and a numpy model of the matrix-core
kernel's documented arithmetic (DESIGN §4.2 "Precision / Range").  Test infrastructure: tests/test_k2_ref.py (CPU) and
tests/test_gpu_k2_reference.py (GPU).  The reference shares nothing with the kernels: no tiles, lists, splits or
windows, only the sparse Jacobian of the oracle and the conventions of k1_cases.reference."""
import numpy as np

import k1_cases as kc
from oracle import ptz_oracle as orc

SF, WAVE, SNB, LMAX = 32, 64, 16, 512  # csrc/ptzba_kernels.h: SCHUR_F1, partner chunk, batch, SCHUR_LMAX
MF_FROW = 128.0                         # csrc/schur_kernels.hip
UI = ((0, 1, 2), (1, 3, 4), (2, 4, 5))  # packed index of U_qr in a slot (k_schur_reduce's `ui`)


def _point(problem, ptz, rays):
    u, v, ptz0, rays0, frame, landmark, xy, weight = problem
    return (ptz0 if ptz is None else ptz), (rays0 if rays is None else rays)


def reduced_system(problem, lam, loss="linear", hcurv=1.0, f_scale=1.0, ptz=None, rays=None, D_prev=None):
    """H = J^T diag(w w2) J = [[U, W], [W^T, V]], g = J^T (w w1 r), D = max(D_prev, diag H, 1e-12), frame 0 fixed;
    V~_l = V_l + lam diag(D_ray,l);  S = U - sum_l W_l V~_l^-1 W_l^T;  b = -g_pose + sum_l W_l V~_l^-1 g_l.
    Returns S [3 nf, 3 nf], b, g_pose, dU = diag U, D_pose, D (all of D: free poses, then rays), scale =
    sqrt(U_ii U_jj), and Vinv [n_lm, 3] / W (sparse) / g_ray for the back-substitution; frame order (row 3 (f - 1) + q)."""
    from scipy.sparse import coo_matrix, diags
    u, v, _, _, frame, landmark, xy, weight = problem
    ptz, rays = _point(problem, ptz, rays)
    n_pose, n_lm = len(ptz), len(rays)
    fr, lm = frame.astype(np.int64), landmark.astype(np.int64)
    x = np.concatenate([ptz[1:].reshape(-1), rays.reshape(-1)])
    J = orc.ba_jacobian(x, n_pose, n_lm, u, v, ptz[0], fr, lm).tocsr()
    r = orc.compute_residual_records(np.concatenate([ptz[0], x]), n_pose, u, v, fr, lm, xy)
    w = np.ones(len(r)) if weight is None else np.repeat(weight, 2)
    _, _, w1, w2 = kc._weights(r, loss, hcurv, f_scale)
    H = (J.T @ diags(w * w2) @ J).tocsr()
    g = J.T @ (w * w1 * r)
    n3 = 3 * (n_pose - 1)
    D = np.maximum(H.diagonal(), 1e-12)
    if D_prev is not None:
        D = np.maximum(D, D_prev)
    U = H[:n3, :n3].toarray()
    W = H[:n3, n3:].tocsr()
    Vs = H[n3:, n3:]
    a = Vs.diagonal()[0::2] + lam * D[n3::2]
    c = Vs.diagonal()[1::2] + lam * D[n3 + 1::2]
    bb = np.asarray(Vs.diagonal(1))[0::2]
    det = a * c - bb * bb
    ok = det > 0
    idet = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    Vinv = np.stack([c * idet, -bb * idet, a * idet], -1)
    e = 2 * np.arange(n_lm)
    Vi = coo_matrix((np.concatenate([Vinv[:, 0], Vinv[:, 1], Vinv[:, 1], Vinv[:, 2]]),
                     (np.concatenate([e, e, e + 1, e + 1]), np.concatenate([e, e + 1, e, e + 1]))),
                    shape=(2 * n_lm, 2 * n_lm)).tocsr()
    WV = W @ Vi
    S = U - (WV @ W.T).toarray()
    b = -g[:n3] + WV @ g[n3:]
    dU = np.diag(U).copy()
    return dict(S=S, b=b, g_pose=g[:n3].copy(), dU=dU, D_pose=D[:n3].copy(), D=D, scale=np.sqrt(np.outer(dU, dU)),
                Vinv=Vinv, W=W, g_ray=g[n3:].copy(), n_free_pose=n_pose - 1, singular=int((~ok).sum()))


def solve_step(rs, lam):
    """dx (free poses, then rays) of the damped step from a reduced_system() result."""
    n3 = len(rs["b"])
    dp = np.linalg.solve(rs["S"] + lam * np.diag(rs["D_pose"]), rs["b"])
    t = -rs["g_ray"] - rs["W"].T @ dp
    vi = rs["Vinv"]
    dr = np.stack([vi[:, 0] * t[0::2] + vi[:, 1] * t[1::2], vi[:, 1] * t[0::2] + vi[:, 2] * t[1::2]], -1)
    return np.concatenate([dp, dr.reshape(-1)])


def written_mask(win, n_fixed=1):
    """[3 nf, 3 nf] bool, frame order: the entries k_schur_reduce writes, f1 <= f2 <= frame_win_hi[f1] (and their
    transposes: the view below is symmetric)."""
    n_pose = len(win)
    f = np.arange(n_fixed, n_pose)
    m = (f[None, :] >= f[:, None]) & (f[None, :] <= np.asarray(win)[n_fixed:, None])
    m = m | m.T
    return np.repeat(np.repeat(m, 3, 0), 3, 1)


def region_view(region, pos, ld, n_aug, win, n_fixed=1):
    """The exchange region (include/ptzba.h: ld x ld of S, lower triangle row-major in the system order, then b | g_pose
    | diag U) in frame order.  Block (f1, f2), f1 <= f2, entry (q, r) lies at row pos[f2] + r, column pos[f1] + q, or --
    when the order puts f2 before f1 -- at row pos[f1] + q, column pos[f2] + r (the mirrored store of k_schur_reduce);
    the whole 3 x 3 block of a pair f1 == f2 is stored.  Returns dict(S (symmetric), b, g_pose, dU, mask = the entries
    written (written_mask), mirrored = number of pairs inside the window stored mirrored, aug = row n_aug of S over the
    frames' columns (b^T after a fused prepare, else zero), rest = the largest |value| of the lower triangle's other
    entries below row n_aug (never written: zero)."""
    pos = np.asarray(pos, np.int64)
    n_pose = len(pos)
    Sr = np.asarray(region[:ld * ld]).reshape(ld, ld)
    vec = np.asarray(region[ld * ld:]).reshape(3, ld)
    fp = np.repeat(pos[n_fixed:], 3) + np.tile(np.arange(3), n_pose - n_fixed)  # system row of frame-order index
    I, Jx = np.meshgrid(fp, fp, indexing="ij")
    lowS = Sr[np.maximum(I, Jx), np.minimum(I, Jx)]
    # diagonal blocks: entry (q, r) at row p + r, column p + q (both triangles of the block are stored)
    n3 = len(fp)
    S = lowS.copy()
    for k in range(0, n3, 3):
        S[k:k + 3, k:k + 3] = Sr[fp[k]:fp[k] + 3, fp[k]:fp[k] + 3].T
    mask = written_mask(win, n_fixed)
    f = np.arange(n_fixed, n_pose)
    inwin = (f[None, :] > f[:, None]) & (f[None, :] <= np.asarray(win)[n_fixed:, None])
    mirrored = int((inwin & (pos[f][None, :] < pos[f][:, None])).sum())
    used = np.zeros((ld, ld), bool)
    used[np.maximum(I, Jx), np.minimum(I, Jx)] = True
    for k in range(0, n3, 3):
        used[fp[k]:fp[k] + 3, fp[k]:fp[k] + 3] = True
    low = np.tril(np.ones((ld, ld), bool))
    low[n_aug:] = False
    rest = float(np.abs(Sr[low & ~used]).max()) if (low & ~used).any() else 0.0
    return dict(S=S, b=vec[0][fp], g_pose=vec[1][fp], dU=vec[2][fp], mask=mask, mirrored=mirrored,
                aug=Sr[n_aug][fp] if n_aug < ld else np.zeros(n3), rest=rest)


def expected_view(rs, lam, fused):
    """What region_view shows after a build at damping lam: the raw system (ptzba_build_reduced, or any build with
    PTZBA_NO_FUSED_PREP), or with the fused prepare of a device-driven build: lam D_pose on the pose diagonal and b^T
    in row n_aug."""
    S = rs["S"] + (lam * np.diag(rs["D_pose"]) if fused else 0.0)
    return dict(S=S, b=rs["b"], g_pose=rs["g_pose"], dU=rs["dU"], aug=rs["b"] if fused else np.zeros_like(rs["b"]))


def metrics(got, rs, mask=None):
    """e_S (written entries, against sqrt(U_ii U_jj)), e_b / e_g (against the largest reference entry of the kind: pan
    and tilt rows, f rows), e_dU (entry-wise relative).  got: dict(S, b, g_pose, dU) in frame order."""
    scale = rs["scale"]
    d = np.abs(got["S"] - rs["S"]) / scale
    e_S = float(d.max() if mask is None else d[mask].max())
    f_row = (np.arange(len(rs["b"])) % 3) == 2

    def kind(a, b):
        return float(max(np.abs(a - b)[k].max() / np.abs(b)[k].max() for k in (f_row, ~f_row)))
    return dict(S=e_S, b=kind(got["b"], rs["b"]), g=kind(got["g_pose"], rs["g_pose"]),
                dU=float((np.abs(got["dU"] - rs["dU"]) / rs["dU"]).max()))


FP64_GATE = 1e-10  # the project's fp64 cost gate; n 2^-53 for the <= ~1e4 terms of an entry is ~1e-12


def fp32_gates(model_metrics):
    """Per metric 10 x max(the model's own error against the same reference, 1e-6): the kernel sums in another order
    than the model, so its error is another sample of the same rounding (the rule of test_gpu_k1_paths._gmax_gate)."""
    return {k: 10.0 * max(v, 1e-6) for k, v in model_metrics.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the arithmetic of k_schur_mfp
# ---------------------------------------------------------------------------------------------------------------------
def rtz16(x):
    """float32 -> float16 rounded toward zero (v_cvt_pkrtz_f16_f32): nearest-even, then one step towards zero where the
    magnitude grew (subnormals included; a value beyond the range becomes +-65504)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    grew = np.abs(h.astype(np.float32)) > np.abs(x)
    return np.where(grew, np.nextafter(h, np.float16(0)), h)


def split16(x):
    """x (float32) -> (hi, lo) as float32 arrays holding fp16 values: hi = rtz(x), lo = rtz(x - hi)."""
    x = np.asarray(x, np.float32)
    hi = rtz16(x).astype(np.float32)
    lo = rtz16(x - hi).astype(np.float32)
    return hi, lo


def tile_plan(n_pose, frame, landmark, n_fixed=1):
    """The tiles, lists and splits ptzba_set_problem builds (csrc/problem_layout.cpp layout_k2), restated: a list of
    dict(f1b, chunk, lms (ascending), splits [(a0, a1)]).  A landmark enters chunk c > 0 when it sees a frame of the
    chunk; split weight = the smallest >= 256 whose item count fits the target (chunk-0 landmarks weigh 6, others 4)."""
    key = np.unique(landmark.astype(np.int64) * n_pose + frame.astype(np.int64))
    seg_lm, seg_fr = key // n_pose, key % n_pose
    n_lm = int(seg_lm.max()) + 1
    last = np.zeros(n_lm, np.int64)
    np.maximum.at(last, seg_lm, seg_fr)
    tiles = []
    for f1b in range(n_fixed, n_pose, SF):
        un = np.unique(seg_lm[(seg_fr >= f1b) & (seg_fr < f1b + SF)])
        hi = max(f1b, int(last[un].max())) if len(un) else f1b
        for c in range((hi - f1b) // WAVE + 1):
            c_lo = f1b + WAVE * c
            lst = un if c == 0 else np.intersect1d(un, np.unique(seg_lm[(seg_fr >= c_lo) & (seg_fr <= c_lo + WAVE - 1)]))
            if len(lst):
                tiles.append(dict(f1b=f1b, chunk=c, lms=lst))
    wt = [len(t["lms"]) * (6 if t["chunk"] == 0 else 4) for t in tiles]
    total_w = sum(wt)
    target = min(256, max(64, (512 * total_w) // 480000))

    def items_for(sw):
        return sum(max(-(-w // sw), -(-len(t["lms"]) // LMAX)) for t, w in zip(tiles, wt))
    lo, hi = 256, max(256, total_w)
    if items_for(lo) <= target:
        hi = lo
    else:
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if items_for(mid) <= target:
                hi = mid
            else:
                lo = mid
    for t, w in zip(tiles, wt):
        n = len(t["lms"])
        parts = max(-(-w // hi), -(-n // LMAX))
        t["splits"] = [(n * p // parts, n * (p + 1) // parts) for p in range(parts)]
    return tiles


def plan_summary(tiles, n_pose):
    """What ptzba_k2_info / ptzba_k2_tile_info report, from tile_plan()."""
    nl = [a1 - a0 for t in tiles for a0, a1 in t["splits"]]
    ns = [len(t["splits"]) for t in tiles]
    return dict(items=len(nl), nl_min=min(nl), nl_max=max(nl), tiles=len(tiles), splits_min=min(ns), splits_max=max(ns),
                tiles_ge9_splits=sum(n >= 9 for n in ns), chunk_max=max(t["chunk"] for t in tiles),
                tiles_past_n_pose=sum(t["f1b"] + WAVE * (t["chunk"] + 1) > n_pose for t in tiles))


MUTATIONS = ("no_lo_hi", "drop_last_of_16k1", "drop_split9", "no_frow_backscale", "mirror_untransposed", "chunk0_only",
             "skip_batch", "stale_batch")


def model_mf(problem, lam, loss="linear", hcurv=1.0, f_scale=1.0, ptz=None, rays=None, D_prev=None, win=None,
             mutate=None, pos=None):
    """S | b | g_pose | dU as the matrix-core kernel computes them (frame order, the written entries; S symmetric):
    J and r rounded to float32 per record, the W | U | g_pose slots rounded to float32; V~^-1 and V~^-1 g in fp64,
    converted to float32; g_l = 2^(e / 2) (C division), e = frexp(V~^-1_00 + V~^-1_11); W rows times g_l, Y = -(W / g_l)
    V~^-1 in float32 (fmaf), f rows times MF_FROW; every operand hi = rtz16(x), lo = rtz16(x - hi); per batch of 16
    landmarks lo.hi, hi.lo, hi.hi (each a 32-term dot product, exact) added to a float32 accumulator in that order over
    the item's batches; back-scaled, stored float32, the tile's splits summed in fp64.  Diagonal terms: float32 sums
    per (list position mod 16, frame) over the item's batches, then fp64.
    mutate: one of MUTATIONS (a deliberately wrong kernel: tests/test_k2_ref.py shows that the gates notice);
    mirror_untransposed needs pos (system positions); skip_batch and stale_batch are hand-off faults of the operand
    ring in one work item of more than three batches: its third batch is never accumulated, or its products are
    formed from the first batch's operands (a buffer consumed before its re-fill).  Also returns max_hi (largest |hi|), sub_lo (share of non-zero
    operands whose lo is subnormal in fp16) and the tile plan."""
    u, v, _, _, frame, landmark, xy, weight = problem
    ptz, rays = _point(problem, ptz, rays)
    n_pose, n_lm = len(ptz), len(rays)
    fr, lm = frame.astype(np.int64), landmark.astype(np.int64)
    f32 = np.float32
    J = orc.record_jacobian(u, v, ptz[fr], rays[lm]).astype(f32).astype(np.float64)  # [R, 2, 5]
    r = orc.compute_residual_records(np.concatenate([ptz.reshape(-1), rays.reshape(-1)]), n_pose, u, v, fr, lm, xy)
    r = r.astype(f32).astype(np.float64)
    _, _, w1, w2 = kc._weights(r, loss, hcurv, f_scale)
    wr = np.ones(len(fr)) if weight is None else np.asarray(weight, np.float64)
    hw = wr[:, None] * w2.reshape(-1, 2)
    gw = wr[:, None] * w1.reshape(-1, 2) * r.reshape(-1, 2)
    # per-record blocks, summed per (landmark, frame) slot and per landmark
    Jp, Jr = J[:, :, :3], J[:, :, 3:]
    Wrec = np.einsum("nk,nkq,nkd->nqd", hw, Jp, Jr)
    Urec = np.einsum("nk,nkq,nkr->nqr", hw, Jp, Jp)
    Urec = np.stack([Urec[:, 0, 0], Urec[:, 0, 1], Urec[:, 0, 2], Urec[:, 1, 1], Urec[:, 1, 2], Urec[:, 2, 2]], -1)
    grec = np.einsum("nk,nkq->nq", gw, Jp)
    Vrec = np.einsum("nk,nkd,nke->nde", hw, Jr, Jr)
    glrec = np.einsum("nk,nkd->nd", gw, Jr)
    def slot_sum(idx, x, n):  # sum the records' rows x [R, k] per index -> [n, k]
        return np.stack([np.bincount(idx, x[:, k], n) for k in range(x.shape[1])], -1)
    Wd = slot_sum(lm * n_pose + fr, Wrec.reshape(-1, 6), n_lm * n_pose).astype(f32).reshape(n_lm, n_pose, 3, 2)
    UGd = slot_sum(lm * n_pose + fr, np.concatenate([Urec, grec], -1), n_lm * n_pose).astype(f32).reshape(n_lm, n_pose, 9)
    V = slot_sum(lm, Vrec.reshape(-1, 4), n_lm).reshape(n_lm, 2, 2)
    gl = slot_sum(lm, glrec, n_lm)
    seen = np.zeros((n_lm, n_pose), bool)
    seen[lm, fr] = True
    first = np.where(seen.any(1), seen.argmax(1), 0)
    last = np.where(seen.any(1), n_pose - 1 - seen[:, ::-1].argmax(1), -1)
    D_ray = np.maximum(np.stack([V[:, 0, 0], V[:, 1, 1]], -1), 1e-12)
    if D_prev is not None:
        D_ray = np.maximum(D_ray, np.asarray(D_prev)[3 * (n_pose - 1):].reshape(-1, 2))
    a, c, bb = V[:, 0, 0] + lam * D_ray[:, 0], V[:, 1, 1] + lam * D_ray[:, 1], V[:, 0, 1]
    det = a * c - bb * bb
    ok = det > 0
    idet = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    vi = np.stack([c * idet, -bb * idet, a * idet], -1)
    vg = np.stack([vi[:, 0] * gl[:, 0] + vi[:, 1] * gl[:, 1], vi[:, 1] * gl[:, 0] + vi[:, 2] * gl[:, 1]], -1).astype(f32)
    ex = np.frexp(vi[:, 0] + vi[:, 2])[1]
    gsc = np.ldexp(1.0, np.trunc(ex / 2.0).astype(np.int64)).astype(f32)  # C's e / 2 truncates toward zero
    vi32 = vi.astype(f32)

    if win is None:
        import ptzba
        win = ptzba.frame_coupling_window(n_pose, frame, landmark)
    tiles = tile_plan(n_pose, frame, landmark)
    n3 = 3 * (n_pose - 1)
    S = np.zeros((n3, n3))
    dsum = np.zeros((n_pose, 12))
    frow_y = np.array([1.0, 1.0, MF_FROW], f32)
    stats = dict(max_hi=0.0, nz=0, sub=0)
    did = dict.fromkeys(MUTATIONS, False)

    def note(hi, lo, x):
        stats["max_hi"] = max(stats["max_hi"], float(np.abs(hi).max(initial=0.0)))
        nz = x != 0
        stats["nz"] += int(nz.sum())
        stats["sub"] += int((nz & (np.abs(lo) < 2.0 ** -14) & (lo != 0)).sum())

    for t in tiles:
        f1b, chunk = t["f1b"], t["chunk"]
        if mutate == "chunk0_only" and chunk > 0:
            did[mutate] = True
            continue
        f2base = f1b + WAVE * chunk
        F1, F2 = np.arange(f1b, f1b + SF), np.arange(f2base, f2base + WAVE)
        T = np.zeros((3 * SF, 3 * WAVE))
        for si, (a0, a1) in enumerate(t["splits"]):
            L = t["lms"][a0:a1]
            if mutate == "drop_split9" and si == 8 and not did[mutate]:
                did[mutate] = True
                continue
            if mutate == "drop_last_of_16k1" and len(L) % SNB == 1 and len(L) > 1 and not did[mutate]:
                did[mutate] = True
                L = L[:-1]
            nl = len(L)

            def rows(F):  # W slots of the list's landmarks over the frames F, zero outside [first, last] or n_pose
                inr = (F[None, :] >= first[L, None]) & (F[None, :] <= last[L, None])
                return np.where(inr[:, :, None, None], Wd[L][:, np.minimum(F, n_pose - 1)], f32(0)), inr
            W1, in1 = rows(F1)
            W2, _ = rows(F2)
            gi = (f32(1) / gsc[L])[:, None]
            v0, v1, v2 = vi32[L, 0, None] * gi, vi32[L, 1, None] * gi, vi32[L, 2, None] * gi  # [nl, 1]
            Y = np.empty((nl, SF, 3, 2), f32)
            for q in range(3):
                w0, w1_ = W1[:, :, q, 0], W1[:, :, q, 1]
                # fmaf(W0, v0, W1 * v1): the product W1 v1 rounded, the fused sum rounded once
                y0 = (w0.astype(np.float64) * v0 + (w1_ * v1).astype(f32)).astype(f32)
                y1 = (w0.astype(np.float64) * v1 + (w1_ * v2).astype(f32)).astype(f32)
                Y[:, :, q, 0] = -frow_y[q] * y0
                Y[:, :, q, 1] = -frow_y[q] * y1
            B = (W2 * gsc[L][:, None, None, None] * frow_y[None, None, :, None]).astype(f32)
            Yh, Yl = split16(Y)
            Bh, Bl = split16(B)
            note(Yh, Yl, Y)
            note(Bh, Bl, B)
            # operand matrices [k = (landmark, d)] x [row = q * 32 + i] and [col = r * 64 + f2]
            def mat(X, n):
                return X.transpose(0, 3, 2, 1).reshape(nl * 2, 3 * n).astype(np.float64)
            Ah, Al, Gh, Gl = mat(Yh, SF), mat(Yl, SF), mat(Bh, WAVE), mat(Bl, WAVE)
            acc = np.zeros((3 * SF, 3 * WAVE), f32)
            dacc = np.zeros((SNB, SF, 12), f32)
            ring_fault = mutate in ("skip_batch", "stale_batch") and nl > 3 * SNB and not did[mutate]
            for p in range(0, nl, SNB):
                k0, k1 = 2 * p, 2 * min(p + SNB, nl)
                if ring_fault and p == 2 * SNB:  # (the products only: the diagonal terms do not pass through the ring)
                    did[mutate] = True
                    k0, k1 = (0, 0) if mutate == "skip_batch" else (0, 2 * SNB)
                if mutate != "no_lo_hi":
                    acc = (acc + (Al[k0:k1].T @ Gh[k0:k1]).astype(f32)).astype(f32)
                else:
                    did[mutate] = True
                acc = (acc + (Ah[k0:k1].T @ Gl[k0:k1]).astype(f32)).astype(f32)
                acc = (acc + (Ah[k0:k1].T @ Gh[k0:k1]).astype(f32)).astype(f32)
                if chunk == 0:
                    Lb = L[p:p + SNB]
                    inb = in1[p:p + SNB]
                    ug = np.where(inb[:, :, None], UGd[Lb][:, np.minimum(F1, n_pose - 1)], f32(0))
                    wb = W1[p:p + SNB]
                    g0, g1 = vg[Lb, 0, None, None], vg[Lb, 1, None, None]
                    wv = (wb[..., 0].astype(np.float64) * g0 + (wb[..., 1] * g1).astype(f32)).astype(f32)
                    term = np.concatenate([ug, wv], -1)
                    dacc[:len(Lb)] = (dacc[:len(Lb)] + term).astype(f32)
            back = np.array([1.0, 1.0, 1.0 / MF_FROW])
            if mutate == "no_frow_backscale":
                did[mutate] = True
                back = np.ones(3)
            acc = acc.reshape(3, SF, 3, WAVE) * back[:, None, None, None].astype(f32) * back[None, None, :, None].astype(f32)
            T += acc.reshape(3 * SF, 3 * WAVE).astype(f32).astype(np.float64)
            if chunk == 0:
                dd = np.zeros((SF, 12))
                for j in range(SNB):
                    dd += dacc[j].astype(np.float64)
                ok1 = F1 < n_pose
                dsum[F1[ok1]] += dd[ok1]
        T4 = T.reshape(3, SF, 3, WAVE)
        for i, f1 in enumerate(F1):
            if f1 >= n_pose:
                break
            j = np.flatnonzero((F2 >= f1) & (F2 <= win[f1]) & (F2 < n_pose))
            if len(j):
                blk = T4[:, i][:, :, j]  # [q, r, f2]
                cols = (3 * (F2[j] - 1)[None, :] + np.arange(3)[:, None])  # [r, f2]
                S[3 * (f1 - 1):3 * f1][:, cols] = blk
    free = np.arange(1, n_pose)
    for q in range(3):
        for rr in range(3):
            S[3 * (free - 1) + q, 3 * (free - 1) + rr] += dsum[free, UI[q][rr]]
    if mutate == "mirror_untransposed":
        assert pos is not None
        done = False
        for f1 in free:
            for f2 in range(f1 + 1, min(int(win[f1]), n_pose - 1) + 1):
                blk = S[3 * (f1 - 1):3 * f1, 3 * (f2 - 1):3 * f2]
                if pos[f2] < pos[f1] and np.abs(blk).max() > 0:
                    S[3 * (f1 - 1):3 * f1, 3 * (f2 - 1):3 * f2] = blk.T.copy()
                    done = True
                    break
            if done:
                break
        did[mutate] = done
    iu = np.triu_indices(n3, 1)
    S[(iu[1], iu[0])] = S[iu]  # blocks were written for f2 >= f1: mirror the strict upper triangle
    d = dsum[1:]
    out = dict(S=S, b=(-d[:, 6:9] + d[:, 9:12]).reshape(-1), g_pose=d[:, 6:9].reshape(-1).copy(),
               dU=d[:, [0, 3, 5]].reshape(-1).copy(), max_hi=stats["max_hi"],
               sub_lo=stats["sub"] / max(stats["nz"], 1), tiles=tiles, applied=(did[mutate] if mutate else None))
    return out
