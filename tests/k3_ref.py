"""Reference and arithmetic model of K3, the reduced-system solver (csrc/chol_kernels.hip: k_chol_prepare, k_chol_step,
k_tile_inv / k_tile_inv_list and the back-substitution kernels).  Host only; tests/test_k3_ref.py (CPU) and
tests/test_gpu_k3_reference.py (GPU).

  region_pack   the inverse of k2_ref.region_view: a frame-order system into the exchange region's layout
  augmented     what k_chol_prepare makes of the region: pose damping, identity padding, b^T in row n_aug with 1e300 on
                its diagonal, identity below
  chol_ref / solve_ref   np.longdouble (eps 1.08e-19), tile by tile, zero tiles skipped; shares nothing with the plan
  model         the project's "same arithmetic, other summation order" model: chol_plan_exec.replay (fp64 numpy, the
                library's own plan) for the factor, explicit fp64 tile inverses M_kt = inv(L_kt,kt) and a back-substitution
                x_kt = M_kt^T r_kt in the summation pattern of the kernel form (right-looking: lookahead; left-looking;
                blocks of four columns: blocked / persistent)
  metrics       evaluated in np.longdouble (see the function)
"""
import numpy as np

import chol_plan_exec as cpe

NB = cpe.NB
LD = np.longdouble
U = 2.0 ** -53
AUG_DIAG = 1e300  # csrc/chol_kernels.hip


def frame_rows(pos, n_fixed=1):
    pos = np.asarray(pos, np.int64)
    return np.repeat(pos[n_fixed:], 3) + np.tile(np.arange(3), len(pos) - n_fixed)


def region_pack(S, b, dU, pos, ld, n_aug, win, n_fixed=1, g=None):
    """The exchange region (ld * ld of S, then b | g_pose | dU; include/ptzba.h) holding the frame-order system S
    (symmetric, support inside k2_ref.written_mask(win)): the lower triangle in the system order -- block (f1, f2),
    f1 <= f2, entry (q, r) at row pos[f2] + r, column pos[f1] + q, or mirrored (row pos[f1] + q, column pos[f2] + r)
    where the order puts f2 before f1 --, both triangles of the diagonal 3 x 3 blocks, zero everywhere else."""
    import k2_ref as kr
    fp = frame_rows(pos, n_fixed)
    assert fp.max() < n_aug and len(fp) == S.shape[0]
    mask = kr.written_mask(win, n_fixed)
    assert np.all(S[~mask] == 0.0)
    Sr = np.zeros((ld, ld))
    a, c = np.nonzero(mask)
    I, J = fp[a], fp[c]
    Sr[np.maximum(I, J), np.minimum(I, J)] = S[a, c]
    for k in range(0, len(fp), 3):
        Sr[fp[k]:fp[k] + 3, fp[k]:fp[k] + 3] = S[k:k + 3, k:k + 3].T
    vec = np.zeros((3, ld))
    vec[0][fp] = b
    if g is not None:
        vec[1][fp] = g
    vec[2][fp] = dU
    return np.concatenate([Sr.reshape(-1), vec.reshape(-1)])


def augmented(S, b, pos, ld, n_aug, lam=0.0, D=None, n_fixed=1):
    """The symmetric ld x ld system k_chol_prepare leaves (fp64, formed as the kernel forms it: S_ii + lam * D_i)."""
    fp = frame_rows(pos, n_fixed)
    A = np.zeros((ld, ld))
    A[np.ix_(fp, fp)] = S
    if lam != 0.0:
        A[fp, fp] = A[fp, fp] + lam * D
    pad = np.ones(ld, bool)
    pad[fp] = False
    pad[n_aug] = False
    A[pad, pad] = 1.0
    A[n_aug, fp] = b
    A[fp, n_aug] = b
    A[n_aug, n_aug] = AUG_DIAG
    return A


def _tiles_nz(A):
    T = A.shape[0] // NB
    return np.abs(A).reshape(T, NB, T, NB).max(axis=(1, 3)) > 0


def _potrf_ld(D):
    L = np.zeros_like(D)
    D = D.copy()
    for j in range(NB):
        d = D[j, j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = D[j + 1:, j] / L[j, j]
        D[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L


def _trsm_ld(Tt, Lkk):
    """X with X Lkk^T = Tt."""
    X = np.zeros_like(Tt)
    for j in range(NB):
        X[:, j] = (Tt[:, j] - X[:, :j] @ Lkk[j, :j]) / Lkk[j, j]
    return X


def chol_ref(A):
    """Lower Cholesky factor of the symmetric A (ld x ld, ld a multiple of 32) in np.longdouble; left-looking by tile
    column, structurally zero tiles skipped."""
    A = np.asarray(A, LD)
    T = A.shape[0] // NB
    nz = np.tril(_tiles_nz(A))
    L = np.zeros_like(A)

    def t(M, i, j):
        return M[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB]
    for k in range(T):
        ps = [p for p in range(k) if nz[k, p]]
        D = t(A, k, k).copy()
        for p in ps:
            D -= t(L, k, p) @ t(L, k, p).T
        Lkk = _potrf_ld(D)
        t(L, k, k)[:] = Lkk
        for i in range(k + 1, T):
            pi = [p for p in ps if nz[i, p]]
            if not nz[i, k] and not pi:
                continue
            Tt = t(A, i, k).copy()
            for p in pi:
                Tt -= t(L, i, p) @ t(L, k, p).T
            t(L, i, k)[:] = _trsm_ld(Tt, Lkk)
            nz[i, k] = True
    return L


def backsub_ref(L, n_aug):
    """x with L[:n, :n]^T x = y, y = row n_aug of L (np.longdouble)."""
    y = L[n_aug, :n_aug]
    x = np.zeros(n_aug, LD)
    for i in range(n_aug - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:n_aug, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_ref(A, b):
    """x = A^-1 b in np.longdouble, A symmetric positive definite [n, n] (any n): through chol_ref of the augmented system."""
    n = len(b)
    ld = (n + 1 + NB - 1) // NB * NB
    Aa = np.zeros((ld, ld), LD)
    Aa[:n, :n] = A
    Aa[n, :n] = Aa[:n, n] = b
    Aa[n, n] = AUG_DIAG
    Aa[np.arange(n + 1, ld), np.arange(n + 1, ld)] = 1.0
    return backsub_ref(chol_ref(Aa), n)


def reference(A, n_aug):
    L = chol_ref(A)
    return dict(L=L, y=L[n_aug, :n_aug].copy(), x=backsub_ref(L, n_aug))


BS_FORMS = ("right", "left", "block")
BSB_P = 4  # csrc/ptzba_kernels.h: columns of a block of the blocked back-substitution


def model(A, tasks, level_off, n_aug, bs_form):
    """dict(L [ld, ld] lower with the diagonal tiles, Ldiag / Minv [T, 32, 32], y, x [n_aug]) in fp64: the plan replayed
    by chol_plan_exec, M_kt = numpy's inverse of the replayed diagonal tile, x_kt = M_kt^T r_kt with r_kt summed as the
    kernel form sums it."""
    assert bs_form in BS_FORMS
    Lf, Ld = cpe.replay(A, tasks, level_off)
    ld = A.shape[0]
    T = ld // NB
    Ldiag = np.stack([Ld[k] for k in range(T)])
    Minv = np.stack([np.linalg.inv(Ld[k]) for k in range(T)])
    nz = np.tril(_tiles_nz(Lf), -1)

    def t(i, j):
        return Lf[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB]
    r = np.zeros(ld)
    r[:n_aug] = Lf[n_aug, :n_aug]
    y = r[:n_aug].copy()
    x = np.zeros(ld)
    Lx = Lf.copy()
    Lx[n_aug:] = 0.0  # rows from n_aug on carry no unknown (the kernels' right-hand side is zero there)
    taug = (n_aug - 1) // NB

    def tx(i, j):
        return Lx[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB]

    def sl(k):
        return slice(k * NB, (k + 1) * NB)
    cols = list(range(taug, -1, -1))
    if bs_form == "right":
        for kt in cols:
            x[sl(kt)] = Minv[kt].T @ r[sl(kt)]
            for j in range(kt):
                if nz[kt, j]:
                    r[sl(j)] -= tx(kt, j).T @ x[sl(kt)]
    elif bs_form == "left":
        for kt in cols:
            s = np.zeros(NB)
            for i in range(kt + 1, taug + 1):
                if nz[i, kt]:
                    s += tx(i, kt).T @ x[sl(i)]
            x[sl(kt)] = Minv[kt].T @ (r[sl(kt)] - s)
    else:
        for g0 in range(0, len(cols), BSB_P):
            grp = cols[g0:g0 + BSB_P]
            for a, kt in enumerate(grp):
                s = np.zeros(NB)
                for i in grp[:a]:
                    if nz[i, kt]:
                        s += tx(i, kt).T @ x[sl(i)]
                x[sl(kt)] = Minv[kt].T @ (r[sl(kt)] - s)
            for j in range(grp[-1]):
                s, any_ = np.zeros(NB), False
                for kt in grp:
                    if nz[kt, j]:
                        s += tx(kt, j).T @ x[sl(kt)]
                        any_ = True
                if any_:
                    r[sl(j)] -= s
    x[n_aug:] = 0.0
    return dict(L=Lf, Ldiag=Ldiag, Minv=Minv, y=y, x=x[:n_aug].copy())


def assemble(region_S, Ldiag, ld):
    """The factor as the kernels leave it: off-diagonal tiles from the region, diagonal tiles from Ldiag."""
    L = np.tril(np.asarray(region_S).reshape(ld, ld)).copy()
    for k in range(ld // NB):
        L[k * NB:(k + 1) * NB, k * NB:(k + 1) * NB] = Ldiag[k]
    return L


def factor_y(L, n_aug):
    return L[n_aug, :n_aug].copy()


def metrics(A, n_aug, pose_rows, ref, L, Minv, x):
    """All in np.longdouble; A = augmented() (ld x ld), ref = reference(A, n_aug), L the assembled factor (diagonal
    tiles included), Minv [T, 32, 32], x = dpose[:n_aug].
      e_bw   max over the lower triangle, rows < n_aug, of |L L^T - A|_ij / sqrt(A_ii A_jj)
      e_L    max |L - L_ref|_ij / sqrt(A_ii), rows < n_aug
      e_y    row n_aug against its largest reference entry
      e_Minv max |Minv_k Ldiag_k - I| over the tile columns that hold pose rows (rows and columns below n_aug)
      e_res  max_i |A x - b|_i / (|L_ref| |L_ref^T| |x|)_i over the rows where the denominator is not zero
      e_x    max |x - x_ref| / max |x_ref|"""
    ld = A.shape[0]
    T = ld // NB
    Aq, Lq = np.asarray(A, LD), np.asarray(L, LD)
    d = np.sqrt(np.diag(Aq))
    nzL = np.tril(_tiles_nz(L))
    nzA = np.tril(_tiles_nz(A))

    def t(M, i, j):
        return M[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB]
    e_bw = LD(0)
    for i in range(T):
        rows = np.arange(i * NB, (i + 1) * NB)
        keep = rows < n_aug
        if not keep.any():
            continue
        for j in range(i + 1):
            ps = [p for p in range(j + 1) if nzL[i, p] and nzL[j, p]]
            if not ps and not nzA[i, j]:
                continue
            R = -t(Aq, i, j)
            for p in ps:
                R = R + t(Lq, i, p) @ t(Lq, j, p).T
            R = np.abs(R) / np.outer(d[rows], d[j * NB:(j + 1) * NB])
            if i == j:
                R = np.tril(R)
            e_bw = max(e_bw, R[keep].max())
    Lr = ref["L"]
    e_L = (np.abs(Lq[:n_aug, :n_aug] - Lr[:n_aug, :n_aug]) / d[:n_aug, None]).max()
    yr = ref["y"]
    e_y = np.abs(Lq[n_aug, :n_aug] - yr).max() / np.abs(yr).max()
    tiles = sorted({int(r) // NB for r in pose_rows})
    e_M = LD(0)
    for k in tiles:  # (the augmented row's tile: its leading block, the rows below n_aug -- both tiles are triangular)
        m = min(NB, n_aug - k * NB)
        e_M = max(e_M, np.abs(np.asarray(Minv[k], LD)[:m, :m] @ t(Lq, k, k)[:m, :m] - np.eye(m, dtype=LD)).max())
    xq = np.asarray(x, LD)
    bq = Aq[n_aug, :n_aug]
    res = np.abs(Aq[:n_aug, :n_aug] @ xq - bq)
    aL = np.abs(Lr[:n_aug, :n_aug])
    den = aL @ (aL.T @ np.abs(xq))
    ok = den > 0
    e_res = (res[ok] / den[ok]).max()
    e_x = np.abs(xq - ref["x"]).max() / np.abs(ref["x"]).max()
    return dict(bw=float(e_bw), L=float(e_L), y=float(e_y), Minv=float(e_M), res=float(e_res), x=float(e_x))


def gates(model_metrics, ld):
    """Gate 1 on e_bw (derived, hard): 2 (ld + 1) u -- Higham, Accuracy and Stability, Thm 10.3 with |L| |L^T|_ij <=
    sqrt(a_ii a_jj) (1 + O(gamma)); the factor 2 covers the second-order term and rsq_fast's 0.6 ulp.  Gate 2 and the
    others: 10 x max(the model's own value, a floor): the margin of the K2 gates for another summation order."""
    m = model_metrics
    return dict(bw1=2.0 * (ld + 1) * U, bw=10.0 * max(m["bw"], 4 * U), L=10.0 * max(m["L"], ld * U),
                y=10.0 * max(m["y"], ld * U), Minv=10.0 * max(m["Minv"], 32 * U), res=10.0 * max(m["res"], ld * U),
                x=10.0 * max(m["x"], ld * U))


def check(e, g, forward):
    """Hold the gates: e_bw (both), e_Minv and e_res always, e_L / e_y / e_x on the forward-gated families."""
    assert all(np.isfinite(v) for v in e.values()), e
    assert e["bw"] <= g["bw1"], ("gate 1", e, g)
    assert e["bw"] <= g["bw"], ("gate 2", e, g)
    assert e["Minv"] <= g["Minv"] and e["res"] <= g["res"], (e, g)
    if forward:
        assert e["L"] <= g["L"] and e["y"] <= g["y"] and e["x"] <= g["x"], (e, g)


def line(tag, e, m=None):
    keys = ("bw", "L", "y", "Minv", "res", "x")
    s = f"K3REF {tag} kernel " + " ".join(f"e_{k}={e[k]:.2e}" for k in keys)
    if m is not None:
        s += " model " + " ".join(f"{k}={m[k]:.2e}" for k in keys)
    return s
