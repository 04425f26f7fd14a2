"""Dense numpy reference of the keyframe marginalisation (shared by test_marginal_cpu.py and test_gpu_marginal.py;
DESIGN.md 4.9, include/ptzba.h ptzba_marginal_prior).

Given a problem p in the pair form, a state (ptz, rays), the leaving frames E and a record mask D:

    J_D, r_D     the oracle's Jacobian and residuals restricted to D, rows scaled by sqrt(rho') (curvature 1)
    clones       every landmark of D is eliminated with D's records only:
                     S_D = U_D - sum_l W_l V_l^-1 W_l^T,      b_D = g_p - sum_l W_l V_l^-1 g_l
    absorbed     every factor naming a free frame of E -- pose priors (frames, mean, info) and an information-form
                 marginal -- is added whole:  A = S_D + sum Lambda_k,  a = b_D + sum (Lambda_k e_k [+ eta_k])
    K            the free frames outside E with a dropped record or named by an absorbed factor, ascending
    result       Lambda = A_KK - A_KE A_EE^-1 A_EK (np.linalg.solve), eta = a_K - A_KE A_EE^-1 a_E, lin = x_K,
                 offset = 1/2 sum_D rho + the absorbed factors' cost at x

Frame 0 is the gauge (n_fixed = 1), as in the oracle's Jacobian.  gn_step / solve add an information-form term to
prior_ref's objective."""
import dataclasses

import numpy as np

import prior_ref


def drop_mask_loop(frame, E):
    """ptzba.drop_mask, written as a loop over the matches."""
    E = set(int(f) for f in np.atleast_1d(E))
    out = np.zeros(len(frame), np.uint8)
    for m in range(len(frame) // 2):
        if int(frame[2 * m]) in E or int(frame[2 * m + 1]) in E:
            out[2 * m] = out[2 * m + 1] = 1
    return out


def _rows3(frames):
    """Rows of the frames (>= 1) among the free-pose parameters."""
    frames = np.asarray(frames, np.int64).reshape(-1)
    return (3 * (frames[:, None] - 1) + np.arange(3)[None, :]).reshape(-1)


def dropped_system(p, ptz, rays, mask, loss="linear", f_scale=1.0):
    """(S_D, b_D over the 3 (n_pose - 1) free-pose parameters, 1/2 sum_D rho, frames with a dropped record)."""
    import scipy.sparse as sp
    J, r, c, w1, _ = prior_ref._records(p, ptz, rays, loss, f_scale)
    rec = np.asarray(mask).reshape(-1) != 0
    rows = np.repeat(rec, 2)
    k = 3 * (p.n_pose - 1)
    sw = np.sqrt(w1[rows])
    Jd = (sp.diags(sw) @ J[rows]).tocsc()
    rd = sw * r[rows]
    Jp, Jl = Jd[:, :k], Jd[:, k:]
    U = np.asarray((Jp.T @ Jp).todense())
    W = (Jp.T @ Jl).tocsc()
    V = (Jl.T @ Jl).tocsr()
    g = np.asarray(Jd.T @ rd).reshape(-1)
    S, b = U.copy(), g[:k].copy()
    for l in np.unique(p.landmark[rec]).astype(np.int64):
        Vl = np.asarray(V[2 * l:2 * l + 2, 2 * l:2 * l + 2].todense())
        Wl = np.asarray(W[:, 2 * l:2 * l + 2].todense())
        Y = Wl @ np.linalg.inv(Vl)
        S -= Y @ Wl.T
        b -= Y @ g[k + 2 * l:k + 2 * l + 2]
    return S, b, float(np.sum(c[rows])), np.unique(p.frame[rec]).astype(np.int64)


def marginal(p, ptz, rays, E, mask=None, loss="linear", f_scale=1.0, factors=(), marg=None):
    """The reference marginal as a ptzba.Marginal, and the list of absorbed factor indices (the marginal: "m")."""
    import ptzba
    ptz = np.asarray(ptz, np.float64)
    E = [int(f) for f in np.atleast_1d(E)]
    if mask is None:
        mask = ptzba.drop_mask(p.frame, E)
    k = 3 * (p.n_pose - 1)
    S, b, off, touched = dropped_system(p, ptz, rays, mask, loss, f_scale)
    A, a = S.copy(), b.copy()
    x = ptz.reshape(-1)
    Ef = [f for f in E if f >= 1]
    named = set(int(f) for f in touched)
    absorbed = []
    for i, (frames, mean, info) in enumerate(factors):
        frames = np.atleast_1d(np.asarray(frames, np.int64))
        if not set(frames.tolist()) & set(Ef):
            continue
        absorbed.append(i)
        named |= set(frames.tolist())
        idx = _rows3(frames)
        e = x[idx + 3] - np.asarray(mean, np.float64).reshape(-1)
        L = np.asarray(info, np.float64)
        A[np.ix_(idx, idx)] += L
        a[idx] += L @ e
        off += 0.5 * float(e @ L @ e)
    if marg is not None and set(marg.frames.tolist()) & set(Ef):
        absorbed.append("m")
        named |= set(marg.frames.tolist())
        idx = _rows3(marg.frames)
        d = x[idx + 3] - marg.lin.reshape(-1)
        A[np.ix_(idx, idx)] += marg.info
        a[idx] += marg.info @ d + marg.grad
        off += marg.value(ptz)
    K = np.array(sorted(f for f in named if f >= 1 and f not in E), np.int64)
    iK = _rows3(K)
    Lam, eta = A[np.ix_(iK, iK)], a[iK]
    cond = None
    if Ef:
        iE = _rows3(Ef)
        AEE, AKE = A[np.ix_(iE, iE)], A[np.ix_(iK, iE)]
        cond = float(np.linalg.cond(AEE))
        X = np.linalg.solve(AEE, AKE.T).T
        Lam = Lam - X @ AKE.T
        eta = eta - X @ a[iE]
    m = ptzba.Marginal(K, ptz[K], 0.5 * (Lam + Lam.T), eta, off)
    m.cond_EE = cond
    return m, absorbed


def clone_problem(p, rays, mask):
    """Q1: p with the records of D relabelled to fresh landmark ids (one clone per landmark of D), and its rays."""
    rec = np.asarray(mask).reshape(-1) != 0
    ids, inv = np.unique(p.landmark[rec], return_inverse=True)
    lm = p.landmark.copy()
    lm[rec] = p.n_landmark + inv
    q1 = dataclasses.replace(p, landmark=lm.astype(np.int32), n_landmark=p.n_landmark + len(ids))
    return q1, np.concatenate([np.asarray(rays, np.float64), np.asarray(rays, np.float64)[ids]])


def kept_problem(p, mask):
    """Q2: p without the records of D (frames and landmarks keep their ids)."""
    keep = np.asarray(mask).reshape(-1) == 0
    return dataclasses.replace(p, frame=p.frame[keep], landmark=p.landmark[keep], xy=p.xy[keep])


def _marg_terms(marg, ptz, n_pose):
    k = 3 * (n_pose - 1)
    P, g = np.zeros((k, k)), np.zeros(k)
    if marg is None or not len(marg.frames):
        return P, g, 0.0
    assert marg.frames.min() >= 1
    idx = _rows3(marg.frames)
    d = np.asarray(ptz, np.float64).reshape(-1)[idx + 3] - marg.lin.reshape(-1)
    P[np.ix_(idx, idx)] = marg.info
    g[idx] = marg.info @ d + marg.grad
    return P, g, marg.value(ptz)


def cost(p, ptz, rays, factors=(), marg=None, loss="linear", f_scale=1.0):
    return prior_ref.cost(p, ptz, rays, list(factors), loss, f_scale) + _marg_terms(marg, ptz, p.n_pose)[2]


def gn_step(p, ptz, rays, factors=(), marg=None, loss="linear", f_scale=1.0, curvature=False):
    """dx of (H + P + Lambda) dx = -(g + P e + Lambda d + eta) over [free poses | rays]; parameters without any term
    (a landmark or frame with no record and no factor) get a unit diagonal, so their step is zero."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    J, r, _, w1, w2 = prior_ref._records(p, ptz, rays, loss, f_scale)
    P, gp, _ = prior_ref.prior_terms(list(factors), ptz, p.n_pose)
    M, gm, _ = _marg_terms(marg, ptz, p.n_pose)
    k = 3 * (p.n_pose - 1)
    Jw = sp.diags(np.sqrt(w2 if curvature else w1)) @ J
    H = (Jw.T @ Jw).tolil()
    H[:k, :k] = H[:k, :k] + sp.lil_matrix(P + M)
    g = np.asarray(J.T @ (w1 * r)).reshape(-1)
    g[:k] += gp + gm
    for i in np.flatnonzero(np.asarray(H.diagonal()) == 0):
        H[i, i] = 1.0
    return spla.spsolve(H.tocsc(), -g), g


def solve(p, ptz0, rays0, factors=(), marg=None, loss="linear", f_scale=1.0, max_iter=100):
    """prior_ref.solve with the information-form term: Gauss-Newton with step halving to the stationary point."""
    ptz = np.array(ptz0, np.float64)
    rays = np.array(rays0, np.float64)
    c = cost(p, ptz, rays, factors, marg, loss, f_scale)
    for _ in range(max_iter):
        dx, _ = gn_step(p, ptz, rays, factors, marg, loss, f_scale, curvature=loss == "huber")
        dptz, drays = prior_ref.split(p, dx)
        t = 1.0
        while True:
            c1 = cost(p, ptz + t * dptz, rays + t * drays, factors, marg, loss, f_scale)
            if c1 <= c + 1e-12 * abs(c) or t < 1e-6:
                break
            t *= 0.5
        ptz, rays, c = ptz + t * dptz, rays + t * drays, min(c, c1)
        if t == 1.0 and np.abs(dptz / np.array([1.0, 1.0, 1e3])).max() < 1e-10 and np.abs(drays).max() < 1e-10:
            break
    return ptz, rays, c


# the cases of the tests: (config, leaving frames)
CASES = (("config1", (0,)), ("config1", (3,)), ("config1", (0, 1)), ("config2", (0,)), ("config2", (24, 25)))


def step_identity(p, E, marg=None, mask=None):
    """One undamped Gauss-Newton step of the clone problem Q1 against the step of Q2 (p without D) plus the marginal,
    at p's initial state, on the kept poses and the rays that still have records.  A free frame of E is left without
    terms in Q2 (zero step).  Returns (identity error, distance of Q2's step without the marginal, max |dx|, dx of
    Q1 restricted to [kept poses | rays of Q2's landmarks], those index arrays)."""
    import ptzba
    if mask is None:
        mask = ptzba.drop_mask(p.frame, E)
    if marg is None:
        marg = marginal(p, p.init_ptz, p.init_rays, E, mask)[0]
    q1, rays1 = clone_problem(p, p.init_rays, mask)
    q2 = kept_problem(p, mask)
    d1 = gn_step(q1, p.init_ptz, rays1)[0]
    d2 = gn_step(q2, p.init_ptz, p.init_rays, marg=marg)[0]
    d3 = gn_step(q2, p.init_ptz, p.init_rays)[0]
    k = 3 * (p.n_pose - 1)
    keepf = np.array([f for f in range(1, p.n_pose) if f not in E], np.int64)
    ik = _rows3(keepf)
    seen = np.unique(q2.landmark).astype(np.int64)
    il = (k + 2 * seen[:, None] + np.arange(2)[None, :]).reshape(-1)
    sel = np.concatenate([ik, il])
    ref = d1[:len(d2)][sel]
    scale = np.abs(ref).max()
    return (np.abs(d2[sel] - ref).max() / scale, np.abs(d3[sel] - ref).max() / scale, scale, ref, keepf, seen)
