"""k_trial (ray back-substitution, trial poses and the step's partial scalars) on landmarks of every length its segment
walk distinguishes, against the oracle's fp64 normal-equation solve: one undamped Gauss-Newton step as in
tests/test_gpu_nested2.py (sparse solve of J^T J dx = -J^T r on the oracle's Jacobian and residual; 1e-7 in fp64) with
the fp32 gates of tests/test_gpu_k1_paths.py (step and predicted reduction 2e-3, |delta|^2 4e-3, max |gradient| 10 x the
change that rounding J and r to float32 makes in the reference, floor 1e-6).

A wave walks its landmark's segments two strides of 64 at a time with clamped, masked lanes, so the problem (140 poses)
holds landmarks of 0, 1, 63, 64, 65, 128 and 140 segments -- no walk, one lane, one lane short of a stride, exactly a
stride, one lane into the second, exactly one trip, a second trip -- two of each, one of every pair seeing the fixed
frame 0 (its segment has no system row and is dropped), besides ~700 landmarks of 3-12 consecutive frames that make the
step well determined.  The test asserts those counts on the unique (landmark, frame) pairs, which is what
ptzba_set_problem's lm_seg_begin holds (problem_info reports their number and the longest landmark).

Checked: the trial poses and rays (the step, per kind), and the partial scalars where the library keeps them apart --
loc[0..3], the pose block's predicted reduction, |dx|^2, |x|^2 and max |g|, and scal[2..5], the fixed-order column sums
(maximum for the last) of the per-landmark partials lm_red -- each against the oracle's own quantity of the same part.
A part of the predicted reduction is a signed sum, so it is held to the gate times the sum of its terms' magnitudes;
the totals (read_scalars) are held to the gates as they stand.  |x|^2 involves no step: 1e-12."""
import numpy as np
import pytest

import k2_cases as k2c

pytestmark = pytest.mark.gpu

N_POSE = 140
LONG = {0: [], 1: [(7, 1), (0, 1)], 63: [(10, 63), (0, 63)], 64: [(70, 64), (0, 64)], 65: [(40, 65), (0, 65)],
        128: [(5, 128), (0, 128)], 140: [(0, 140), (0, 140)]}  # segments: [(first frame, frames)]
_cache = {}


def _problem():
    if "p" not in _cache:
        rng = np.random.default_rng(91)
        segs, lm, want = [], 0, {}
        for n, runs in LONG.items():
            for f0, k in runs or [(0, 0), (0, 0)]:
                segs += [(lm, f, int(rng.integers(1, 3))) for f in range(f0, f0 + k)]
                want[lm] = n
                lm += 1
        for j in range(700):
            k = int(rng.integers(3, 13))
            s = min(j % N_POSE, N_POSE - k) if j < 2 * N_POSE else int(rng.integers(0, N_POSE - k + 1))
            segs += [(lm, f, int(rng.integers(1, 3))) for f in range(s, s + k)]
            lm += 1
        _cache["p"] = (k2c.build(N_POSE, segs, 92), want)
    return _cache["p"]


def _segments(p):
    """Segments per landmark: the unique (landmark, frame) pairs of the records, and which landmarks see frame 0."""
    frame, landmark = p[4].astype(np.int64), p[5].astype(np.int64)
    pairs = np.unique(landmark * N_POSE + frame)
    cnt = np.bincount(pairs // N_POSE, minlength=len(p[3]))
    fixed = np.zeros(len(p[3]), bool)
    fixed[pairs[pairs % N_POSE == 0] // N_POSE] = True
    return cnt, fixed, len(pairs)


def _oracle(round32=False):
    """The reference step and its parts, computed once and never modified."""
    key = ("ref", round32)
    if key not in _cache:
        import scipy.sparse.linalg as spla
        from oracle import ptz_oracle as orc
        p, _ = _problem()
        u, v, ptz0, rays0, frame, landmark, xy, _w = p
        n_lm = len(rays0)
        x0 = np.concatenate([ptz0[1:].reshape(-1), rays0.reshape(-1)])
        fr, lm = frame.astype(np.int64), landmark.astype(np.int64)
        J = orc.ba_jacobian(x0, N_POSE, n_lm, u, v, ptz0[0], fr, lm).tocsc()
        r = orc.compute_residual_records(np.concatenate([ptz0[0], x0]), N_POSE, u, v, fr, lm, xy)
        if round32:
            J = J.astype(np.float32).astype(np.float64)
            r = r.astype(np.float32).astype(np.float64)
        g = J.T @ r
        n3 = 3 * (N_POSE - 1)
        if round32:
            _cache[key] = dict(gmax_pose=np.abs(g[:n3]).max(), gmax_ray=np.abs(g[n3:]).max())
            return _cache[key]
        cnt, _, _ = _segments(p)
        live = np.concatenate([np.ones(n3, bool), np.repeat(cnt > 0, 2)])  # a landmark nobody sees has no equations
        H = (J.T @ J).tocsc()[live][:, live]
        dx = np.zeros(len(x0))
        dx[live] = spla.spsolve(H, -g[live])
        tp, tr = -0.5 * g[:n3] * dx[:n3], -0.5 * g[n3:] * dx[n3:]  # undamped: the predicted reduction is -1/2 g.dx
        seen = np.repeat(cnt > 0, 2)
        _cache[key] = dict(
            dx=dx, n3=n3, pred_pose=tp.sum(), pred_pose_abs=np.abs(tp).sum(), pred_ray=tr.sum(),
            pred_ray_abs=np.abs(tr).sum(), dx2_pose=(dx[:n3] ** 2).sum(), dx2_ray=(dx[n3:] ** 2).sum(),
            x2_pose=(ptz0 ** 2).sum(), x2_ray=(rays0.reshape(-1)[seen] ** 2).sum(), gmax_pose=np.abs(g[:n3]).max(),
            gmax_ray=np.abs(g[n3:]).max())
        _cache[key]["dx"].setflags(write=False)
    return _cache[key]


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("precision", [0, 1])
def test_undamped_step_and_partial_scalars_match_oracle(gpu_available, precision):
    import torch
    import bench
    import ptzba
    p, want = _problem()
    u, v, ptz0, rays0, frame, landmark, xy, _w = p
    cnt, fixed, n_seg = _segments(p)
    for n in LONG:
        ls = [l for l, k in want.items() if k == n]
        assert len(ls) == 2 and all(cnt[l] == n for l in ls), (n, ls, cnt[ls])
        assert n == 0 or fixed[ls].any(), n  # one landmark of every length sees the fixed frame
    assert any(cnt[l] >= 129 for l in want)
    h = ptzba.BAHandle(0)
    h.set_problem(N_POSE, len(rays0), frame, landmark, xy, u, v, precision=precision)
    info = h.info()
    assert info["n_segments"] == n_seg and info["max_seg_per_landmark"] == int(cnt.max()), (info, n_seg, cnt.max())
    assert info["n_active_landmarks"] == int((cnt > 0).sum())
    h.set_state(ptz0, rays0)
    h.linearize()
    h.build_reduced(0.0)
    h.solve_reduced()
    s = h.read_scalars()
    assert s[5] == 0
    _, _, sc = h.exchange()
    parts = torch.as_tensor(bench._DevArray(sc, 16), device="cuda:0").cpu().numpy().copy()  # scal[0..8) | loc[0..8)
    h.accept(True)
    ptz1, rays1 = h.get_state()
    h.close()
    ref = _oracle()
    n3 = ref["n3"]
    tol, d2_tol = (1e-7, 1e-7) if precision == 0 else (2e-3, 4e-3)
    assert np.array_equal(ptz1[0], ptz0[0])  # the fixed frame does not move
    dx_gpu = np.concatenate([(ptz1 - ptz0)[1:].reshape(-1), (rays1 - rays0).reshape(-1)])
    e_pose = np.abs(dx_gpu[:n3] - ref["dx"][:n3]).max() / np.abs(ref["dx"][:n3]).max()
    e_ray = np.abs(dx_gpu[n3:] - ref["dx"][n3:]).max() / np.abs(ref["dx"][n3:]).max()
    named = np.array(sorted(want))
    e_named = np.abs((rays1 - rays0)[named].reshape(-1) - ref["dx"][n3:].reshape(-1, 2)[named].reshape(-1)).max() / \
        np.abs(ref["dx"][n3:]).max()
    assert np.array_equal(rays1[cnt == 0], rays0[cnt == 0])  # a landmark nobody sees stays where it is
    loc, red = parts[8:12], parts[2:6]
    e = dict(pose=e_pose, ray=e_ray, named=e_named,
             pred_pose=abs(loc[0] - ref["pred_pose"]) / ref["pred_pose_abs"],
             pred_ray=abs(red[0] - ref["pred_ray"]) / ref["pred_ray_abs"],
             pred=_rel(s[2], ref["pred_pose"] + ref["pred_ray"]),
             dx2_pose=_rel(loc[1], ref["dx2_pose"]), dx2_ray=_rel(red[1], ref["dx2_ray"]),
             dx2=_rel(s[3], ref["dx2_pose"] + ref["dx2_ray"]),
             x2_pose=_rel(loc[2], ref["x2_pose"]), x2_ray=_rel(red[2], ref["x2_ray"]),
             gmax_pose=_rel(loc[3], ref["gmax_pose"]), gmax_ray=_rel(red[3], ref["gmax_ray"]),
             gmax=_rel(s[6], max(ref["gmax_pose"], ref["gmax_ray"])))
    if precision == 0:
        g_gate = dict(pose=1e-7, ray=1e-7)
    else:
        r32 = _oracle(round32=True)
        g_gate = {k: max(10.0 * _rel(r32["gmax_" + k], ref["gmax_" + k]), 1e-6) for k in ("pose", "ray")}
    print(f"TRIALCHAIN precision={precision} segments max {cnt.max()} " +
          " ".join(f"{k}={x:.3e}" for k, x in e.items()) + f" gmax gates {g_gate}")
    assert max(e["pose"], e["ray"], e["named"]) <= tol, e
    assert max(e["pred_pose"], e["pred_ray"], e["pred"]) <= tol, e
    assert max(e["dx2_pose"], e["dx2_ray"], e["dx2"]) <= d2_tol, e
    assert max(e["x2_pose"], e["x2_ray"]) <= 1e-12, e
    assert e["gmax_pose"] <= g_gate["pose"] and e["gmax_ray"] <= g_gate["ray"], (e, g_gate)
    assert e["gmax"] <= max(g_gate.values()), (e, g_gate)
