"""The tile reduction of K2 (k_schur_reduce: schur_reduce_elem / schur_reduce_vec) at every split count its load
batching distinguishes, against the dense fp64 reference of tests/k2_ref.py -- the reference, metrics and gates of
tests/test_gpu_k2_reference.py (fp64 1e-10; fp32 10 x max(the arithmetic model's own error, 1e-6) and e_S <= 1e-4).

The reduce requests a tile's split partials in batches of eight, two batches before the first add, with indices past
the tile clamped to its last split; the diagonal lanes' U terms come from one load per wave (lane u = split u) and are
taken in item order by lane reads; the b | g_pose | diag U threads read eight splits at a time.  So the problem below
(145 poses: five F1 blocks, the last of 16 frames; landmarks of 2-4 consecutive frames inside one block, so only
chunk-0 tiles, which carry all three paths; 1,860 landmarks) has tiles of 1, 4, 8, 12 and 20 splits -- the classes
1 | 2-7 | exactly 8 | 9-15 | >= 16 -- and every test asserts, from the groups the library reports
(BAHandle.schur_groups), that all five occur.  Frame 0 is fixed (n_fixed = 1) and unobserved blocks do not exist.

Builds: ptzba_build_reduced (raw region), the device-driven LM's build without priors (the fused prepare: lambda D_pose
on the pose diagonal from the reduce's own sum of diag U, b^T in row n_aug), and the same build under a unary pose
prior on every fourth free frame (priors switch the fused prepare off: the prepare launch damps from dU, and the
region is the raw system plus P, P e and diag P, which the reference adds in frame order)."""
import numpy as np
import pytest

import k2_cases as k2c
import k2_ref as kr
import prior_ref

pytestmark = pytest.mark.gpu

FP64, FP32 = 0, 1
LOSS, HCURV, F_SCALE = "huber", 0.1, 2.5
LAM = 1e-2
N_POSE = 145
# landmarks per F1 block (first frame, frames, landmarks): a chunk-0 landmark weighs 6 and a split 256, so the tiles
# get ceil(6 n / 256) = 1, 4, 8, 12, 20 splits (45 items: under the 64 the builder aims at for a small problem)
BLOCKS = ((1, 32, 40), (33, 32, 150), (65, 32, 330), (97, 32, 500), (129, 16, 840))
CLASSES = {"1": (1, 1), "2-7": (2, 7), "8": (8, 8), "9-15": (9, 15), ">=16": (16, 1 << 30)}
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _problem():
    def make():
        rng = np.random.default_rng(81)
        segs, lm = [], 0
        for f0, nf, count in BLOCKS:
            for j in range(count):
                k = int(rng.integers(2, 5))
                # the first landmarks walk the block so that every frame is seen, the rest fall anywhere inside it
                s = f0 + min(j % nf, nf - k) if j < nf else int(rng.integers(f0, f0 + nf - k + 1))
                segs += [(lm, f, int(rng.integers(1, 3))) for f in range(s, s + k)]
                lm += 1
        return k2c.build(N_POSE, segs, 82)
    return _memo("problem", make)


def _struct():
    import ptzba

    def make():
        p = _problem()
        win = ptzba.frame_coupling_window(N_POSE, p[4], p[5])
        pos, _, _, n_aug, _ = ptzba.plan_export(win, 1, ptzba.ORDER_NESTED)
        return dict(win=win, pos=pos, n_aug=n_aug, mask=kr.written_mask(win))
    return _memo("struct", make)


def _ref(hcurv=HCURV):
    """The reference at x0 (per curvature weight), computed once and never modified."""
    return _memo(("ref", hcurv), lambda: kr.reduced_system(_problem(), LAM, LOSS, hcurv, F_SCALE))


def _model(hcurv=HCURV):
    def make():
        m = kr.model_mf(_problem(), LAM, LOSS, hcurv, F_SCALE, win=_struct()["win"])
        return kr.metrics(m, _ref(hcurv), _struct()["mask"])
    return _memo(("model", hcurv), make)


def _factors():
    p = _problem()
    W = np.diag(1.0 / prior_ref.SIGMA ** 2)
    rng = np.random.default_rng(83)
    return [([f], p[2][f] + rng.uniform(-3, 3, 3) * prior_ref.SIGMA, W) for f in range(1, N_POSE, 4)]


def _open(precision, monkeypatch, priors=False):
    import ptzba
    monkeypatch.delenv("PTZBA_NO_FUSED_PREP", raising=False)
    u, v, ptz0, rays0, frame, landmark, xy, weight = _problem()
    h = ptzba.BAHandle(0)
    h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, weight=weight, precision=precision,
                  loss=ptzba.LOSS_HUBER, f_scale=F_SCALE, ordering=ptzba.ORDER_NESTED)
    g = h.schur_groups()
    ns = g[:, 3] - g[:, 2]
    assert len(g) == h.k2_tile_info()["tiles"] and ns.min() >= 1
    seen = {k: int(((ns >= lo) & (ns <= hi)).sum()) for k, (lo, hi) in CLASSES.items()}
    print(f"REDCHAIN splits per tile {ns.tolist()} chunks {g[:, 1].tolist()} classes {seen}")
    assert all(seen.values()), seen  # every class of split counts the reduce distinguishes really runs
    assert (g[:, 1] == 0).all()      # chunk-0 tiles: each also runs the diagonal and the vector paths
    if priors:
        h.set_pose_priors(_factors())
    h.set_state(ptz0, rays0)
    h.set_huber_curvature(HCURV)
    h.linearize()
    return h


def _region(h):
    import torch
    import bench
    h.sync()
    sp, n, _ = h.exchange()
    return torch.as_tensor(bench._DevArray(sp, n), device="cuda:0").cpu().numpy().copy()


def _view(h, region):
    s = _struct()
    si = h.solver_info()
    assert si["n_aug"] == s["n_aug"] and si["ld"] * (si["ld"] + 3) == len(region)
    return kr.region_view(region, s["pos"], si["ld"], si["n_aug"], s["win"])


def _check(what, precision, view, rs, want_S, want_aug, hcurv=HCURV):
    ref = dict(rs, S=want_S)
    e = kr.metrics(view, ref, view["mask"])
    gates = dict.fromkeys(e, kr.FP64_GATE) if precision == FP64 else kr.fp32_gates(_model(hcurv))
    print(f"REDCHAIN {what} precision={precision} " + " ".join(f"e_{k}={e[k]:.3e}" for k in ("S", "b", "g", "dU")) +
          " gates " + " ".join(f"{k}={gates[k]:.3e}" for k in ("S", "b", "g", "dU")))
    assert np.isfinite(view["S"]).all()
    assert np.all(view["S"][~view["mask"]] == 0.0)
    aug_scale = np.abs(rs["b"]).max()
    assert np.abs(view["aug"] - want_aug).max() <= (1e-10 if precision == FP64 else gates["b"]) * aug_scale
    for k in e:
        assert e[k] <= gates[k], (k, e, gates)
    if precision == FP32:
        assert e["S"] <= 1e-4, e


@pytest.mark.parametrize("precision", [FP64, FP32])
def test_raw_build_matches_fp64_and_repeats_bitwise(gpu_available, precision, monkeypatch):
    """ptzba_build_reduced twice on one linearisation: the region against the reference, and S | b | g_pose | diag U of
    the second build bit for bit those of the first (every sum of the reduce runs in one fixed order)."""
    h = _open(precision, monkeypatch)
    h.build_reduced(LAM)
    r1 = _region(h)
    h.build_reduced(LAM)
    r2 = _region(h)
    view = _view(h, r1)
    h.close()
    rs = _ref()
    _check("raw", precision, view, rs, rs["S"], np.zeros_like(rs["b"]))
    assert view["rest"] == 0.0
    assert np.array_equal(r1, r2)  # the whole region: S, b, g_pose and diag U


@pytest.mark.parametrize("precision", [FP64, FP32])
def test_fused_prepare_build_matches_fp64(gpu_available, precision, monkeypatch):
    """The device-driven LM's first build on a fresh handle (no priors: the fused prepare runs in the reduce): lambda
    D_pose on the pose diagonal, D_pose = max(0, diag U) from the diagonal lanes' own sums, and b^T in row n_aug.  (The
    device-driven LM linearises its first point itself, with the curvature weight 1 until its switch: the reference of
    this case is the one at weight 1.)"""
    import ptzba
    h = _open(precision, monkeypatch)
    h.lm_start()
    h.lm_init(ptzba.ptzba_lm_opts(1e-14, 1e-16, 0.0, LAM, 1e-12, 1e16, 1, 30, 0, HCURV, 0.0))
    h.lm_build()
    view = _view(h, _region(h))
    h.close()
    rs = _ref(1.0)
    want = kr.expected_view(rs, LAM, True)
    _check("fused", precision, view, rs, want["S"], want["aug"], hcurv=1.0)
    d = np.arange(len(rs["b"]))
    assert np.all(view["S"][d, d] - rs["S"][d, d] > 0.5 * LAM * rs["dU"])  # the damping is there, and it is not small


@pytest.mark.parametrize("precision", [FP64, FP32])
def test_build_with_pose_prior_matches_fp64(gpu_available, precision, monkeypatch):
    """A unary prior on every fourth free frame: the build adds P to S, P e to g_pose (and takes it from b) and diag P
    to diag U after the reduce (priors switch the fused prepare off, so the region is otherwise raw)."""
    p = _problem()
    P, Pe, _ = prior_ref.prior_terms(_factors(), p[2], N_POSE)
    rs0 = _ref()
    dU = rs0["dU"] + np.diag(P)
    rs = dict(rs0, S=rs0["S"] + P, b=rs0["b"] - Pe, g_pose=rs0["g_pose"] + Pe, dU=dU)  # (scale stays the records')
    assert np.abs(np.diag(P)).max() > 10 * kr.FP64_GATE * rs0["dU"].max()  # a dropped prior could not pass
    h = _open(precision, monkeypatch, priors=True)
    h.build_reduced(LAM)
    view = _view(h, _region(h))
    h.close()
    _check("prior", precision, view, rs, rs["S"], np.zeros_like(rs["b"]))
