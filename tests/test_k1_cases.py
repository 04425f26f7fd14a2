"""CPU tests that pin tests/k1_cases.py (the crafted K1 problems and the dense fp64 step reference the GPU tests of
tests/test_gpu_k1_paths.py compare against): the reference's gradient against finite differences of the oracle's cost,
its normal-equation blocks against the oracle's own block accumulation, and the conditions the generator promises."""
import numpy as np
import pytest

import k1_cases as kc
from oracle import ptz_oracle as orc


@pytest.fixture(scope="module")
def problems():
    return {(extra, weighted): kc.craft(extra=extra, weighted=weighted) for extra in range(4) for weighted in (False, True)}


@pytest.mark.parametrize("loss,f_scale", [("linear", 1.0), ("huber", 1.0), ("huber", 2.5)])
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_gradient_matches_fd_of_oracle_cost(problems, loss, f_scale, weighted):
    """g of the reference == central finite differences of orc.ba_cost (integer weights as repeated records) on 40
    random coordinates; steps and tolerance of test_analytic_jacobian_matches_fd_cpu."""
    p = problems[(0, weighted)]
    u, v, ptz0, rays0, frame, landmark, xy, _ = kc.expand(p)
    n_pose = len(ptz0)
    fr, lm = frame.astype(np.int64), landmark.astype(np.int64)
    g = kc.reference(p, 0.0, loss, 0.1, f_scale)["g"]
    x0 = np.concatenate([ptz0[1:].reshape(-1), rays0.reshape(-1)])
    cost = lambda x: orc.ba_cost(np.concatenate([ptz0[0], x]), n_pose, u, v, fr, lm, xy, loss, f_scale)
    rng = np.random.default_rng(0)
    gmax = np.abs(g).max()
    for c in rng.choice(len(x0), 40, replace=False):
        e = np.zeros_like(x0)
        e[c] = 1e-5 if c < 3 * (n_pose - 1) and c % 3 != 2 else (1e-3 if c < 3 * (n_pose - 1) else 1e-5)
        fd = (cost(x0 + e) - cost(x0 - e)) / (2 * e[c])
        np.testing.assert_allclose(g[c], fd, rtol=1e-5, atol=1e-5 * max(1.0, abs(fd)), err_msg=f"coordinate {c} of |g|max {gmax}")


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_blocks_match_oracle_normal_blocks(problems, weighted):
    """At hcurv = 0.3 (the oracle's fixed curvature floor), f_scale = 1: the reference's H blocks and g == the oracle's
    _normal_blocks (U, V, W, g_pose, g_ray), to 1e-12 of each block kind's largest entry -- the helper is tied to the
    oracle test_oracle_golden.py pins."""
    p = problems[(1, weighted)]
    u, v, ptz0, rays0, frame, landmark, xy, _ = kc.expand(p)
    n, m = len(ptz0), len(rays0)
    fr, lm = frame.astype(np.int64), landmark.astype(np.int64)
    key, seg = np.unique(lm * n + fr, return_inverse=True)
    U, V, W, gp, gr, cost = orc._normal_blocks(ptz0, rays0, u, v, fr, lm, xy, seg.astype(np.int64), len(key), "huber", 1.0)
    R = kc.reference(p, 0.0, "huber", 0.3, 1.0)
    H, g, nf = R["H"], R["g"], n - 1
    assert abs(R["cost"] - cost) <= 1e-12 * cost

    def close(a, b, what):
        err = np.abs(a - b).max() / np.abs(b).max()
        assert err <= 1e-12, (what, err)

    Hp = H[:3 * nf, :3 * nf].reshape(nf, 3, nf, 3)
    close(np.stack([Hp[i, :, i, :] for i in range(nf)]), U[1:], "U")
    off = Hp.copy()
    for i in range(nf):
        off[i, :, i, :] = 0
    assert np.abs(off).max() == 0  # no pose-pose coupling between frames
    Hr = H[3 * nf:, 3 * nf:].reshape(m, 2, m, 2)
    close(np.stack([Hr[l, :, l, :] for l in range(m)]), V, "V")
    Hw = H[:3 * nf, 3 * nf:].reshape(nf, 3, m, 2)
    seg_lm, seg_fr = key // n, key % n
    free = seg_fr > 0
    close(Hw[seg_fr[free] - 1, :, seg_lm[free], :], W[free], "W")
    mask = np.zeros((nf, m), bool)
    mask[seg_fr[free] - 1, seg_lm[free]] = True
    assert np.abs(Hw.transpose(0, 2, 1, 3)[~mask]).max() == 0  # W only where a segment exists
    close(g[:3 * nf].reshape(nf, 3), gp[1:], "g_pose")
    close(g[3 * nf:].reshape(m, 2), gr, "g_ray")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_generator_conditions(problems, extra, weighted):
    """What the GPU tests rely on, so a later edit of the generator cannot drift into an ill-posed or uninformative
    case: the record layout reaches the K1 paths (four windows, every record-group alignment at an inner window
    boundary, a run over more than two 256-record batches, one-record and one-segment landmarks), no residual near the
    Huber unit at x0, both Huber branches populated per image axis, every free frame seen by >= 3 landmarks, and a
    well-conditioned (Jacobi-scaled) H."""
    p = problems[(extra, weighted)]
    n_pose, n_lm = len(p[2]), len(p[3])
    L = kc.layout(p)
    assert L["max_windows"] >= 4
    assert L["boundary_alignments"] == {0, 1, 2, 3}
    assert L["max_run"] > 2 * 256
    assert min(L["frames_seen"][1:]) >= 3
    nrec = np.bincount(p[5], minlength=n_lm)
    key = np.unique(p[5].astype(np.int64) * n_pose + p[4])
    nseg = np.bincount(key // n_pose, minlength=n_lm)
    assert (nrec == 1).any() and ((nseg == 1) & (nrec > 1)).any()
    assert n_lm == 142 + extra and nrec.min() >= 1
    assert (p[7] is not None) == weighted
    if weighted:
        assert set(np.unique(p[7])) == {1.0, 2.0, 3.0, 5.0}
    assert np.array_equal(p[2][0], kc.craft(extra=extra, weighted=weighted)[2][0])  # deterministic
    for f_scale in kc.F_SCALES:
        for hcurv in (1.0, 0.1):
            R = kc.reference(p, 0.0, "huber", hcurv, f_scale)
            z = R["z"].reshape(-1, 2)
            assert np.abs(z - 1.0).min() >= 1e-3
            share = (z > 1.0).mean(0)
            assert np.all(share >= 0.05) and np.all(share <= 0.60), share
            d = 1.0 / np.sqrt(np.diag(R["H"]))
            cond = np.linalg.cond(R["H"] * d[:, None] * d[None, :])
            assert cond <= 1e5, cond


def test_reference_damping_memory_and_prediction(problems):
    """D never shrinks below D_prev, the step solves the damped system, and the predicted reduction is the model's:
    cost(x) - model(x + dx) = -g.dx - 1/2 dx^T H dx == -1/2 g.dx + 1/2 lam dx^T D dx at the damped solution."""
    p = problems[(0, False)]
    R1 = kc.reference(p, 1e-2, "huber", 0.1, 2.5)
    R2 = kc.reference(p, 1e-1, "huber", 0.1, 2.5, D_prev=10.0 * R1["D"])
    assert np.array_equal(R2["D"], 10.0 * R1["D"])
    for R, lam in ((R1, 1e-2), (R2, 1e-1)):
        A = R["H"] + lam * np.diag(R["D"])
        assert np.abs(A @ R["dx"] + R["g"]).max() <= 1e-9 * R["gmax"]
        model = -float(R["g"] @ R["dx"]) - 0.5 * float(R["dx"] @ R["H"] @ R["dx"])
        assert abs(model - R["pred"]) <= 1e-9 * abs(R["pred"])
        assert R["pred"] > 0
    assert R2["dx2"] < R1["dx2"]
