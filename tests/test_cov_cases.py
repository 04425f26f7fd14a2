"""CPU checks of tests/cov_cases.py: conditions on the inputs of tests/test_gpu_cov_reference.py, asserted on the reference
alone -- every crafted system is positive definite, the dense and the Schur route of the reference agree, each
configuration has the shape it is used for, the strided selection makes a workgroup of k_cov_gram climb and drop between
two blocks under the packing model, and the reference pivot is known to far more digits than its gate asks."""
import numpy as np
import pytest

import cov_cases as cc
import cov_ref
import k3_cases as kc

STRUCTS = ("one_tile", "chain", "nd2_small", "nd2", "wide")


@pytest.mark.parametrize("struct", STRUCTS)
def test_reference_is_positive_definite_and_its_routes_agree(struct):
    """H is positive definite (numpy's Cholesky succeeds, as does the Huber-weighted H of nd2), and np.linalg.inv(H)
    and the Schur route give the same blocks to 1e-9 in block_err: 100 times inside the 1e-7 they are used to check."""
    p = cc.problem(struct)
    H = cc.normal_matrix(struct)
    assert H.shape == (3 * (p.n_pose - 1) + 2 * p.n_landmark,) * 2
    np.linalg.cholesky(H)
    d = 1.0 / np.sqrt(np.diag(H))
    ev = np.linalg.eigvalsh(H * np.outer(d, d))
    pose, ray = cc.reference_blocks(struct)
    ps, rs = cov_ref.schur_blocks(p, p.init_ptz, p.init_rays)
    ep, er = cov_ref.block_err(ps, pose), cov_ref.block_err(rs, ray)
    print(f"COVCASE {struct}: {p.n_pose} frames {p.n_landmark} landmarks {len(p.frame)} records; scaled cond "
          f"{ev[-1] / ev[0]:.2e} min scaled eigenvalue {ev[0]:.2e}; dense vs schur pose {ep:.2e} ray {er:.2e}; "
          f"e_round {cc.e_round(struct):.2e}; the fp32 K2 model's pose blocks {cc.k2_model_error(struct):.2e}")
    assert ev[0] > 0
    assert ep <= 1e-9 and er <= 1e-9, (ep, er)
    assert not pose[0].any() and np.all(np.linalg.eigvalsh(pose[1:]) > 0) and np.all(np.linalg.eigvalsh(ray) > 0)
    assert not pose.flags.writeable and not ray.flags.writeable and not cc.inverse(struct).flags.writeable
    if struct == "nd2":
        np.linalg.cholesky(cc.normal_matrix(struct, "huber", 1.0))
        ph, rh = cc.reference_blocks(struct, "huber", 1.0)
        assert cov_ref.block_err(ph, pose) > 1e-3  # (the weights matter: the Huber comparison can fail)


@pytest.mark.parametrize("config", cc.CONFIGS)
def test_configurations_have_the_shapes_they_are_named_for(config, monkeypatch):
    pl = kc.plan(config, monkeypatch)
    kc.check_shape(config, pl)
    got, want = cc.shape_facts(pl), cc.FACTS[config]
    print(f"COVCASE {config}: {got}")
    assert got == want, (got, want)
    T = got["T"]
    if config == "one_tile":
        assert got["n_aug"] % 32 == 1 and got["last_live"] == 1  # the last visited tile holds one live row
    if config in ("nd2_small", "nd2", "nd2_nd1", "wide"):
        assert got["n_aug"] % 32 == 0 and pl["ld"] == got["n_aug"] + 32  # the augmented row opens a tile never visited
        assert got["padding"] > 0
        assert got["pattern"][0] < got["pattern"][1]  # sparser than the full lower triangle
    if config != "nd2_small":
        assert got["straddle"] >= 1
    assert T >= 2
    if config != "one_tile":
        assert cc.blocks(config, pl).max() >= 1  # some block starts after the first tile
    # the model's two first-tile rules are ordered as the kernel's comment says
    assert np.all(cc.landmark_t0(config, pl, True) <= cc.landmark_t0(config, pl, False))


@pytest.mark.parametrize("config,per_cu", [("nd2", 1), ("wide", 2)])
@pytest.mark.parametrize("groups_bound", [256, 512])
def test_strided_selection(config, per_cu, groups_bound, monkeypatch):
    """blocks > groups_bound, and under the packing model one workgroup takes a block whose first tile is at least 2
    higher than its previous block's and one takes a block at least 2 lower -- whichever frames the first-tile rule
    looks at."""
    pl = kc.plan(config, monkeypatch)
    idx = cc.strided_selection(config, pl, groups_bound)
    p = cc.problem(config)
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < p.n_landmark
    assert len(np.unique(idx)) < len(idx)  # with repeats
    for span in (True, False):
        t0 = cc.blocks(config, pl, idx, span=span)
        assert len(t0) > groups_bound
        g = cc.groups(pl, groups_bound // per_cu, len(t0), per_cu)
        assert g == groups_bound, g  # (the workspace cap does not bind on these systems)
        rise, fall = cc.stride_jumps(t0, g)
        print(f"COVCASE {config} bound {groups_bound} span {span}: {len(idx)} indices, {len(t0)} blocks, rise {rise} "
              f"fall {fall}")
        assert rise >= 2 and fall >= 2, (rise, fall)
    # a plain "all" call never strides on these systems: the selection is what makes the loop turn
    assert len(cc.blocks(config, pl)) <= groups_bound


@pytest.mark.parametrize("config", cc.CONFIGS)
def test_reference_pivot(config, monkeypatch):
    """The float64 and the np.longdouble smallest pivot of the reduced system in system order agree to 1e-9 relative."""
    pl = kc.plan(config, monkeypatch)
    p64, pld = cc.ref_pivot(pl, cc.struct_of(config))
    rel = float(abs(np.longdouble(p64) - pld) / pld)
    print(f"COVCASE {config}: min pivot {p64:.17e} (float64) vs longdouble: {rel:.2e} relative; gate {cc.pivot_gate(p64, pld):.1e}")
    assert p64 > 0 and rel <= 1e-9, rel
    assert cc.pivot_gate(p64, pld) == 1e-7


def test_joint_selections(monkeypatch):
    """The joint cases select what they are named for: nd2 every frame (frame 0 among them), wide frames of both parts and
    the separator, nd2_small blocks with differing first tiles."""
    pl = kc.plan("nd2", monkeypatch)
    fr, lm = cc.joint_selection("nd2", pl)
    assert sorted(fr) == list(range(120)) and fr[60] == 0 and len(set(lm)) == 200
    pl = kc.plan("wide", monkeypatch)
    fr, lm = cc.joint_selection("wide", pl)
    tiles = np.asarray(pl["pos"])[fr] // 32
    assert len(set(fr)) == 100 and len(set(lm)) == 300 and tiles.min() == 0 and tiles.max() == 28
    assert len(np.unique(tiles)) >= 9
    pl = kc.plan("nd2_small", monkeypatch)
    fr, lm = cc.joint_selection("nd2_small", pl)
    assert len(set(fr)) == 5 and len(set(lm)) == 5
    for span in (True, False):
        t0 = cc.joint_blocks("nd2_small", pl, fr, lm, span)
        assert len(t0) == 2 and t0[0] != t0[1], t0


def test_scale_problem_strides():
    """The residual-scale case has more records than k_cov_resid_part's 1,024 workgroups of 256 threads take in one
    pass, no pair twice, and residuals on both sides of the unit at f_scale 2.5."""
    p, mult = cc.scale_problem()
    n = len(p.frame)
    assert n > cc.RESID_PARTS * cc.RESID_WG and min(cc.RESID_PARTS, -(-n // cc.RESID_WG)) == cc.RESID_PARTS
    pair = p.frame.astype(np.int64) * p.n_landmark + p.landmark
    assert len(np.unique(pair)) == n
    assert set(np.unique(mult)) == {1.0, 2.0, 3.0}
    r = cc.scale_residuals()
    z = (r / 2.5) ** 2
    share = float(np.mean(z > 1.0))
    print(f"COVCASE scale problem: {n} records, share of z > 1 at f_scale 2.5: {share:.3f}")
    assert 0.0 < share < 1.0
