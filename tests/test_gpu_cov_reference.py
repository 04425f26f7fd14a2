"""The covariance kernels (csrc/cov_kernels.hip: k_cov_tile_inv, k_cov_gram<real, JOINT>, k_cov_cross, k_cov_resid_part;
host side csrc/api_cov.hip) pinned to the dense inverse on the crafted systems of tests/cov_cases.py -- the problems of
tests/k3_cases.py, whose plans reach what the synthetic configs 1 and 2 do not: up to 29 row tiles with most blocks
starting after the first, a sparse tile pattern (8 of 21 to 308 of 406 lower tiles), padding rows, frames straddling a
tile edge, n_aug % 32 == 1 (one live row in the last visited tile) and n_aug % 32 == 0 (the augmented row opens a tile
that is never visited), k_cov_gram's grid-stride loop with a second block that starts above or below the first, and
k_cov_resid_part's own grid-stride loop (more than 1,024 x 256 records), weighted and under every loss.

Reference: C = np.linalg.inv(H), H = cov_ref.normal_matrix at the problem's own (ptz0, rays0) (tests/test_cov_cases.py:
positive definite, scaled condition 2.5e3 - 1.6e5, the dense and the Schur route agree to 2.7e-10 or better).  Metrics:
cov_ref.block_err / cov_joint_ref.joint_err.  Gates: fp64 test_gpu_covariance.TOL[0] = 1e-7; fp32 records
max(TOL[1] = 2e-3, 10 e_round), e_round the same metric between the blocks of the float32-rounded Jacobian and the fp64
reference (computed on the CPU, the rule of test_gpu_k1_paths for max |gradient|); min_pivot max(1e-7, 10 x the
relative float64 - longdouble difference of the reference pivot).  No gate is taken from a GPU result.

Each case sets its configuration's knobs (k3_cases.plan), asserts k3_cases.check_shape on the handle's solver_info()
and prints one line `COVREF ...` with what it measured.  Measured on an MI355X: DESIGN sections 4.7 and 4.7.1."""
import numpy as np
import pytest

import cov_cases as cc
import cov_joint_ref as jref
import cov_ref
import k3_cases as kc
from test_gpu_covariance import TOL

pytestmark = pytest.mark.gpu

FP64, FP32 = 0, 1
KNOB = "PTZBA_COV_WG_PER_CU"


def _open(config, monkeypatch, precision=FP64, loss="linear", f_scale=1.0, per_cu=None, records=None):
    """(handle at the problem's initial state, plan, problem) of a configuration under its knobs; the handle really has
    the shape the configuration is named for.  records: a boolean mask of the records to keep (the coupling window of
    the full record set is then passed, so the plan stays the configuration's)."""
    import ptzba
    pl = kc.plan(config, monkeypatch)  # (sets the plan's knobs)
    if per_cu is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(per_cu))
    p = cc.problem(config)
    h = ptzba.BAHandle(0)
    try:
        _set(h, config, pl, p, precision, loss, f_scale, records)
    except BaseException:
        h.close()
        raise
    return h, pl, p


def _set(h, config, pl, p, precision=FP64, loss="linear", f_scale=1.0, records=None):
    keep = slice(None) if records is None else records
    h.set_problem(p.n_pose, p.n_landmark, p.frame[keep], p.landmark[keep], p.xy[keep], p.u, p.v, precision=precision,
                  loss=loss, f_scale=f_scale, ordering=kc.ordering(config),
                  frame_win_hi=None if records is None else pl["win"])
    kc.check_shape(config, pl, h.solver_info())
    h.set_state(p.init_ptz, p.init_rays)


def _gate(config, precision):
    return TOL[FP64] if precision == FP64 else cc.fp32_gate(cc.e_round(cc.struct_of(config)))


def _n_free(p):
    return 3 * (p.n_pose - 1) + 2 * p.n_landmark


def _check_blocks(pose, ray, pose_ref, ray_ref):
    """(pose error, ray error) after the structure every result has: frame 0 zero, every block symmetric bit for bit."""
    if pose is not None:
        assert not pose[0].any() and pose[1:].reshape(len(pose) - 1, -1).any(axis=1).all()
        assert np.array_equal(pose, pose.transpose(0, 2, 1))
    assert np.array_equal(ray, ray.transpose(0, 2, 1))
    return (cov_ref.block_err(pose, pose_ref) if pose is not None else 0.0), cov_ref.block_err(ray, ray_ref)


@pytest.mark.parametrize("precision", [FP64, FP32])
@pytest.mark.parametrize("config", cc.CONFIGS)
def test_blocks_match_dense_inverse(gpu_available, config, precision, monkeypatch):
    """covariance("all") == the blocks of the dense inverse on every crafted configuration; frame 0 exactly zero, every
    block symmetric bit for bit, n_free exact.

    [wide-1] (fp32 records, scaled condition 1.6e5) is the case that found a defect: with the covariance build on the
    solver's matrix-core K2 it measured pose 3.53e-3, ray 3.56e-3 against the gate of 2e-3 -- the error of the five
    structures grew as 2e-8 x the condition number, and the CPU model of that K2 (cov_cases.k2_model_error), inverted
    densely with no covariance kernel involved, gives the same 3.9e-3, while the float32 slots alone cost 4.8e-5.  The
    covariance build now runs the VALU K2 (csrc/api_cov.hip CovBorrow): 3.2e-5 / 2.5e-5 here.  DESIGN section 4.7."""
    struct = cc.struct_of(config)
    pose_ref, ray_ref = cc.reference_blocks(struct)
    h, pl, p = _open(config, monkeypatch, precision)
    try:
        pose, ray, info = h.covariance("all")
    finally:
        h.close()
    ep, er = _check_blocks(pose, ray, pose_ref, ray_ref)
    gate = _gate(config, precision)
    print(f"COVREF blocks config={config} precision={precision} n_aug={pl['n_aug']} pose={ep:.3e} ray={er:.3e} "
          f"gate={gate:.1e} e_round={cc.e_round(struct):.2e} min_pivot={info['min_pivot']:.6e}")
    assert info["scale"] == 1.0 and info["n_free"] == _n_free(p)
    assert ep <= gate and er <= gate, (ep, er, gate)


def test_huber_weights(gpu_available, monkeypatch):
    """Huber (f_scale 1) on nd2, fp64, against the sqrt(rho')-weighted reference; residuals lie on both sides of the
    unit, and the unweighted reference is far away (the comparison can fail)."""
    import loss_ref
    p = cc.problem("nd2")
    r = loss_ref.records(p, p.init_ptz, p.init_rays, "huber", 1.0)[1]
    beyond = np.abs(r) > 1.0
    assert beyond.any() and not beyond.all()
    pose_ref, ray_ref = cc.reference_blocks("nd2", "huber", 1.0)
    h, pl, p = _open("nd2", monkeypatch, loss="huber", f_scale=1.0)
    try:
        pose, ray, info = h.covariance("all")
    finally:
        h.close()
    ep, er = _check_blocks(pose, ray, pose_ref, ray_ref)
    away = cov_ref.block_err(pose, cc.reference_blocks("nd2")[0])
    print(f"COVREF huber config=nd2 beyond_unit={beyond.mean():.3f} pose={ep:.3e} ray={er:.3e} gate={TOL[FP64]:.1e} "
          f"unweighted_reference={away:.3e}")
    assert info["n_free"] == _n_free(p)
    assert ep <= TOL[FP64] and er <= TOL[FP64], (ep, er)
    assert away > 1e-3


@pytest.mark.parametrize("config", cc.CONFIGS)
def test_min_pivot(gpu_available, config, monkeypatch):
    """info["min_pivot"] == the smallest diagonal entry of the reference Cholesky factor of the reduced system in the
    plan's system order.  Like with like: k_cov_tile_inv reads the factor's diagonal tiles, which hold L_ii -- the pivot
    AFTER the square root -- and the reference takes the diagonal of L as well (not of D = L_ii^2)."""
    p64, pld = cc.ref_pivot(kc.plan(config, monkeypatch), cc.struct_of(config))
    gate = cc.pivot_gate(p64, pld)
    h, pl, p = _open(config, monkeypatch)
    try:
        info = h.covariance(None)[2]
        info_j = h.covariance_joint([1], [0])[1]
    finally:
        h.close()
    rel = float(abs(np.longdouble(info["min_pivot"]) - pld) / pld)
    print(f"COVREF min_pivot config={config} gpu={info['min_pivot']:.17e} reference={p64:.17e} rel={rel:.3e} "
          f"gate={gate:.1e}")
    assert info_j["min_pivot"] == info["min_pivot"]
    assert rel <= gate, (rel, gate)


@pytest.mark.parametrize("config,per_cu,precision", [("nd2", 1, FP64), ("wide", None, FP64), ("nd2", 1, FP32)])
def test_grid_stride_loop(gpu_available, config, per_cu, precision, monkeypatch):
    """More blocks than workgroups in flight: nd2 with PTZBA_COV_WG_PER_CU=1 (set before the handle's first covariance
    call), wide with the knob unset; the selection is sized from the device's CU count.  Under the packing model some
    workgroup's second block starts at least two tiles above its first and some workgroup's at least two below.  (A) the
    ray blocks equal byte for byte ray_all[idx] of a plain covariance("all") on the same handle (which does not stride),
    and the pose blocks likewise: a column of Z depends neither on its block nor on what the workgroup ran before;
    (B) they meet the dense reference at the gate."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    struct = cc.struct_of(config)
    pose_ref, ray_ref = cc.reference_blocks(struct)
    h, pl, p = _open(config, monkeypatch, precision, per_cu=per_cu)
    try:
        eff = cc.COV_WG_PER_CU if per_cu is None else per_cu
        bound = cc.max_groups(pl, cus, eff)
        idx = cc.strided_selection(config, pl, bound)
        jumps = []
        for span in (True, False):
            t0 = cc.blocks(config, pl, idx, span=span)
            g = cc.groups(pl, cus, len(t0), eff)
            assert len(t0) > g == bound, (len(t0), g, bound)
            jumps.append(cc.stride_jumps(t0, g))
            assert min(jumps[-1]) >= 2, jumps
        assert len(cc.blocks(config, pl)) <= bound  # the plain call runs one block per workgroup
        pose_s, ray_s, info_s = h.covariance(idx)
        pose_a, ray_a, info_a = h.covariance("all")
        pose_t, ray_t, _ = h.covariance(idx)
    finally:
        h.close()
    ep, er = _check_blocks(pose_s, ray_s, pose_ref, ray_ref[idx])
    gate = _gate(config, precision)
    same_ray = ray_s.tobytes() == ray_a[idx].tobytes()
    same_pose = pose_s.tobytes() == pose_a.tobytes()
    n_diff = int(np.sum(np.any(ray_s != ray_a[idx], axis=(1, 2))))
    print(f"COVREF stride config={config} per_cu={per_cu} precision={precision} cus={cus} groups={bound} "
          f"indices={len(idx)} blocks={len(t0)} rise/fall={jumps} pose={ep:.3e} ray={er:.3e} gate={gate:.1e} "
          f"bytes_equal pose={same_pose} ray={same_ray} (ray blocks that differ: {n_diff})")
    assert same_ray and same_pose
    assert pose_t.tobytes() == pose_s.tobytes() and ray_t.tobytes() == ray_s.tobytes()  # and again after the plain call
    assert info_s["min_pivot"] == info_a["min_pivot"] and info_s["n_free"] == _n_free(p)
    assert ep <= gate and er <= gate, (ep, er, gate)


@pytest.mark.parametrize("config,precision", [("nd2", FP64), ("wide", FP64), ("nd2_small", FP64), ("nd2", FP32)])
def test_joint_matrix_over_many_tiles(gpu_available, config, precision, monkeypatch):
    """covariance_joint against the whole cut of the dense inverse.  nd2: all 119 free frames in reverse order with frame
    0 among them, 200 landmarks permuted; wide: 100 frames of both dissection parts and the separator, 300 landmarks
    permuted; nd2_small: 5 frames and 5 landmarks whose two blocks start at different tiles (k_cov_cross pairs them from
    the later one).  The 3 x 3 / 2 x 2 diagonal blocks are byte-equal to covariance()'s; frame 0's rows and columns are
    exactly zero; the matrix is symmetric bit for bit."""
    struct = cc.struct_of(config)
    C = cc.inverse(struct)
    h, pl, p = _open(config, monkeypatch, precision)
    try:
        frames, landmarks = cc.joint_selection(config, pl)
        if config == "nd2_small":
            for span in (True, False):
                t0 = cc.joint_blocks(config, pl, frames, landmarks, span)
                assert len(t0) == 2 and t0[0] != t0[1], t0
        else:
            assert len(np.unique(cc.joint_blocks(config, pl, frames, landmarks))) >= 5
        cov, info = h.covariance_joint(frames, landmarks)
        pose, ray, info_b = h.covariance("all")
    finally:
        h.close()
    pidx = jref.param_index(p, frames, landmarks)
    ref = jref.cut(C, pidx)
    err = jref.joint_err(cov, ref)
    nf = 3 * len(frames)
    live = np.diag(ref) > 0
    d = np.sqrt(np.where(live, np.diag(ref), 1.0))
    rel = np.abs(cov - ref) / np.outer(d, d)
    if precision == FP64:
        e_rnd, gate = 0.0, TOL[FP64]
    else:
        e_rnd = jref.joint_err(jref.cut(cc.inverse32(struct), pidx), ref)
        gate = cc.fp32_gate(e_rnd)
    print(f"COVREF joint config={config} precision={precision} shape={cov.shape} joint={err:.3e} "
          f"pose-pose={rel[:nf, :nf].max():.3e} pose-ray={rel[:nf, nf:].max():.3e} ray-ray={rel[nf:, nf:].max():.3e} "
          f"gate={gate:.1e} e_round={e_rnd:.2e}")
    assert cov.tobytes() == cov.T.tobytes()
    for q, f in enumerate(frames):
        blk = cov[3 * q:3 * q + 3, 3 * q:3 * q + 3]
        assert blk.tobytes() == pose[f].tobytes(), f
        if f == 0:
            assert not cov[3 * q:3 * q + 3].any() and not cov[:, 3 * q:3 * q + 3].any()
    if config == "nd2":
        assert 0 in frames
    for q, l in enumerate(landmarks):
        o = nf + 2 * q
        assert cov[o:o + 2, o:o + 2].tobytes() == ray[l].tobytes(), l
    assert info["n_free"] == _n_free(p) and info["min_pivot"] == info_b["min_pivot"]
    assert err <= gate, (err, gate)


def test_singular_system_over_several_tiles(gpu_available, monkeypatch):
    """nd2_small (7 visited row tiles) without the records of one free frame whose rows lie in the last visited tile, then
    of one in a middle tile: covariance and covariance_joint raise "not positive definite" -- an error return, no numbers
    -- and after set_problem with the full records the handle's blocks meet the gate again.  The coupling window of the
    full record set is passed, so the plan (and the frame's tile) stays the configuration's."""
    import ptzba
    config = "nd2_small"
    pose_ref, ray_ref = cc.reference_blocks(config)
    h, pl, p = _open(config, monkeypatch)
    try:
        pos = np.asarray(pl["pos"], np.int64)
        T = cc.shape_facts(pl)["T"]
        for name, tile in (("last", T - 1), ("middle", T // 2)):
            cand = [f for f in range(1, p.n_pose - 1) if pos[f] // 32 == tile]  # (not the last frame: its landmarks are its own)
            assert cand, (name, tile)
            f = cand[0]
            _set(h, config, pl, p, records=p.frame != f)
            assert h.info()["n_obs"] == int(np.sum(p.frame != f)) < len(p.frame)
            with pytest.raises(ptzba.PtzbaError, match="not positive definite"):
                h.covariance("all")
            with pytest.raises(ptzba.PtzbaError, match="not positive definite"):
                h.covariance_joint([f, 1], [0, p.n_landmark - 1])
            _set(h, config, pl, p)
            pose, ray, info = h.covariance("all")
            ep, er = _check_blocks(pose, ray, pose_ref, ray_ref)
            print(f"COVREF singular config={config} frame={f} (tile {tile}, {name}) raised twice; afterwards "
                  f"pose={ep:.3e} ray={er:.3e} gate={TOL[FP64]:.1e}")
            assert ep <= TOL[FP64] and er <= TOL[FP64], (ep, er)
    finally:
        h.close()


def test_residual_scale_beyond_the_partial_sums(gpu_available):
    """covariance(None, scale="residual")["scale"] == sum w rho'(z) r^2 / (2 R - n_free) of loss_ref to 1e-9 relative
    (the gate of test_covariance_at_cauchy_optimum) on 266,000 records: k_cov_resid_part's 1,024 workgroups of 256
    threads take a second record each.  Linear, Huber, soft_l1, Cauchy and arctan at f_scale 2.5, and Cauchy once more
    with integer multiplicities as weight= (rec_w non-null)."""
    import ptzba
    p, mult = cc.scale_problem()
    r = cc.scale_residuals()
    fs = 2.5
    z = (r / fs) ** 2
    share = float(np.mean(z > 1.0))
    assert 0.0 < share < 1.0
    n_free = _n_free(p)
    h = ptzba.BAHandle(0)
    try:
        for loss, weight in (("linear", None), ("huber", None), ("soft_l1", None), ("cauchy", None), ("arctan", None),
                             ("cauchy", mult)):
            h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v, weight=weight, loss=loss,
                          f_scale=fs)
            n_rec = h.info()["n_obs"]
            assert n_rec == len(p.frame) > cc.RESID_PARTS * cc.RESID_WG  # as the handle holds them: nothing merged
            h.set_state(p.init_ptz, p.init_rays)
            pose, none, info = h.covariance(None, scale="residual")
            want = cc.residual_scale(r, loss, fs, n_free, weight)
            rel = abs(info["scale"] - want) / want
            print(f"COVREF scale loss={loss} weighted={weight is not None} records={n_rec} share_beyond_unit={share:.3f} "
                  f"gpu={info['scale']:.12e} reference={want:.12e} rel={rel:.2e}")
            assert none is None and info["n_free"] == n_free and info["min_pivot"] > 0
            assert rel <= 1e-9, (loss, rel)
    finally:
        h.close()
