"""CPU checks of the joint covariance feature (ptzba_covariance_joint): the formula the kernels implement,
Cov = D + Z^T Z with L Z = [E_F | -Y_L], equals the dense inverse's sub-matrix; the +Y variant does not (the sign is
pinned, and the GPU tests' metric can fail); the Python binding declares the entry point as include/ptzba.h does."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import cov_joint_ref as jref

HEADER = os.path.join(ROOT, "include", "ptzba.h")


def _selection(cfg, p):
    rng = np.random.default_rng(3)
    frames = rng.permutation(np.arange(1, p.n_pose))
    if cfg == "config1":
        landmarks = rng.permutation(p.n_landmark)
        assert len(frames) == 9 and len(landmarks) == 130
    else:
        from test_gpu_covariance import _config2_landmarks
        landmarks = _config2_landmarks(p)
        assert len(frames) == 49 and len(landmarks) == 50
    return frames, landmarks


@pytest.mark.parametrize("cfg", ["config1", "config2"])
def test_formula_with_minus_y_is_the_dense_inverse(cfg):
    """config 1: all 9 free frames and all 130 rays, shuffled; config 2: all 49 free frames and 50 rays.  The Schur
    form with -Y matches the cut of np.linalg.inv(H) to 1e-10 in the metric (measured 6e-14 / 3e-12: cond(H) 6e6 /
    3e7); with +Y it is off by more than 1 (measured 1.55 / 1.74), far above the GPU tests' 1e-7 / 2e-3."""
    import cov_ref
    p, C = jref.synthetic_inverse(cfg)
    frames, landmarks = _selection(cfg, p)
    ref = jref.cut(C, jref.param_index(p, frames, landmarks))
    H = cov_ref.normal_matrix(p, p.init_ptz, p.init_rays)
    good = jref.joint_err(jref.schur_joint(H, p, frames, landmarks, sign=-1.0), ref)
    wrong = jref.joint_err(jref.schur_joint(H, p, frames, landmarks, sign=+1.0), ref)
    d = np.sqrt(np.diag(ref))
    corr = np.abs(ref) / np.outer(d, d)
    nf = 3 * len(frames)
    off_ray = corr[nf:, nf:].copy()
    for q in range(len(landmarks)):
        off_ray[2 * q:2 * q + 2, 2 * q:2 * q + 2] = 0.0
    print(f"{cfg}: -Y {good:.3e}, +Y {wrong:.3e}; largest correlation pose-ray {corr[:nf, nf:].max():.2f}, "
          f"two rays {off_ray.max():.2f}")
    assert good <= 1e-10, good
    assert wrong > 1.0, wrong


def test_fixed_frames_and_recordless_landmarks_cut_to_zero():
    """The reference's cut: a fixed frame and a landmark named dead give all-zero rows and columns, the rest is the
    inverse's sub-matrix; joint_err refuses a non-zero entry there."""
    p, C = jref.synthetic_inverse("config1")
    idx = jref.param_index(p, [3, 0, 5], [7, 2], dead=(2,))
    assert list(idx[3:6]) == [-1, -1, -1] and list(idx[-2:]) == [-1, -1]
    ref = jref.cut(C, idx)
    assert not ref[3:6].any() and not ref[:, 3:6].any() and not ref[-2:].any()
    assert ref[0, 0] == C[6, 6] and ref[6, 9] == C[12, 3 * 9 + 14]
    assert jref.joint_err(ref, ref) == 0.0
    bad = ref.copy()
    bad[4, 0] = 1e-30
    with pytest.raises(AssertionError):
        jref.joint_err(bad, ref)


def test_binding_declares_covariance_joint_as_the_header():
    import ptzba
    txt = open(HEADER).read()
    m = re.search(r"PTZBA_EXPORT\s+int\s+ptzba_covariance_joint\s*\(([^)]*)\)", txt)
    assert m
    params = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(params) == 8 and params[1].startswith("const ptzba_cov_opts*")
    assert params[3].startswith("int32_t") and params[5].startswith("int32_t")
    m = re.search(r"#define\s+PTZBA_COV_JOINT_MAX_COLS\s+(\d+)", txt)
    assert m and int(m.group(1)) == ptzba.COV_JOINT_MAX_COLS == 2048
    assert "ptzba_covariance_joint" in ptzba.EXPORTED_SYMBOLS
    assert hasattr(ptzba.BAHandle, "covariance_joint") and hasattr(ptzba.BAHandle, "relative_pose_covariance")
    assert hasattr(ptzba.LMSolver, "covariance_joint")
    if os.path.exists(ptzba.LIB_PATH):
        fn = ptzba.lib().ptzba_covariance_joint
        assert len(fn.argtypes) == 8 and fn.restype is ctypes.c_int
        assert fn.argtypes[1] is ctypes.POINTER(ptzba.ptzba_cov_opts)
        assert fn.argtypes[3] is ctypes.c_int32 and fn.argtypes[5] is ctypes.c_int32
        version = ptzba.lib().ptzba_version()
        assert b"ptzba 0.8" in version and b"ptzba_covariance_joint" in version
        assert b"0.2" in version and b"0.3" in version  # (the earlier clauses stay)
        # argument errors need no device: a null handle is "no problem set"
        assert fn(None, None, None, 0, None, 0, None, None) != 0
        assert b"no problem set" in ptzba.lib().ptzba_last_error()
