"""CPU checks of the covariance feature: the reference the GPU tests compare against is itself consistent (two
independent routes), and the Python binding declares ptzba_covariance / ptzba_cov_opts as include/ptzba.h does."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ptzba.h")


def test_reference_routes_agree_config1():
    """np.linalg.inv(J^T J) and the Schur route (S = U - W V^-1 W^T, V^-1 + Y^T S^-1 Y) give the same pose and ray
    blocks at config 1 to 1e-10 in the correlation-scaled metric (cond(S) ~ 5e6: the reference is far tighter than the
    1e-7 / 2e-3 it is used to check); the Huber-weighted form likewise."""
    import synthetic
    import cov_ref
    p = synthetic.make_problem("config1", seed=0)
    for loss, fs in (("linear", 1.0), ("huber", 1.0)):
        pd, rd = cov_ref.dense_blocks(p, p.init_ptz, p.init_rays, loss, fs)
        ps, rs = cov_ref.schur_blocks(p, p.init_ptz, p.init_rays, loss, fs)
        ep, er = cov_ref.block_err(ps, pd), cov_ref.block_err(rs, rd)
        print(f"config1 {loss}: dense vs schur route pose {ep:.3e} ray {er:.3e}")
        assert ep <= 1e-10 and er <= 1e-10, (ep, er)
        assert not pd[0].any() and np.all(np.linalg.eigvalsh(pd[1:]) > 0) and np.all(np.linalg.eigvalsh(rd) > 0)
    # two fixed frames: the blocks of frames 0 and 1 vanish, the rest is the inverse with both poses removed
    p2, _ = cov_ref.dense_blocks(p, p.init_ptz, p.init_rays, n_fixed=2)
    assert not p2[:2].any() and np.all(np.linalg.eigvalsh(p2[2:]) > 0)
    assert np.all(np.diagonal(p2[2:], axis1=1, axis2=2) <= np.diagonal(pd[2:], axis1=1, axis2=2) * (1 + 1e-9))


def _header_struct_fields(name):
    txt = open(HEADER).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", txt)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_binding_declares_covariance_as_the_header():
    import ptzba
    ctypes_of = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    fields = _header_struct_fields("ptzba_cov_opts")
    assert [(n, ctypes_of[t]) for n, t in fields] == list(ptzba.ptzba_cov_opts._fields_)
    assert fields[0] == ("struct_size", "int32_t")
    # the size the header's layout has under the C ABI (4 + 4 + 8, no padding) is what the binding passes
    assert ctypes.sizeof(ptzba.ptzba_cov_opts) == 16
    txt = open(HEADER).read()
    m = re.search(r"PTZBA_EXPORT\s+int\s+ptzba_covariance\s*\(([^)]*)\)", txt)
    assert m
    params = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(params) == 7 and params[1].startswith("const ptzba_cov_opts*") and params[4].startswith("int32_t")
    assert "ptzba_covariance" in ptzba.EXPORTED_SYMBOLS
    if os.path.exists(ptzba.LIB_PATH):
        fn = ptzba.lib().ptzba_covariance
        assert len(fn.argtypes) == 7 and fn.restype is ctypes.c_int
        assert fn.argtypes[1] is ctypes.POINTER(ptzba.ptzba_cov_opts) and fn.argtypes[4] is ctypes.c_int32
        assert b"0.3" in ptzba.lib().ptzba_version()
        # argument errors need no device: a null handle is "no problem set"
        assert fn(None, None, None, None, 0, None, None) != 0
        assert b"no problem set" in ptzba.lib().ptzba_last_error()
