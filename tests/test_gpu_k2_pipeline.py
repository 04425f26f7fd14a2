"""K2's matrix-core kernel (k_schur_mfp, csrc/schur_kernels.hip: four staging waves, four product waves, an LDS ring
handed over through LDS counters) inside device-driven LM runs: an accepted trial (the alternate linearisation slot)
and repeated resident solves (no ring state survives a launch) come out the same, bit for bit, on two fresh handles
and on every restored solve of one handle.

This arm has no independent reference: the block-synchronous twin kernel these runs used to be compared with is
retired, and what is left here is determinism.  What K2 computes is pinned elsewhere -- the reduced system of the same
problems (and of a build that reads the device-chosen slot) entry by entry to a dense fp64 reference in
tests/test_gpu_k2_reference.py, and these LM sequences with the build's prologue folded into K2 against the prologue
launch, bit for bit, in tests/test_gpu_build_fold.py."""
import numpy as np
import pytest

import k2_cases as k2c

pytestmark = pytest.mark.gpu


def _open(loss):
    import ptzba
    u, v, ptz0, rays0, frame, landmark, xy, _ = k2c.problem("config2")
    h = ptzba.BAHandle(0)
    h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, precision=ptzba.FP32,
                  loss=ptzba.LOSS_HUBER if loss == "huber" else ptzba.LOSS_LINEAR)
    h.set_state(ptz0, rays0)
    return h


def test_alternate_slot_trial_bitwise_equal(gpu_available):
    """One accepted device-driven LM trial: the build reads the linearisation slot the device chose (alt / sel)."""
    out = []
    for _ in range(2):
        h = _open("huber")
        r = h.solve_resident(ftol=1e-14, xtol=1e-16, max_iter=1)
        out.append((h.get_state(), (r.cost, r.njev, r.nfev, r.status)))
        h.close()
    assert out[0][1][1] >= 1 and out[0][1][0] > 0
    for (ptz, rays), res in out[1:]:
        assert res == out[0][1]
        assert np.array_equal(ptz, out[0][0][0]) and np.array_equal(rays, out[0][0][1])
    assert not np.array_equal(out[0][0][0], k2c.problem("config2")[2])  # the trial was accepted: the state moved


def test_repeated_solves_bitwise_equal(gpu_available):
    """Three restored solves of three LM iterations per handle: every launch starts from a clean ring."""
    out = []
    for _ in range(2):
        h = _open("huber")
        h.save_state()
        rs = [h.solve_resident(restore=True, ftol=1e-14, xtol=1e-16, max_iter=3) for _ in range(3)]
        out.append((h.get_state(), [(r.cost, r.njev, r.nfev, r.status) for r in rs]))
        h.close()
    assert out[0][1][0] == out[0][1][1] == out[0][1][2]
    for (ptz, rays), res in out[1:]:
        assert res == out[0][1]
        assert np.array_equal(ptz, out[0][0][0]) and np.array_equal(rays, out[0][0][1])
