"""K1 (k_linearize) pinned block-level to a dense fp64 reference on crafted problems (tests/k1_cases.py) that reach, at
~5,500 records: both frame-table paths of a launch (LDS-staged and the global-table fallback of workgroups whose
landmarks span >= 384 frames), landmarks walked in four segment windows with every record-group alignment at a window
boundary, a run over three 256-record batches, one-record / one-segment landmarks, every n_work % 4, weighted records,
and the Huber Hessian / gradient weights at f_scale != 1 and curvature != 1.  Every case asserts through
BAHandle.k1_info() that the launch really took those paths.

Gates (relative; the project's own numbers): fp64 cost 1e-10, step per kind / overall and the step scalars 1e-7;
fp32 cost 2e-6, step and predicted reduction 2e-3, |delta|^2 4e-3, max |gradient| 10x the change that rounding J and r
to float32 makes in the reference (floor 1e-6).  Each case prints its measured errors (DESIGN §4.1 records the worst)."""
import numpy as np
import pytest

import k1_cases as kc

pytestmark = pytest.mark.gpu

LOSSES = {"linear": ("linear", 1.0, 1.0), "huber": ("huber", 1.0, 1.0), "huber_c0.1_s2.5": ("huber", 0.1, 2.5)}
_cache = {}


def _problem(extra, weighted):
    k = ("p", extra, weighted)
    if k not in _cache:
        _cache[k] = kc.craft(extra=extra, weighted=weighted)
    return _cache[k]


def _lin(extra, weighted, loss_id, round32=False):
    """The reference linearisation at x0, computed once per case family and never modified."""
    k = ("lin", extra, weighted, loss_id, round32)
    if k not in _cache:
        loss, hcurv, f_scale = LOSSES[loss_id]
        _cache[k] = kc.linearise(_problem(extra, weighted), loss, hcurv, f_scale, round32=round32)
    return _cache[k]


def _open(p, precision, loss_id):
    """set_problem + the k1_info assertions + set_state (+ curvature) + linearize."""
    import ptzba
    u, v, ptz0, rays0, frame, landmark, xy, weight = p
    loss, hcurv, f_scale = LOSSES[loss_id]
    h = ptzba.BAHandle(0)
    h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, weight=weight, precision=precision,
                  loss=ptzba.LOSS_HUBER if loss == "huber" else ptzba.LOSS_LINEAR, f_scale=f_scale)
    info = h.k1_info()
    assert info[0] == len(rays0) and info[1] == (info[0] + 3) // 4
    assert 1 <= info[2] < info[1], info  # at least one workgroup on either frame-table path
    assert info[3] >= 4, info            # a landmark walked in >= 4 windows
    h.set_state(ptz0, rays0)
    if loss == "huber":
        h.set_huber_curvature(hcurv)
    h.linearize()
    return h, info


def _step(h, lam):
    h.build_reduced(lam)
    h.solve_reduced()
    s = h.read_scalars()
    assert s[5] == 0
    return s


def _delta(ptz1, rays1, ptz0, rays0):
    return np.concatenate([(ptz1 - ptz0)[1:].reshape(-1), (rays1 - rays0).reshape(-1)])


def _rel(a, b):
    return abs(a - b) / abs(b)


def _step_errors(dx_gpu, ref):
    nf = ref["n_free_pose"]
    kg, kr = kc.split_kinds(dx_gpu, nf), kc.split_kinds(ref["dx"], nf)
    err = {k: float(np.abs(kg[k] - kr[k]).max() / np.abs(kr[k]).max()) for k in kr}
    err["all"] = float(np.abs(dx_gpu - ref["dx"]).max() / np.abs(ref["dx"]).max())
    return err


def _gmax_gate(extra, weighted, loss_id):
    """fp32 max |gradient|: 10x the change rounding J and r to float32 makes in the reference's own value, floor 1e-6."""
    g64, g32 = _lin(extra, weighted, loss_id)["gmax"], _lin(extra, weighted, loss_id, round32=True)["gmax"]
    return max(10.0 * abs(g32 - g64) / g64, 1e-6)


@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss_id", list(LOSSES))
@pytest.mark.parametrize("precision", [0, 1])
def test_step_matches_fp64_reference(gpu_available, precision, loss_id, weighted, lam):
    """One (damped) step from x0: cost, the step per parameter kind, predicted reduction, |delta|^2 and max |gradient|
    against the reference; the trial cost (K1 at a second point, into the other linearisation slot) against the
    reference cost at the GPU's own trial state."""
    p = _problem(0, weighted)
    loss, hcurv, f_scale = LOSSES[loss_id]
    ref = kc.reference(p, lam, lin=_lin(0, weighted, loss_id))
    h, info = _open(p, precision, loss_id)
    s = _step(h, lam)
    h.accept(True)
    ptz1, rays1 = h.get_state()
    h.close()
    err = _step_errors(_delta(ptz1, rays1, p[2], p[3]), ref)
    e_cost = _rel(s[0], ref["cost"])
    e_trial = _rel(s[1], kc.cost_at(p, ptz1, rays1, loss, f_scale))
    e_pred, e_dx2, e_g = _rel(s[2], ref["pred"]), _rel(s[3], ref["dx2"]), _rel(s[6], ref["gmax"])
    g_gate = 1e-7 if precision == 0 else _gmax_gate(0, weighted, loss_id)
    print(f"K1PATHS step precision={precision} loss={loss_id} weighted={weighted} lam={lam} k1_info={info} cost={e_cost:.3e} "
          f"trial_cost={e_trial:.3e} dx={ {k: f'{x:.3e}' for k, x in err.items()} } pred={e_pred:.3e} dx2={e_dx2:.3e} "
          f"gmax={e_g:.3e} gmax_gate={g_gate:.3e}")
    c_tol, d_tol, d2_tol = (1e-10, 1e-7, 1e-7) if precision == 0 else (2e-6, 2e-3, 4e-3)
    assert e_cost <= c_tol and e_trial <= c_tol, (e_cost, e_trial)
    assert max(err.values()) <= d_tol, err
    assert e_pred <= d_tol and e_dx2 <= d2_tol, (e_pred, e_dx2)
    assert e_g <= g_gate, (e_g, g_gate)


def test_every_work_count_residue(gpu_available):
    """n_work % 4 = 0..3 (the clamped descriptor reads of the last workgroup and its waves that leave after the barrier):
    fp64, linear loss, undamped step against the reference."""
    seen = set()
    for extra in range(4):
        p = _problem(extra, False)
        ref = kc.reference(p, 0.0, lin=_lin(extra, False, "linear"))
        h, info = _open(p, 0, "linear")
        s = _step(h, 0.0)
        h.accept(True)
        ptz1, rays1 = h.get_state()
        h.close()
        seen.add(info[0] % 4)
        err = _step_errors(_delta(ptz1, rays1, p[2], p[3]), ref)
        e_cost = _rel(s[0], ref["cost"])
        print(f"K1PATHS residue extra={extra} k1_info={info} cost={e_cost:.3e} dx={ {k: f'{x:.3e}' for k, x in err.items()} }")
        assert e_cost <= 1e-10, (extra, e_cost)
        assert max(err.values()) <= 1e-7, (extra, err)
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("precision", [0, 1])
def test_damping_memory_and_rejection(gpu_available, precision):
    """A rejected trial, then a larger lambda on the same linearisation, then a step from the accepted state: each step
    equals the reference with the damping scale D = max(D, diag H) remembered from the first build (Huber, curvature
    0.1, f_scale 2.5)."""
    loss_id = "huber_c0.1_s2.5"
    loss, hcurv, f_scale = LOSSES[loss_id]
    p = _problem(0, False)
    lin = _lin(0, False, loss_id)
    D1 = kc.reference(p, 1e-2, lin=lin)["D"]
    tol = 1e-7 if precision == 0 else 2e-3
    h, info = _open(p, precision, loss_id)
    _step(h, 1e-2)
    h.accept(False)
    ptz_r, rays_r = h.get_state()
    assert np.array_equal(ptz_r, p[2]) and np.array_equal(rays_r, p[3])  # the rejected trial left the state alone
    _step(h, 1e-1)
    h.accept(True)
    ptz1, rays1 = h.get_state()
    ref2 = kc.reference(p, 1e-1, D_prev=D1, lin=lin)
    err2 = _step_errors(_delta(ptz1, rays1, p[2], p[3]), ref2)
    h.linearize()
    s = _step(h, 1e-2)
    h.accept(True)
    ptz2, rays2 = h.get_state()
    h.close()
    lin3 = kc.linearise(p, loss, hcurv, f_scale, ptz1, rays1)
    ref3 = kc.reference(p, 1e-2, D_prev=D1, lin=lin3)
    err3 = _step_errors(_delta(ptz2, rays2, ptz1, rays1), ref3)
    # the memory matters here: without it the reference's third step differs by far more than the fp64 gate
    forget = _step_errors(kc.reference(p, 1e-2, lin=lin3)["dx"], ref3)
    print(f"K1PATHS damping precision={precision} k1_info={info} second={ {k: f'{x:.3e}' for k, x in err2.items()} } "
          f"third={ {k: f'{x:.3e}' for k, x in err3.items()} } cost3={_rel(s[0], lin3['cost']):.3e} "
          f"third_without_memory={forget['all']:.3e}")
    assert (lin3["H"].diagonal() < D1).any() and forget["all"] > 1e-5, forget
    assert max(err2.values()) <= tol, err2
    assert max(err3.values()) <= tol, err3
    assert _rel(s[0], lin3["cost"]) <= (1e-10 if precision == 0 else 2e-6)
