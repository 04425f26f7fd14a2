"""K1's merged record stream (ptzba_k1_merge_info) on crafted problems of a few thousand records: the merged count
against numpy's statement of the run rule (tests/test_k1_merge_cpu.py), one step against the dense fp64 reference of
tests/k1_cases.py at the gates of test_gpu_k1_paths.py, and against the same problem under PTZBA_K1_MERGE=0.

Shapes (each asserted through the info query and the numpy rule): every segment one run -- with single-record segments
and a 700-record segment that becomes one record --, segments A A B A (adjacent-only merging), user weights times
multiplicities (constant inside runs, and weights that split runs), a landmark of more than 128 segments (several
windows), problems just below and just above the halving rule, n_work % 4 taking every value.

Gates (relative): fp64 cost 1e-10, step and step scalars 1e-7; fp32 cost 2e-6, step and predicted reduction 2e-3,
|delta|^2 4e-3.  Merged against unmerged, fp64: GATE_REORDER (10 x the worst measured, floor 1e-13: the two differ in
the order of the per-segment sums only).  lm_out is not readable through the C-ABI: the fronts and the knob are compared
through everything formed from it -- the step scalars and the state after the step, bitwise.

The readers that keep the unmerged arrays -- ptzba_residual, the covariance's residual scale and degrees of freedom,
ptzba_marginal_prior with a drop mask that splits runs -- and dedup-form input are bitwise equal to the knob-off
handle."""
import contextlib
import os

import numpy as np
import pytest

import k1_cases as kc
from reuse_cases import N_POSE, pair_form as craft, segments as _segments  # noqa: F401  (shared with the reuse tests)
from test_k1_merge_cpu import numpy_runs

pytestmark = pytest.mark.gpu

LOSSES = {"linear": ("linear", 1.0, 1.0), "huber": ("huber", 1.0, 1.0), "huber_c0.1_s2.5": ("huber", 0.1, 2.5)}
# merged against unmerged (and the one-record form against the general kernel) in fp64, relative: 10 x the worst
# measured over this file's cases, floor 1e-13.  Measured: cost 1.7e-16, trial cost 2.6e-15, the step scalars 2.3e-14,
# the step per parameter kind 1.09e-13
GATE_REORDER = {"cost": 1e-13, "step": 1.1e-12, "scalar": 2.4e-13}
_cache = {}


@contextlib.contextmanager
def _knob_off(name="PTZBA_K1_MERGE"):
    old = os.environ.get(name)
    os.environ[name] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _lin(shape, extra, loss_id):
    k = ("lin", shape, extra, loss_id)
    if k not in _cache:
        loss, hcurv, f_scale = LOSSES[loss_id]
        _cache[k] = kc.linearise(craft(shape, extra), loss, hcurv, f_scale)
    return _cache[k]


def _open(p, precision, loss="linear", hcurv=1.0, f_scale=1.0, merge=True, front=None, one=True):
    import ptzba
    u, v, ptz0, rays0, frame, landmark, xy, weight = p
    ids = {"linear": ptzba.LOSS_LINEAR, "huber": ptzba.LOSS_HUBER, "cauchy": ptzba.LOSS_CAUCHY}
    h = ptzba.BAHandle(0)
    if front is not None:
        h.set_setup_front(front)
    with (contextlib.nullcontext() if merge else _knob_off()), \
            (contextlib.nullcontext() if one else _knob_off("PTZBA_K1_ONE")):
        h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, weight=weight, precision=precision,
                      loss=ids[loss], f_scale=f_scale)
    h.set_state(ptz0, rays0)
    if loss != "linear":
        h.set_huber_curvature(hcurv)
    h.linearize()
    return h


def _step(h, lam):
    h.build_reduced(lam)
    h.solve_reduced()
    s = np.array(h.read_scalars(), np.float64)
    assert s[5] == 0
    h.accept(True)
    ptz1, rays1 = h.get_state()
    return s, ptz1, rays1


def _expect_runs(p, precision):
    _, first, _ = numpy_runs(len(p[2]), p[4], p[5], p[6], p[7], precision)
    return len(first)


def _assert_shape(h, p, precision, merged=True):
    mi = h.k1_merge_info()
    runs, used = mi["runs"], mi["merged"]
    assert runs == _expect_runs(p, precision), (runs, _expect_runs(p, precision))
    assert used == merged and used == (2 * runs <= len(p[4])), (runs, len(p[4]), used)
    assert h.info()["n_obs"] == len(p[4])  # the caller's record count, whatever K1 reads
    # the one-record form of the kernel exactly when every segment is one run
    assert mi["one_record"] == (used and runs == h.info()["n_segments"])
    return runs


def _rel(a, b):
    return abs(a - b) / abs(b)


def _delta(ptz1, rays1, p):
    return np.concatenate([(ptz1 - p[2])[1:].reshape(-1), (rays1 - p[3]).reshape(-1)])


def _against_reference(tag, p, precision, loss_id, lam, s, ptz1, rays1, ref):
    loss, hcurv, f_scale = LOSSES[loss_id]
    dx = _delta(ptz1, rays1, p)
    nf = ref["n_free_pose"]
    kg, kr = kc.split_kinds(dx, nf), kc.split_kinds(ref["dx"], nf)
    err = {k: float(np.abs(kg[k] - kr[k]).max() / np.abs(kr[k]).max()) for k in kr}
    e_cost = _rel(s[0], ref["cost"])
    e_trial = _rel(s[1], kc.cost_at(p, ptz1, rays1, loss, f_scale))
    e_pred, e_dx2 = _rel(s[2], ref["pred"]), _rel(s[3], ref["dx2"])
    print(f"K1MERGE {tag} precision={precision} loss={loss_id} lam={lam} cost={e_cost:.3e} trial_cost={e_trial:.3e} "
          f"dx={ {k: f'{x:.3e}' for k, x in err.items()} } pred={e_pred:.3e} dx2={e_dx2:.3e}")
    c_tol, d_tol, d2_tol = (1e-10, 1e-7, 1e-7) if precision == 0 else (2e-6, 2e-3, 4e-3)
    assert e_cost <= c_tol and e_trial <= c_tol, (e_cost, e_trial)
    assert max(err.values()) <= d_tol, err
    assert e_pred <= d_tol and e_dx2 <= d2_tol, (e_pred, e_dx2)


def _against_unmerged(tag, precision, a, b, p, what="merged-vs-unmerged"):
    """a, b = (scalars, ptz1, rays1) of two handles after the same step from p's x0: cost and trial cost, the step
    scalars (predicted reduction, |delta|^2, max |gradient|) and the step per parameter kind, relative."""
    e_cost, e_trial = _rel(a[0][0], b[0][0]), _rel(a[0][1], b[0][1])
    e_sc = max(_rel(a[0][k], b[0][k]) for k in (2, 3, 6))
    nf = len(p[2]) - 1
    ka, kb = kc.split_kinds(_delta(a[1], a[2], p), nf), kc.split_kinds(_delta(b[1], b[2], p), nf)
    e_dx = max(float(np.abs(ka[k] - kb[k]).max() / np.abs(kb[k]).max()) for k in kb)
    print(f"K1MERGE {tag} precision={precision} {what} cost={e_cost:.3e} trial_cost={e_trial:.3e} "
          f"scalars={e_sc:.3e} step={e_dx:.3e}")
    if precision == 0:
        assert max(e_cost, e_trial) <= GATE_REORDER["cost"], (e_cost, e_trial)
        assert e_dx <= GATE_REORDER["step"] and e_sc <= GATE_REORDER["scalar"], (e_dx, e_sc)


# ------------------------------------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("loss_id", list(LOSSES))
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("shape", ["one_run", "aaba", "w_const", "w_split"])
def test_merged_step_matches_reference_and_unmerged(gpu_available, shape, precision, loss_id, lam):
    p = craft(shape)
    loss, hcurv, f_scale = LOSSES[loss_id]
    n = len(p[4])
    start = _segments(p[4], p[5])[3]
    cnt = np.diff(np.flatnonzero(np.concatenate([start, [True]])))
    assert cnt.max() == 700 and (cnt == 1).any() and n < 4000  # the long run, single-record segments
    h = _open(p, precision, loss, hcurv, f_scale)
    runs = _assert_shape(h, p, precision)
    if shape in ("one_run", "w_const"):
        assert runs == len(cnt)  # every segment one run: the 700-record segment is one record
    elif shape == "aaba":
        assert runs == len(cnt) + 2 * int((cnt >= 4).sum()) and (cnt >= 4).sum() >= 2  # A A | B | A ...: three runs
    else:
        assert len(cnt) < runs
    a = _step(h, lam)
    h.close()
    _against_reference(shape, p, precision, loss_id, lam, *a, kc.reference(p, lam, lin=_lin(shape, 0, loss_id)))
    h0 = _open(p, precision, loss, hcurv, f_scale, merge=False)
    assert h0.k1_merge_info() == {"runs": n, "merged": False, "one_record": False}
    b = _step(h0, lam)
    h0.close()
    _against_unmerged(shape, precision, a, b, p)


@pytest.mark.parametrize("precision", [0, 1])
def test_newer_loss_merged_against_unmerged(gpu_available, precision):
    """Cauchy (robust_loss.h): the merged stream against the knob-off handle, damped step, curvature floor 0.1."""
    p = craft("w_const")
    out = []
    for merge in (True, False):
        h = _open(p, precision, "cauchy", 0.1, 2.5, merge=merge)
        assert h.k1_merge_info()["merged"] == merge
        out.append(_step(h, 1e-2))
        h.close()
    _against_unmerged("cauchy", precision, *out, p)
    if precision == 1:  # both are fp32 roundings of one cost: the fp32 gates of the reference comparison, between them
        assert _rel(out[0][0][0], out[1][0][0]) <= 2e-6
        assert np.abs(out[0][1] - out[1][1]).max() <= 2e-3 * np.abs(out[1][1] - p[2]).max()


@pytest.mark.parametrize("precision", [0, 1])
def test_every_work_count_residue(gpu_available, precision):
    seen = set()
    for extra in range(4):
        p = craft("one_run", extra)
        h = _open(p, precision)
        _assert_shape(h, p, precision)
        seen.add(h.k1_info()[0] % 4)
        a = _step(h, 0.0)
        h.close()
        _against_reference(f"residue extra={extra}", p, precision, "linear", 0.0, *a,
                           kc.reference(p, 0.0, lin=_lin("one_run", extra, "linear")))
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("shape", ["below_half", "above_half"])
def test_halving_rule(gpu_available, shape, precision):
    """runs == floor(R / 2): merged; one run more: the unmerged stream, bitwise the knob-off handle."""
    p = craft(shape)
    n = len(p[4])
    h = _open(p, precision)
    runs = _assert_shape(h, p, precision, merged=shape == "below_half")
    assert runs == n // 2 + (shape == "above_half")
    a = _step(h, 1e-2)
    h.close()
    _against_reference(shape, p, precision, "linear", 1e-2, *a, kc.reference(p, 1e-2, lin=_lin(shape, 0, "linear")))
    h0 = _open(p, precision, merge=False)
    b = _step(h0, 1e-2)
    h0.close()
    if shape == "above_half":
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    else:
        _against_unmerged(shape, precision, a, b, p)


@pytest.mark.parametrize("one", [True, False])
@pytest.mark.parametrize("precision", [0, 1])
def test_landmarks_crossing_the_window(gpu_available, precision, one):
    """Landmarks of up to 256 segments (pair form: every segment one run) against the reference on the de-duplicated,
    weighted statement of the same cost."""
    import synthetic
    q = synthetic.make_small_problem(260, 80, 50.0, 52.0, seed=5)
    p = (q.u, q.v, q.init_ptz, q.init_rays, q.frame, q.landmark, q.xy, None)
    if "win" not in _cache:
        fr, lm, xy, w, _ = synthetic.dedup_records(q.frame, q.landmark, q.xy)
        pd = (q.u, q.v, q.init_ptz, q.init_rays, fr, lm, xy, w)
        _cache["win"] = (pd, kc.reference(pd, 0.0))
    pd, ref = _cache["win"]
    h = _open(p, precision, one=one)  # (one=False: the general kernel walks the merged stream in several windows)
    assert h.info()["max_seg_per_landmark"] > 128 and h.k1_info()[3] >= 2
    mi = h.k1_merge_info()
    assert mi["merged"] and mi["one_record"] == one and mi["runs"] == _expect_runs(p, precision) == h.info()["n_segments"]
    a = _step(h, 0.0)
    h.close()
    _against_reference(f"window one_record={one}", pd, precision, "linear", 0.0, *a, ref)


@pytest.mark.parametrize("loss_id", ["linear", "huber_c0.1_s2.5"])
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("shape", ["one_run", "w_const"])
def test_one_record_form_against_general_merged_path(gpu_available, shape, precision, loss_id):
    """Every segment one run: k_linearize's one-record form, against the reference and against the general kernel on
    the same merged stream (PTZBA_K1_ONE=0); a problem with three-run segments takes the general kernel."""
    p = craft(shape)
    loss, hcurv, f_scale = LOSSES[loss_id]
    out = []
    for one in (True, False):
        h = _open(p, precision, loss, hcurv, f_scale, one=one)
        assert h.k1_merge_info()["merged"] and h.k1_merge_info()["one_record"] == one
        out.append(_step(h, 1e-2))
        h.close()
        _against_reference(f"{shape} one_record={one}", p, precision, loss_id, 1e-2, *out[-1],
                           kc.reference(p, 1e-2, lin=_lin(shape, 0, loss_id)))
    _against_unmerged(shape, precision, *out, p, what="one-record-vs-general")
    h = _open(craft("aaba"), precision, loss, hcurv, f_scale)
    assert h.k1_merge_info()["merged"] and not h.k1_merge_info()["one_record"]
    h.close()


# ------------------------------------------------------------------------------------------------ bitwise
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("shape", ["aaba", "w_split"])
def test_host_and_device_fronts_bitwise_equal(gpu_available, shape, precision):
    p = craft(shape)
    out = []
    for front in (0, 2 ** 40):  # the device front always / never
        h = _open(p, precision, "huber", 0.1, 2.5, front=front)
        out.append((h.k1_merge_info(), _step(h, 1e-2)))
        h.close()
    assert out[0][0] == out[1][0] and out[0][0]["merged"]
    assert all(np.array_equal(x, y) for x, y in zip(out[0][1], out[1][1]))


@pytest.mark.parametrize("precision", [0, 1])
def test_unmerged_readers_bitwise_equal_to_knob_off(gpu_available, precision):
    """ptzba_residual, the covariance's residual scale and degrees of freedom, ptzba_marginal_prior with a drop mask
    that splits runs: they read the unmerged arrays."""
    p = craft("w_const")
    u, v, ptz0, rays0, frame, landmark, xy, weight = p
    x_full = np.concatenate([ptz0.reshape(-1), rays0.reshape(-1)])
    mask = (frame == 0) & (np.arange(len(frame)) % 2 == 0)  # every other record of the leaving frame
    _, first, mult = numpy_runs(len(ptz0), frame, landmark, xy, weight, precision)
    o = _segments(frame, landmark)[0]
    sm = mask[o]
    starts = np.flatnonzero(np.isin(o, first))
    split = [s for s, m in zip(starts, mult) if m >= 2 and 0 < sm[s:s + m].sum() < m]
    assert split  # a run with dropped and kept records
    out = []
    for merge in (True, False):
        h = _open(p, precision, "huber", 1.0, 2.5, merge=merge)
        assert h.k1_merge_info()["merged"] == merge
        r = h.residual(x_full)
        pose_cov, _, ci = h.covariance(scale="residual")
        m, st = h.marginal_prior([0], drop_mask=mask.astype(np.uint8))
        out.append((r, ci["scale"], ci["n_free"], pose_cov, m, st["dropped_records"]))
        h.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[5] == b[5] == int(mask.sum())
    assert np.array_equal(a[4].frames, b[4].frames) and np.array_equal(a[4].info, b[4].info)
    assert np.array_equal(a[4].grad, b[4].grad) and a[4].offset == b[4].offset
    # the covariance itself is formed from K1's linearisation (merged): equal to rounding, not bitwise
    np.testing.assert_allclose(a[3], b[3], rtol=1e-8 if precision == 0 else 2e-3, atol=0)


@pytest.mark.parametrize("precision", [0, 1])
def test_dedup_form_is_untouched(gpu_available, precision):
    """De-duplicated weighted input has no repeats: the merged stream is not built and every bit equals the knob-off
    handle's."""
    import synthetic
    u, v, ptz0, rays0, frame, landmark, xy, _ = craft("one_run")
    fr, lm, xd, w, _ = synthetic.dedup_records(frame, landmark, xy)
    p = (u, v, ptz0, rays0, fr, lm, xd, w)
    out = []
    for merge in (True, False):
        h = _open(p, precision, "huber", 0.1, 2.5, merge=merge)
        assert h.k1_merge_info() == {"runs": len(fr), "merged": False, "one_record": False}
        out.append(_step(h, 1e-2))
        h.close()
    assert all(np.array_equal(x, y) for x, y in zip(*out))
