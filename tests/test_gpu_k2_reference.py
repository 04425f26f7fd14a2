"""K2's reduced camera system S | b | g_pose | diag U (k_schur<double>, k_schur_mfp, k_schur_reduce and the
tile / list / split builder of ptzba_set_problem) pinned entry by entry to the dense fp64 reference of tests/k2_ref.py on
the problems of tests/k2_cases.py.  The reference knows no tiles, lists, splits or windows, so what the fp32 and fp64
kernels share is not common-mode here.

Per case: set_problem, set_state, set_huber_curvature, linearize, build_reduced(lam), sync; the exchange region goes
through k2_ref.region_view and is compared with k2_ref.reduced_system.  Metrics (one line `K2REF` per case):
e_S = max over the written entries |S - S_ref|_ij / sqrt(U_ii U_jj); e_b, e_g against the largest reference entry of the
kind (pan / tilt rows, f rows); e_dU entry-wise relative.  Gates: fp64 1e-10 on all four; fp32 10 x max(the error of
the arithmetic model k2_ref.model_mf against the same reference, 1e-6) per metric, and e_S <= 1e-4 besides on every
case but the operand-range ones.  Every case asserts through k2_info() / k2_tile_info() that the builder gave it the
shape tests/k2_ref.tile_plan predicts (and tests/test_k2_ref.py checks that shape against the case's name)."""
import numpy as np
import pytest

import k2_cases as k2c
import k2_ref as kr

pytestmark = pytest.mark.gpu

LOSSES = {"linear": ("linear", 1.0, 1.0), "huber_c0.1_s2.5": ("huber", 0.1, 2.5)}
# the pipeline shapes' losses: the curvature weight 1 is continuous at the Huber unit, so an fp32 branch flip among the
# grid problem's million records cannot move the reference
PIPELINE_LOSSES = {"linear": LOSSES["linear"], "huber_c1_s1": ("huber", 1.0, 1.0)}
LOSS_SETTINGS = dict(LOSSES, **PIPELINE_LOSSES)
FP64, FP32 = 0, 1
KERNELS = {"fp64": FP64, "fp32": FP32}  # k_schur<double> | k_schur_mfp, each with its k_schur_reduce
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _struct(name, ordering=None):
    """The case's coupling window, system positions and tile plan (host only)."""
    import ptzba

    def make():
        p = k2c.problem(name)
        n_pose = len(p[2])
        win = ptzba.frame_coupling_window(n_pose, p[4], p[5])
        pos, _, _, n_aug, _ = ptzba.plan_export(win, 1, ptzba.ORDER_NESTED if ordering is None else ordering)
        return dict(win=win, pos=pos, n_aug=n_aug, mask=kr.written_mask(win),
                    plan=kr.plan_summary(kr.tile_plan(n_pose, p[4], p[5]), n_pose))
    return _memo(("struct", name, ordering), make)


def _ref(name, lam, loss_id, state=None, D_prev=None, tag=None):
    """The reference at the case's x0 (or at `state`, cached under `tag`): computed once, never modified."""
    loss, hcurv, f_scale = LOSS_SETTINGS[loss_id]
    ptz, rays = state if state is not None else (None, None)
    return _memo(("ref", name, lam, loss_id, tag),
                 lambda: kr.reduced_system(k2c.problem(name), lam, loss, hcurv, f_scale, ptz, rays, D_prev))


def _model(name, lam, loss_id, state=None, D_prev=None, tag=None):
    """The arithmetic model's result and its own metrics against the reference."""
    loss, hcurv, f_scale = LOSS_SETTINGS[loss_id]
    ptz, rays = state if state is not None else (None, None)

    def make():
        s = _struct(name)
        m = kr.model_mf(k2c.problem(name), lam, loss, hcurv, f_scale, ptz, rays, D_prev, win=s["win"])
        e = kr.metrics(m, _ref(name, lam, loss_id, state, D_prev, tag), s["mask"])
        return dict(metrics=e, max_hi=m["max_hi"], sub_lo=m["sub_lo"])
    return _memo(("model", name, lam, loss_id, tag), make)


def _open(name, kernel, loss_id, monkeypatch, ordering=None):
    """set_problem + the shape assertions + set_state + curvature + linearize."""
    import ptzba
    precision = KERNELS[kernel]
    u, v, ptz0, rays0, frame, landmark, xy, weight = k2c.problem(name)
    loss, hcurv, f_scale = LOSS_SETTINGS[loss_id]
    h = ptzba.BAHandle(0)
    h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, weight=weight, precision=precision,
                  loss=ptzba.LOSS_HUBER if loss == "huber" else ptzba.LOSS_LINEAR, f_scale=f_scale,
                  ordering=ptzba.ORDER_NESTED if ordering is None else ordering)
    plan = _struct(name, ordering)["plan"]
    got = dict(h.k2_info(), **h.k2_tile_info())
    assert {k: got[k] for k in plan} == plan, (name, got, plan)  # the shape the case is named for really runs
    h.set_state(ptz0, rays0)
    if loss == "huber":
        h.set_huber_curvature(hcurv)
    h.linearize()
    return h


def _view(h, name, ordering=None):
    import torch
    import bench
    h.sync()
    sp, n, _ = h.exchange()
    region = torch.as_tensor(bench._DevArray(sp, n), device="cuda:0").cpu().numpy().copy()
    s = _struct(name, ordering)
    si = h.solver_info()
    assert si["n_aug"] == s["n_aug"] and si["ld"] * (si["ld"] + 3) == n
    return kr.region_view(region, s["pos"], si["ld"], si["n_aug"], s["win"])


def _check(what, name, kernel, loss_id, lam, view, rs, model=None, tight=True, fused=False, extra=""):
    """Print the K2REF line, then hold the gates."""
    want = kr.expected_view(rs, lam, fused)
    ref = dict(rs, S=want["S"])
    e = kr.metrics(view, ref, view["mask"])
    fp64 = KERNELS[kernel] == FP64
    gates = dict.fromkeys(e, kr.FP64_GATE) if fp64 else kr.fp32_gates(model["metrics"])
    line = f"K2REF {what} case={name} kernel={kernel} loss={loss_id} lam={lam:g} " + \
        " ".join(f"e_{k}={e[k]:.3e}" for k in ("S", "b", "g", "dU"))
    if not fp64:
        line += " model " + " ".join(f"{k}={model['metrics'][k]:.3e}" for k in ("S", "b", "g", "dU")) + \
            f" max_hi={model['max_hi']:.1f} subnormal_lo={model['sub_lo']:.3f}"
    print(line + extra)
    assert np.isfinite(view["S"]).all()
    # unwritten entries: the reference has nothing outside the window the library reports, and the region nothing either
    assert np.all(rs["S"][~view["mask"]] == 0.0) and np.all(view["S"][~view["mask"]] == 0.0)
    assert fused or view["rest"] == 0.0  # (a fused prepare puts 1 on the diagonal of padding rows)
    aug_scale = np.abs(rs["b"]).max()
    assert np.abs(view["aug"] - want["aug"]).max() <= (1e-10 if fp64 else gates["b"]) * aug_scale
    for k in e:
        assert e[k] <= gates[k], (k, e, gates)
    if not fp64 and tight:
        assert e["S"] <= 1e-4, e
    return e


def _run(name, kernel, loss_id, lams, monkeypatch, what="build", tight=True, ordering=None):
    h = _open(name, kernel, loss_id, monkeypatch, ordering)
    out = []
    for lam in lams:  # several builds on one linearisation: nothing of an earlier one survives in the written part
        h.build_reduced(lam)
        view = _view(h, name, ordering)
        model = None if KERNELS[kernel] == FP64 else _model(name, lam, loss_id)
        out.append((view, _check(what, name, kernel, loss_id, lam, view, _ref(name, lam, loss_id), model, tight)))
    h.close()
    return out


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("loss_id", list(LOSSES))
@pytest.mark.parametrize("name", ["crafted", "crafted_w"])
def test_crafted_full_matrix(gpu_available, name, loss_id, kernel, monkeypatch):
    """The crafted problem (chunks 0-6, lists of 3-19 landmarks), weighted and not: every kernel, both losses, lambda 0
    and 1e-2 built one after the other on one linearisation."""
    _run(name, kernel, loss_id, (0.0, 1e-2), monkeypatch)


@pytest.mark.parametrize("kernel", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["tiny", "a", "b34", "b65", "b161", "b161gap"])
def test_structure_cases(gpu_available, name, kernel, monkeypatch):
    """One-batch lists, split tiles (ten splits: the reduce's eight-in-flight loop and its remainder; three: the
    remainder alone), ragged last blocks and partner ranges past n_pose, far chunks with and without a middle list."""
    _run(name, kernel, "huber_c0.1_s2.5", (1e-2, 0.0), monkeypatch)


@pytest.mark.parametrize("kernel", ["fp64", "fp32"])
def test_full_lists(gpu_available, kernel, monkeypatch):
    """Lists of SCHUR_LMAX = 512 landmarks: 32 batches, the longest fp32 accumulation, 256 splits of one tile."""
    assert _struct("c")["plan"]["nl_max"] == 512 and _struct("c")["plan"]["splits_max"] == 256
    _run("c", kernel, "huber_c0.1_s2.5", (1e-2,), monkeypatch)


@pytest.mark.parametrize("kernel", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["a", "b161", "b161gap", "crafted"])
def test_both_orders(gpu_available, name, kernel, monkeypatch):
    """ORDER_NATURAL and ORDER_NESTED_FORCE: the natural order stores no block mirrored; the dissected order of (a) and
    of the far-chunk problem without an all-frame landmark does (pairs with pos[f2] < pos[f1], counted from the plan's
    positions), and the frame-order view equals the reference either way.  A landmark seen by every frame couples every
    frame to the last: (b, 161) and the crafted problem admit the natural order only, under either setting."""
    import ptzba
    mirrored = {}
    for o in (ptzba.ORDER_NATURAL, ptzba.ORDER_NESTED_FORCE):
        (view, _), = _run(name, kernel, "huber_c0.1_s2.5", (1e-2,), monkeypatch, what=f"order{o}", ordering=o)
        mirrored[o] = view["mirrored"]
    print(f"K2REF mirrored pairs case={name}: {mirrored}")
    assert mirrored[ptzba.ORDER_NATURAL] == 0
    assert (mirrored[ptzba.ORDER_NESTED_FORCE] > 0) == (name in ("a", "b161gap"))


@pytest.mark.parametrize("kernel", ["fp64", "fp32"])
@pytest.mark.parametrize("name", list(k2c.E_VARIANTS))
def test_operand_ranges(gpu_available, name, kernel, monkeypatch):
    """f in {800, 3000, 20000}, a 700-record segment beside single records, outliers of 300 / 1000 px under Huber, the
    two worst together; lambda 0, 1e-2 and 1e3.  The model shows every operand inside fp16's range before the build."""
    lams = (0.0, 1e-2, 1e3)
    for lam in lams:
        assert _model(name, lam, "huber_c0.1_s2.5")["max_hi"] < 65504
    _run(name, kernel, "huber_c0.1_s2.5", lams, monkeypatch, tight=False)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kernel", ["fp64", "fp32"])
def test_region_layouts(gpu_available, kernel, fused, monkeypatch):
    """What the region holds (include/ptzba.h, ptzba_exchange): raw after ptzba_build_reduced with or without
    PTZBA_NO_FUSED_PREP; after a build of the device-driven LM lambda D_pose on the pose diagonal and b^T in row n_aug
    (the fused prepare of k_schur_reduce), raw again with PTZBA_NO_FUSED_PREP=1."""
    import ptzba
    name, loss_id, lam = "crafted", "linear", 1e-2
    if fused:
        monkeypatch.delenv("PTZBA_NO_FUSED_PREP", raising=False)
    else:
        monkeypatch.setenv("PTZBA_NO_FUSED_PREP", "1")
    rs = _ref(name, lam, loss_id)
    model = None if kernel == "fp64" else _model(name, lam, loss_id)
    h = _open(name, kernel, loss_id, monkeypatch)
    h.build_reduced(lam)
    _check(f"host_build fused_env={fused}", name, kernel, loss_id, lam, _view(h, name), rs, model)
    h.close()
    # a fresh handle: once a caller has taken the region's pointer (ptzba_exchange, as _view does) the library assumes
    # that it sums the system between build and solve and no longer fuses the prepare into the build
    h = _open(name, kernel, loss_id, monkeypatch)
    h.lm_start()
    h.lm_init(ptzba.ptzba_lm_opts(1e-14, 1e-16, 0.0, lam, 1e-12, 1e16, 1, 30, 0, 1.0, 0.0))
    h.lm_build()
    view = _view(h, name)
    h.close()
    _check(f"lm_build fused_env={fused}", name, kernel, loss_id, lam, view, rs, model, fused=fused)
    if fused:  # the damping on the diagonal is lam D_pose = lam max(0, dU): it is there, and it is not small
        d = np.arange(len(rs["b"]))
        assert np.all(view["S"][d, d] - rs["S"][d, d] > 0.5 * lam * rs["dU"])


@pytest.mark.parametrize("kernel", ["fp64", "fp32"])
def test_second_point_and_damping_memory(gpu_available, kernel, monkeypatch):
    """step(1e-2), accept, linearize, build_reduced(1e-2): the region equals the reference at the accepted state (the
    other linearisation slot) with the rays' damping scale D = max(D, diag V) remembered from the first build; without
    the memory the reference itself moves by more than the gate.  (ptzba_build_reduced leaves the pose diagonal
    undamped, so the pose scale's memory shows in a step, where tests/test_gpu_k1_paths.py holds it, not here.)"""
    name, loss_id, lam = "crafted", "huber_c0.1_s2.5", 1e-2
    D1 = _ref(name, lam, loss_id)["D"]
    h = _open(name, kernel, loss_id, monkeypatch)
    h.step(lam)
    s = h.read_scalars()
    assert s[5] == 0
    h.accept(True)
    state = h.get_state()
    p = k2c.problem(name)
    assert not np.array_equal(state[0], p[2])
    h.linearize()
    h.build_reduced(lam)
    view = _view(h, name)
    h.close()
    tag = ("second", kernel)  # the accepted state differs between the precisions
    rs = _ref(name, lam, loss_id, state, D1, tag)
    model = None if kernel == "fp64" else _model(name, lam, loss_id, state, D1, tag)
    e = _check("second_point", name, kernel, loss_id, lam, view, rs, model)
    loss, hcurv, f_scale = LOSS_SETTINGS[loss_id]
    rs_forgot = kr.reduced_system(p, lam, loss, hcurv, f_scale, state[0], state[1])
    forgot = kr.metrics(rs_forgot, rs, view["mask"])
    gate = kr.FP64_GATE if kernel == "fp64" else kr.fp32_gates(model["metrics"])["S"]
    print(f"K2REF second_point kernel={kernel} without_memory e_S={forgot['S']:.3e} gate={gate:.3e}")
    n3 = len(rs["b"])
    assert (rs["D"][n3:] > rs_forgot["D"][n3:]).any()  # some ray's scale is the remembered one
    assert forgot["S"] > gate >= e["S"]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("loss_id", list(PIPELINE_LOSSES))
@pytest.mark.parametrize("name", k2c.PIPELINE_NAMES)
def test_pipeline_shapes(gpu_available, name, loss_id, kernel, monkeypatch):
    """The four problems that together run every shape of k_schur_mfp's hand-off (see
    test_problems_cover_the_pipeline_shapes), lambda 0 and 1e-3 built one after the other.  The model's own error on
    them is e_S <= 3.8e-7 and <= 2.3e-7 in the other metrics, so every fp32 gate is 10 x 1e-6 = 1e-5 (measured on
    MI355X: fp32 e_S <= 2.1e-6, fp64 <= 2.3e-13 in every metric)."""
    _run(name, kernel, loss_id, (0.0, 1e-3), monkeypatch, what="pipeline")


def test_problems_cover_the_pipeline_shapes(gpu_available, monkeypatch):
    """The four problems together run every shape of the hand-off: a single batch (nothing to re-fill), an odd batch
    count beyond it (the batch staged after the two-batch loop), an even one, ragged last batches, and items with
    and without the diagonal terms."""
    infos = {}
    for name in k2c.PIPELINE_NAMES:
        h = _open(name, "fp32", "linear", monkeypatch)
        infos[name] = h.k2_info()
        h.close()
        print(f"K2PIPE k2_info {name}: {infos[name]}")
    for name, i in infos.items():
        assert i["items"] >= 1 and 1 <= i["nl_min"] <= i["nl_max"] <= 512, (name, i)
        assert i["nl_mod32_1_16"] + i["nl_mod32_17_31"] + i["nl_mod32_0"] == i["items"], (name, i)
        assert 1 <= i["chunk0_items"] <= i["items"], (name, i)
    t = infos["tiny"]
    assert t["nl_max"] <= 16 and t["nl_le16"] == t["items"] and t["chunk0_items"] < t["items"], t
    tot = {k: sum(i[k] for i in infos.values()) for k in infos["tiny"]}
    assert tot["nl_le16"] > 0                            # one batch
    assert tot["nl_mod32_1_16"] - tot["nl_le16"] > 0     # 3, 5, ... batches
    assert tot["nl_mod32_17_31"] + tot["nl_mod32_0"] > 0  # an even batch count
    assert tot["nl_mod32_17_31"] > 0                     # ... with a ragged last batch
    assert any(i["nl_min"] % 16 for i in infos.values())
    assert tot["chunk0_items"] > 0 and tot["items"] - tot["chunk0_items"] > 0
    assert infos["grid"]["nl_min"] > 4 * 16              # more batches than ring buffers: every item re-fills them


@pytest.mark.parametrize("kernel", ["fp64", "fp32"])
def test_device_chosen_slot(gpu_available, kernel, monkeypatch):
    """A build that reads the linearisation slot picked on the device (SchurArgs::sel): one device-driven LM trial from
    lambda 1e-2, accepted by lm_decide, then the next trial's build.  Its region (fused layout) equals the reference
    at the accepted state, at the damping the decision left, with the damping scales remembered from the first build
    (as test_second_point_and_damping_memory shows for the host-step path).  fp32: both builds had the prologue folded
    into K2, so the slot was read by k_schur_mfp's own list build as well.  Measured on MI355X: fp32 e_S 2.0e-6, e_g
    6.3e-6 (gates 1e-5, 1.3e-5); fp64 e_g 9.5e-11 of the 1e-10 gate -- after the accepted step the gradient is a small
    difference of large terms, and g_pose carries that cancellation in kernel and reference alike."""
    import ptzba
    name, loss_id, lam0 = "crafted", "linear", 1e-2
    D1 = _ref(name, lam0, loss_id)["D"]
    h = _open(name, kernel, loss_id, monkeypatch)
    h.lm_start()
    h.lm_init(ptzba.ptzba_lm_opts(1e-14, 1e-16, 0.0, lam0, 1e-12, 1e16, 3, 30, 0, 1.0, 0.0))
    h.lm_build()
    h.lm_solve()
    h.lm_decide(0)
    h.lm_build()
    rec = h.lm_wait(0)
    assert rec.accepted == 1 and rec.done == 0, (rec.accepted, rec.done, rec.status)
    lam = float(rec.lam)
    state = h.get_state()
    assert not np.array_equal(state[0], k2c.problem(name)[2])
    info = h.build_info()
    view = _view(h, name)
    h.close()
    if kernel == "fp32":
        assert info["folded_builds"] == 2 and info["prologue_builds"] == 0, info
    tag = ("device_slot", kernel)  # the accepted state differs between the precisions
    rs = _ref(name, lam, loss_id, state, D1, tag)
    model = None if kernel == "fp64" else _model(name, lam, loss_id, state, D1, tag)
    _check("device_slot", name, kernel, loss_id, lam, view, rs, model, fused=True)
