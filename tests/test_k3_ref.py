"""The inputs of tests/test_gpu_k3_reference.py are fair, shown without a GPU: the region packing round-trips, the
np.longdouble reference and the fp64 model (tests/k3_ref.py) agree with numpy on a well-conditioned system, every
configuration's plan has the shape it is named for, the model ALONE meets the gates on every (configuration, matrix
family) pair -- so a kernel that misses one has an error the same arithmetic in another order does not have --, and
the gates notice a factor entry that is off by 1e-9 relative, a Minv tile of another solve and a wrong dpose."""
import numpy as np
import pytest

import k2_ref as kr
import k3_cases as kc
import k3_ref as k3


def _setup(config, family, monkeypatch):
    """The plan, the matrix, the augmented system and the reference of a pair (cached: never modified)."""
    pl = kc.plan(config, monkeypatch)
    struct = kc.CONFIGS[config][0]
    m = kc.matrix(struct, family)

    def make():
        D = np.maximum(m["dU"], 1e-12)
        A = k3.augmented(m["S"], m["b"], pl["pos"], pl["ld"], pl["n_aug"], m["lam"], D)
        return A, k3.reference(A, pl["n_aug"])
    A, ref = kc._memo(("ref", config, family), make)
    return pl, m, A, ref


def _model(config, family, form, monkeypatch):
    pl, m, A, ref = _setup(config, family, monkeypatch)

    def make():
        mo = k3.model(A, pl["tasks"], pl["level_off"], pl["n_aug"], form)
        e = k3.metrics(A, pl["n_aug"], k3.frame_rows(pl["pos"]), ref, mo["L"], mo["Minv"], mo["x"])
        return mo, e
    return kc._memo(("model", config, family, form), make)


@pytest.mark.parametrize("config", list(kc.CONFIGS))
def test_plan_has_the_shape_it_is_named_for(config, monkeypatch):
    pl = kc.plan(config, monkeypatch)
    kc.check_shape(config, pl)
    rows = kc.indefinite_rows(pl)
    fp = set(k3.frame_rows(pl["pos"]).tolist())
    assert all(r in fp for r in rows.values()), rows
    assert rows["block_lo"] % 4 == 0 and rows["block_hi"] == rows["block_lo"] + 3 and rows["block_lo"] % 32 >= 4
    if config == "wide":  # the split of a level's task list: the first CHOL_KT by value, the rest through the pointer
        n = np.diff(pl["level_off"])
        assert n.max() == 254 and (n > kc.CHOL_KT).sum() >= 1


@pytest.mark.parametrize("config", list(kc.CONFIGS))
def test_region_pack_round_trips(config, monkeypatch):
    """region_view(region_pack(x)) == x bit for bit, mirrored pairs included; the packed system lies inside the plan's
    fill tiles (so "outside the fill tiles" means "zero" in the GPU test) and is zero from row n_aug on."""
    pl = kc.plan(config, monkeypatch)
    struct = kc.CONFIGS[config][0]
    mirrored = None
    for family in ("well", "graded", "damped"):
        m = kc.matrix(struct, family)
        reg = k3.region_pack(m["S"], m["b"], m["dU"], pl["pos"], pl["ld"], pl["n_aug"], pl["win"], g=m["g"])
        assert len(reg) == pl["ld"] * (pl["ld"] + 3)
        v = kr.region_view(reg, pl["pos"], pl["ld"], pl["n_aug"], pl["win"])
        for k in ("S", "b", "g_pose", "dU"):
            assert np.array_equal(v[k], m["g" if k == "g_pose" else k]), (family, k)
        assert v["rest"] == 0.0 and not v["aug"].any()
        Sr = reg[:pl["ld"] ** 2].reshape(pl["ld"], pl["ld"])
        assert not Sr[pl["n_aug"]:].any()
        low = np.tril(Sr)
        assert not (k3._tiles_nz(low) & ~pl["fill"]).any()
        up = np.triu(Sr, 1)  # upper entries: the diagonal 3 x 3 blocks only (one may straddle two tiles)
        for p in pl["pos"][1:]:
            up[p:p + 3, p:p + 3] = 0.0
        assert not up.any()
        mirrored = v["mirrored"]
    assert (mirrored > 0) == (pl["summary"]["nd_depth"] > 0)  # a dissected order stores pairs mirrored


def test_reference_and_model_agree_with_numpy(monkeypatch):
    pl, m, A, ref = _setup("nd2_small", "well", monkeypatch)
    n = pl["n_aug"]
    Ln = np.linalg.cholesky(A[:n, :n])
    assert np.abs(np.asarray(ref["L"][:n, :n], float) - Ln).max() <= 1e-14
    xn = np.linalg.solve(A[:n, :n], A[n, :n])
    assert np.abs(np.asarray(ref["x"], float) - xn).max() <= 1e-13 * np.abs(xn).max()
    fp = np.sort(k3.frame_rows(pl["pos"]))
    xs = np.asarray(k3.solve_ref(m["S"], m["b"]), float)  # frame order, no padding: the same solution
    assert np.abs(xs - xn[k3.frame_rows(pl["pos"])]).max() <= 1e-13 * np.abs(xn).max()
    assert np.finfo(np.longdouble).eps < 2e-19
    x_by_form = []
    for form in k3.BS_FORMS:
        mo, _ = _model("nd2_small", "well", form, monkeypatch)
        assert np.abs(mo["L"][:n, :n] - Ln).max() <= 1e-13
        assert np.abs(mo["x"] - xn).max() <= 1e-12 * np.abs(xn).max()
        pad = np.setdiff1d(np.arange(n), fp)
        assert len(pad) and not mo["x"][pad].any()  # padding rows: exactly zero
        x_by_form.append(mo["x"])
    assert not np.array_equal(x_by_form[0], x_by_form[1])  # the forms do sum in different orders


@pytest.mark.parametrize("family", kc.FAMILIES)
@pytest.mark.parametrize("config", list(kc.CONFIGS))
def test_model_alone_meets_the_gates(config, family, monkeypatch):
    """The fp64 replay factors every family, and its own metrics meet gate 1 (and, trivially, the gates derived from
    them): the condition that the inputs are fair.  Prints the K3REF model line."""
    pl, m, A, ref = _setup(config, family, monkeypatch)
    for form in k3.BS_FORMS:
        mo, e = _model(config, family, form, monkeypatch)
        g = k3.gates(e, pl["ld"])
        print(k3.line(f"config={config} matrix={family} form={form} model-only", e) + f" gate1={g['bw1']:.2e}")
        k3.check(e, g, family in kc.FORWARD_GATED)
        assert np.isfinite(mo["L"]).all() and np.isfinite(mo["x"]).all()
    if family == "mid":  # the conditioning the family is named for (delta 1e-4: cond ~ 6e4, smallest pivot ~ 1e-2)
        fp = np.sort(k3.frame_rows(pl["pos"]))
        assert 1e4 < np.linalg.cond(A[np.ix_(fp, fp)]) < 1e6
        assert 1e-3 < np.diag(np.asarray(ref["L"], float))[fp].min() < 1e-1
    if family in ("pow2_up", "pow2_down"):  # scale invariance (a report, not a gate)
        s = 200 if family == "pow2_up" else -200
        mo, _ = _model(config, family, "right", monkeypatch)
        mid, _ = _model(config, "mid", "right", monkeypatch)
        fp = k3.frame_rows(pl["pos"])
        same_L = np.array_equal(mo["L"][np.ix_(fp, fp)], np.ldexp(mid["L"][np.ix_(fp, fp)], s))
        print(f"K3REF config={config} matrix={family} model-only L_bitwise_scaled={same_L} "
              f"x_bitwise_same={np.array_equal(mo['x'], mid['x'])}")


def test_damped_reference_remembers_the_larger_scale(monkeypatch):
    """The damped family's second solve lowers dU everywhere: the reference S + lam diag(max(D_prev, dU, 1e-12)) is the
    first solve's, and forgetting D_prev moves the factor by far more than its gate."""
    pl, m, A, ref = _setup("nd2_small", "damped", monkeypatch)
    assert np.all(m["dU2"] < m["dU"])
    A2 = k3.augmented(m["S"], m["b"], pl["pos"], pl["ld"], pl["n_aug"], m["lam"], np.maximum(m["dU2"], 1e-12))
    mo = k3.model(A2, pl["tasks"], pl["level_off"], pl["n_aug"], "right")
    e = k3.metrics(A, pl["n_aug"], k3.frame_rows(pl["pos"]), ref, mo["L"], mo["Minv"], mo["x"])
    _, em = _model("nd2_small", "damped", "right", monkeypatch)
    g = k3.gates(em, pl["ld"])
    assert e["bw"] > 1e6 * g["bw"] and e["L"] > 1e6 * g["L"] and e["x"] > 1e6 * g["x"], (e, g)


MUTATIONS = ("fill_entry_1e-9", "diag_entry_1e-9", "stale_minv", "dpose_1e-9", "y_1e-9")


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("config,family", [("nd2_small", "well"), ("nd2", "mid"), ("wide", "well")])
def test_gates_notice(config, family, mutation, monkeypatch):
    """A result that is off where one Gauss-Newton step at 1e-7 would not show it misses a gate: one entry of a fill
    tile (an update panel skipped or applied twice at an entry of that size) or of a diagonal factor tile off by 1e-9
    relative, a Minv tile left over from another system, one dpose entry or one entry of y off by 1e-9 of the largest."""
    pl, m, A, ref = _setup(config, family, monkeypatch)
    mo, em = _model(config, family, "right", monkeypatch)
    g = k3.gates(em, pl["ld"])
    L, Minv, x = mo["L"].copy(), mo["Minv"].copy(), mo["x"].copy()
    n = pl["n_aug"]
    fp = k3.frame_rows(pl["pos"])
    if mutation == "fill_entry_1e-9":
        # where there is one, a fill tile the injected system does not touch: it holds nothing but update panels
        fillonly = np.argwhere(np.tril(pl["fill"], -1) & ~k3._tiles_nz(np.tril(A)))
        cand = fillonly if len(fillonly) else np.argwhere(np.tril(pl["fill"], -1))
        i, j = (int(v) for v in cand[len(cand) // 2])
        if (i + 1) * 32 > n:
            i, j = (int(v) for v in cand[0])
        t = L[i * 32:(i + 1) * 32, j * 32:(j + 1) * 32]
        r, c = np.unravel_index(np.abs(t).argmax(), t.shape)
        assert t[r, c] != 0 and i * 32 + r < n
        t[r, c] *= 1 + 1e-9
    elif mutation == "diag_entry_1e-9":
        k = int(fp[len(fp) // 2])
        L[k, k] *= 1 + 1e-9
    elif mutation == "stale_minv":
        other, _ = _model(config, "graded" if family != "graded" else "well", "right", monkeypatch)
        Minv[1] = other["Minv"][1]
    elif mutation == "dpose_1e-9":
        x[int(fp[3])] += 1e-9 * np.abs(x).max()
    else:
        L[n, int(fp[5])] += 1e-9 * np.abs(L[n, :n]).max()
    e = k3.metrics(A, n, fp, ref, L, Minv, x)
    with pytest.raises(AssertionError):
        k3.check(e, g, True)
    if family == "well":  # and the step itself moves by less than the 1e-7 of the Gauss-Newton tests
        assert e["x"] < 1e-8
