"""CPU tests of the K2 reference, the region map and the arithmetic model (tests/k2_ref.py, tests/k2_cases.py): the
reference reproduces k1_cases.reference's step, the coupling window loses nothing, the fp16 split is the documented
one, the cases have the structure they are named for, and the fp32 gate of tests/test_gpu_k2_reference.py notices
every deliberately wrong kernel."""
import numpy as np
import pytest

import k1_cases as kc
import k2_cases as k2c
import k2_ref as kr

_cache = {}


def _win(name):
    import ptzba
    if ("win", name) not in _cache:
        p = k2c.problem(name)
        _cache["win", name] = ptzba.frame_coupling_window(len(p[2]), p[4], p[5])
    return _cache["win", name]


def _plan(name):
    if ("plan", name) not in _cache:
        p = k2c.problem(name)
        _cache["plan", name] = kr.tile_plan(len(p[2]), p[4], p[5])
    return _cache["plan", name]


@pytest.mark.parametrize("loss_id", [("linear", 1.0, 1.0), ("huber", 0.1, 2.5)])
@pytest.mark.parametrize("lam", [0.0, 1e-2])
def test_reduced_solve_reproduces_the_dense_step(lam, loss_id):
    """(S + lam D_pose) dx = b and the rays' back-substitution against the dense solve of k1_cases.reference."""
    loss, hcurv, f_scale = loss_id
    p = k2c.problem("crafted")
    ref = kc.reference(p, lam, loss, hcurv, f_scale)
    rs = kr.reduced_system(p, lam, loss, hcurv, f_scale)
    dx = kr.solve_step(rs, lam)
    err = float(np.abs(dx - ref["dx"]).max() / np.abs(ref["dx"]).max())
    print(f"K2REF cpu step lam={lam} loss={loss_id}: {err:.3e}")
    assert rs["singular"] == 0 and err <= 1e-9
    n3 = 3 * ref["n_free_pose"]
    assert np.allclose(rs["g_pose"], ref["g"][:n3], rtol=1e-12, atol=0) and np.array_equal(rs["D"], ref["D"])


@pytest.mark.parametrize("name", k2c.NAMES)
def test_nothing_outside_the_coupling_window(name):
    """S of the reference is exactly zero outside f1 <= f2 <= frame_win_hi[f1]: the window the kernel uses to skip
    entries loses nothing."""
    p = k2c.problem(name)
    rs = kr.reduced_system(p, 1e-2, "huber", 0.1, 2.5)
    mask = kr.written_mask(_win(name))
    assert mask.shape == rs["S"].shape and np.all(rs["S"][~mask] == 0.0)
    assert np.abs(rs["S"][mask]).max() > 0 and rs["singular"] == 0


def test_rtz_split():
    rng = np.random.default_rng(3)
    x = (np.exp2(rng.uniform(-3, 15, 200000)) * rng.choice([-1.0, 1.0], 200000)).astype(np.float32)
    hi, lo = kr.split16(x)
    assert np.all(np.abs(hi) <= np.abs(x)) and np.all(np.sign(hi) == np.sign(x))
    assert np.all((lo == 0) | (np.sign(lo) == np.sign(x)))  # toward zero: the rest keeps the sign
    rel = np.abs((hi.astype(np.float64) + lo.astype(np.float64)) - x) / np.abs(x)
    assert rel.max() <= 2.0 ** -21, rel.max()
    # toward zero, not to nearest: 1 + 2^-11 + 2^-20 rounds up to 1 + 2^-10 in fp16
    y = np.float32(1 + 2.0 ** -11 + 2.0 ** -20)
    assert np.float16(y) > y and kr.rtz16(y) == np.float16(1.0)
    # subnormal results and the range's end
    s = np.float32(2.0 ** -24 * 5.75)
    assert kr.rtz16(s) == np.float16(2.0 ** -24 * 5) and kr.rtz16(np.float32(1e6)) == np.float16(65504)


@pytest.mark.parametrize("fused", [False, True])
def test_region_view_inverts_the_reduce_store(fused):
    """A region written element by element the way schur_reduce_elem / schur_reduce_vec store it (case (a) under
    ORDER_NESTED_FORCE: mirrored blocks) comes back as the reference through region_view."""
    import ptzba
    p = k2c.problem("a")
    n_pose, lam = len(p[2]), 1e-2
    win = _win("a")
    pos, _, _, n_aug, _ = ptzba.plan_export(win, 1, ptzba.ORDER_NESTED_FORCE)
    ld = ptzba.plan_summary(win, 1, ptzba.ORDER_NESTED_FORCE)["ld"]
    rs = kr.reduced_system(p, lam, "huber", 0.1, 2.5)
    S = np.zeros((ld, ld))
    vec = np.zeros((3, ld))
    for f1 in range(1, n_pose):
        for f2 in range(f1, int(win[f1]) + 1):
            for q in range(3):
                for r in range(3):
                    v = rs["S"][3 * (f1 - 1) + q, 3 * (f2 - 1) + r]
                    if f1 == f2 and q == r and fused:
                        v += lam * rs["D_pose"][3 * (f1 - 1) + q]
                    if pos[f2] >= pos[f1]:
                        S[pos[f2] + r, pos[f1] + q] = v
                    else:
                        S[pos[f1] + q, pos[f2] + r] = v
        for q in range(3):
            for k, name in enumerate(("b", "g_pose", "dU")):
                vec[k, pos[f1] + q] = rs[name][3 * (f1 - 1) + q]
            if fused:
                S[n_aug, pos[f1] + q] = rs["b"][3 * (f1 - 1) + q]
    view = kr.region_view(np.concatenate([S.reshape(-1), vec.reshape(-1)]), pos, ld, n_aug, win)
    want = kr.expected_view(rs, lam, fused)
    bu = np.kron(np.triu(np.ones((n_pose - 1, n_pose - 1))), np.ones((3, 3))) > 0  # the blocks f2 >= f1 are stored
    assert np.array_equal(view["S"][bu], want["S"][bu]) and np.array_equal(view["S"][~bu], view["S"].T[~bu])
    for k in ("b", "g_pose", "dU", "aug"):
        assert np.array_equal(view[k], want[k]), k
    assert view["mirrored"] > 0 and view["rest"] == 0.0 and np.array_equal(view["mask"], kr.written_mask(win))
    e = kr.metrics(view, dict(rs, S=want["S"]), view["mask"])
    assert max(e.values()) <= 1e-14  # (the reference's two triangles differ by their own rounding)


def test_case_structure():
    """What each case is named for, as far as the structure alone tells: the splits the builder's rule gives, ragged
    last blocks, far chunks, the empty middle list, full lists at the smallest count."""
    s = {n: kr.plan_summary(_plan(n), len(k2c.problem(n)[2])) for n in k2c.NAMES if n != "c"}
    for n, v in s.items():
        print(f"K2REF plan {n}: {v}")
    a = _plan("a")
    assert [(t["f1b"], t["chunk"], len(t["splits"])) for t in a] == [(1, 0, 10), (33, 0, 3)]
    assert [b - a_ for a_, b in a[1]["splits"]] == [32, 33, 33]  # lists of 16 k + 1 landmarks
    for n, last in (("b34", 1), ("b65", 32), ("b161", 32)):
        n_pose = len(k2c.problem(n)[2])
        assert (n_pose - 1 - 1) % 32 + 1 == last and s[n]["tiles_past_n_pose"] >= 1
    assert s["b161"]["chunk_max"] == 2 and s["b161gap"]["chunk_max"] == 2
    assert {t["chunk"] for t in _plan("b161") if t["f1b"] == 1} == {0, 1, 2}
    assert {t["chunk"] for t in _plan("b161gap") if t["f1b"] == 1} == {0, 2}  # the middle list is empty: no tile
    win = _win("b161gap")
    assert win[1] == 131  # ... although the window covers the middle chunk's frames
    assert s["crafted"]["chunk_max"] == 6 and s["tiny"]["nl_max"] <= 16 and s["tiny"]["chunk_max"] == 1
    # (c): 512 landmarks in a list first at c_landmarks()
    n = k2c.c_landmarks()
    for k, want in ((n - 1, 511), (n, 512)):
        segs_f = np.random.default_rng(40).integers(1, 32, k)
        frame = np.stack([segs_f, segs_f + 1], -1).reshape(-1)
        landmark = np.repeat(np.arange(k), 2)
        c = kr.plan_summary(kr.tile_plan(k2c.C_POSES, frame, landmark), k2c.C_POSES)
        assert c["nl_max"] == want and c["tiles"] == 1 and c["items"] == 256, c


def test_operand_ranges_fit_fp16():
    """Every operand-range case stays inside the documented range of the scheme (max |hi| < 65504) at every damping;
    the share of operands whose lo half is subnormal is recorded (it explains the model's own error; not gated)."""
    for name in k2c.E_VARIANTS:
        for lam in (0.0, 1e-2, 1e3):
            m = kr.model_mf(k2c.problem(name), lam, "huber", 0.1, 2.5, win=_win(name))
            print(f"K2REF operands {name} lam={lam}: max|hi|={m['max_hi']:.1f} subnormal_lo={m['sub_lo']:.3f}")
            assert 0 < m["max_hi"] < 65504, (name, lam, m["max_hi"])


RING_MUTATIONS = {"skip_batch", "stale_batch"}  # hand-off faults: they need a work item of more than three batches


@pytest.mark.parametrize("name", ["crafted", "a", "grid"])
def test_the_gates_bite(name):
    """Each deliberately wrong kernel (k2_ref.MUTATIONS) that the case's structure can show exceeds the fp32 gate of
    tests/test_gpu_k2_reference.py in at least one metric; printed: by how much.  The grid problem (lists of 10-13
    batches) is there for the two faults of the operand ring alone, at the settings of test_pipeline_shapes."""
    import ptzba
    p = k2c.problem(name)
    grid = name == "grid"
    lam, loss = (1e-3, ("huber", 1.0, 1.0)) if grid else (1e-2, ("huber", 0.1, 2.5))
    win = _win(name)
    pos = ptzba.plan_export(win, 1, ptzba.ORDER_NESTED_FORCE)[0]
    rs = kr.reduced_system(p, lam, *loss)
    mask = kr.written_mask(win)
    base = kr.metrics(kr.model_mf(p, lam, *loss, win=win), rs, mask)
    gates = kr.fp32_gates(base)
    assert base["S"] <= 1e-4
    applied = set()
    for mut in (sorted(RING_MUTATIONS) if grid else kr.MUTATIONS):
        m = kr.model_mf(p, lam, *loss, win=win, mutate=mut, pos=pos)
        if not m["applied"]:
            continue
        applied.add(mut)
        e = kr.metrics(m, rs, mask)
        excess = {k: e[k] / gates[k] for k in e}
        print(f"K2REF mutation {name} {mut}: " + " ".join(f"{k}={e[k]:.2e}({excess[k]:.1f}x gate)" for k in e))
        assert max(excess.values()) > 1.0, (mut, e, gates)
    plan = kr.plan_summary(_plan(name), len(p[2]))
    if grid:
        assert plan["nl_min"] > 3 * kr.SNB and applied == RING_MUTATIONS, (plan, applied)
        return
    want = {"no_lo_hi", "drop_last_of_16k1", "no_frow_backscale"}
    if plan["tiles_ge9_splits"]:
        want.add("drop_split9")
    if plan["chunk_max"] > 0:
        want.add("chunk0_only")
    f = np.arange(1, len(p[2]))
    if (((f[None, :] > f[:, None]) & (f[None, :] <= win[1:, None])) & (pos[f][None, :] < pos[f][:, None])).any():
        want.add("mirror_untransposed")
    assert applied == want, (applied, want)
    # together the two cases show every mutation but the ring's: the crafted problem has the far chunks (its all-frame
    # landmarks couple every frame to the last, so no order but the natural one exists for it: nothing is mirrored),
    # (a) the nine-split tile and, dissected once under ORDER_NESTED_FORCE, mirrored blocks
    assert want == set(kr.MUTATIONS) - RING_MUTATIONS - ({"drop_split9", "mirror_untransposed"} if name == "crafted"
                                                         else {"chunk0_only"})


def test_ring_faults_need_more_than_three_batches():
    """skip_batch and stale_batch cannot apply to the crafted problem (shown above: they are not among its applied
    mutations) or to config2, whose lists have at most 43 landmarks: only the grid problem guards the ring."""
    for name in ("crafted", "config2"):
        assert kr.plan_summary(_plan(name), len(k2c.problem(name)[2]))["nl_max"] <= 3 * kr.SNB
    p = k2c.problem("config2")
    for mut in sorted(RING_MUTATIONS):
        assert not kr.model_mf(p, 1e-3, "huber", 1.0, 1.0, win=_win("config2"), mutate=mut)["applied"]


