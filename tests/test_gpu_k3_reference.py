"""K3, the reduced-system solver (csrc/chol_kernels.hip: k_chol_prepare, k_chol_step, k_tile_inv / k_tile_inv_list and
the back-substitution kernels k_chol_backsolve_la / _ll / _blk / _pst), pinned to the dense np.longdouble reference of
tests/k3_ref.py on systems of the tests' own choosing (tests/k3_cases.py): structures that reach every task type, the
second panel pair, one- and two-level dissections and the by-value / by-pointer split of a level's task list at 240
tasks; matrices from cond 7 to 6e11, graded by 1e8 and scaled by 2^+-400.

Per case: set_problem (a real problem with the structure's coupling window), set_state, linearize, build_reduced(lam),
sync; k3_ref.region_pack(...) is copied over the exchange region (ptzba_exchange); solve_reduced, sync, read_scalars; the
factor's off-diagonal tiles and the forward-substituted row y (row n_aug) are read back from the region, Ldiag, Minv,
dpose and info through ptzba_solver_buffers.  The factor overwrites S: every solve is preceded by an injection.  dx is
never read through accept / get_state (ptz + d - ptz loses the digits these tests are about).

One line `K3REF` per case: the kernel's and the model's value of every metric (k3_ref.metrics, all in np.longdouble):
e_bw <= 2 (ld + 1) u (gate 1) and <= 10 max(model, 4 u) (gate 2) on every family; e_Minv and e_res <= 10 max(model,
floor) on every family; e_L, e_y, e_x alike on well / mid / graded / pow2_* / damped (reported on ill*).  Structure:
outside the plan's fill tiles the region is bitwise what was injected, b | g | dU are untouched, the Ldiag tiles are
lower triangular, dpose is zero on padding rows and from row n_aug on.

Measured on an MI355X (kernel | model, the largest over the back-solve forms): DESIGN section 4.3."""
import numpy as np
import pytest

import k3_cases as kc
import k3_ref as k3

pytestmark = pytest.mark.gpu

FP64, FP32 = 0, 1
# (configuration, back-solve form or None = the library's choice)
RUNS = [("one_tile", None), ("chain", None), ("chain_d2", None)] + \
       [(c, f) for c in ("nd2_small", "nd2") for f in kc.FORMS] + \
       [("nd2_nd1", None), ("nd2_d2", None), ("nd2_b0", None), ("wide", None)]
DEFAULT_FORM = {"one_tile": "la", "chain": "la", "chain_d2": "la", "nd2_small": "la", "nd2": "la", "nd2_nd1": "la",
                "nd2_d2": "la", "nd2_b0": "la", "wide": "pst"}  # n_aug >= 512: blocked, persistent


class _DevInts:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 3,
                                         "strides": None}


class Session:
    """One FP64 (or FP32) handle on a configuration's problem, with torch views of the region and the solver's buffers."""

    def __init__(self, config, form, monkeypatch, precision=FP64):
        import torch
        import bench
        import ptzba
        self.torch = torch
        self.config, self.form = config, form or DEFAULT_FORM[config]
        self.pl = pl = kc.plan(config, monkeypatch)  # (sets the plan's knobs)
        env, want_bs = kc.FORMS[form] if form else ({}, kc.FORMS[DEFAULT_FORM[config]][1])
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        (u, v, ptz0, rays0, frame, landmark, xy, weight), _ = kc.problem(kc.CONFIGS[config][0])
        self.h = h = ptzba.BAHandle(0)
        try:
            h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, precision=precision,
                          ordering=kc.ordering(config))
            si = h.solver_info()
            kc.check_shape(config, pl, si)  # the shape the case is named for really runs
            assert si["backsolve"] == want_bs, (config, form, si)
            h.set_state(ptz0, rays0)
            h.linearize()
            h.build_reduced(0.0)
            h.sync()
            sp, n, _ = h.exchange()
            assert n == pl["ld"] * (pl["ld"] + 3)
            self.region = torch.as_tensor(bench._DevArray(sp, n), device="cuda:0")
            b = h.solver_buffers()
            assert b["Ldiag"][1] == b["Minv"][1] == pl["ld"] * 32 and b["dpose"][1] == pl["ld"] and b["info"][1] == 1
            self.bufs = {k: torch.as_tensor(bench._DevArray(*b[k]), device="cuda:0") for k in ("Ldiag", "Minv", "dpose")}
            self.info = torch.as_tensor(_DevInts(*b["info"]), device="cuda:0")
        except BaseException:
            h.close()
            raise
        self.fp = k3.frame_rows(pl["pos"])

    def close(self):
        self.h.close()

    def solve(self, S, b, dU, g, lam=0.0):
        """build_reduced(lam), inject, solve_reduced; dict(injected, region, Ldiag, Minv [T, 32, 32], dpose, info, flag)."""
        pl, h, torch = self.pl, self.h, self.torch
        h.build_reduced(lam)
        h.sync()
        inj = k3.region_pack(S, b, dU, pl["pos"], pl["ld"], pl["n_aug"], pl["win"], g=g)
        self.region.copy_(torch.from_numpy(inj))
        torch.cuda.synchronize()
        h.solve_reduced()
        h.sync()
        flag = h.read_scalars()[5]
        torch.cuda.synchronize()
        T = pl["ld"] // 32
        return dict(injected=inj, region=self.region.cpu().numpy().copy(),
                    Ldiag=self.bufs["Ldiag"].cpu().numpy().reshape(T, 32, 32).copy(),
                    Minv=self.bufs["Minv"].cpu().numpy().reshape(T, 32, 32).copy(),
                    dpose=self.bufs["dpose"].cpu().numpy().copy(), info=int(self.info.cpu().numpy()[0]), flag=flag)


def _reference(config, family, A_key, make_A, pl):
    """The augmented system and its np.longdouble reference: computed once per module, never modified."""
    def make():
        A = make_A()
        return A, k3.reference(A, pl["n_aug"])
    return kc._memo(("gpu_ref", config, family, A_key), make)


def _model(config, family, A_key, form, A, ref, pl):
    def make():
        mo = k3.model(A, pl["tasks"], pl["level_off"], pl["n_aug"], kc.MODEL_FORM[form])
        return mo, k3.metrics(A, pl["n_aug"], k3.frame_rows(pl["pos"]), ref, mo["L"], mo["Minv"], mo["x"])
    return kc._memo(("gpu_model", config, family, A_key, kc.MODEL_FORM[form]), make)


def _verify(ses, family, out, D, tag="", A_key=0):
    """The K3REF line of one solve, then the flag, the structure and the gates.  D: the damping scale the reference uses
    (max(D_prev, dU, 1e-12)).  Returns (metrics, assembled factor)."""
    pl, config = ses.pl, ses.config
    m = kc.matrix(kc.CONFIGS[config][0], family)
    ld, n = pl["ld"], pl["n_aug"]
    A, ref = _reference(config, family, A_key, lambda: k3.augmented(m["S"], m["b"], pl["pos"], ld, n, m["lam"], D), pl)
    mo, em = _model(config, family, A_key, ses.form, A, ref, pl)
    Sr = out["region"][:ld * ld].reshape(ld, ld)
    L = k3.assemble(Sr, out["Ldiag"], ld)
    x = out["dpose"][:n]
    e = k3.metrics(A, n, ses.fp, ref, L, out["Minv"], x)
    g = k3.gates(em, ld)
    print(k3.line(f"config={config} form={ses.form} matrix={family}{tag}", e, em) +
          f" gate1={g['bw1']:.2e} flag={out['flag']:g}")
    assert out["flag"] == 0 and out["info"] == 0, (out["flag"], out["info"])
    # structure
    inj = out["injected"]
    fill = np.kron(pl["fill"], np.ones((32, 32), bool))
    Si = inj[:ld * ld].reshape(ld, ld)
    assert np.array_equal(Sr[~fill], Si[~fill])           # outside the plan's fill tiles: bitwise what was injected
    assert not Si[np.tril(~fill)].any()                   # ... which is zero in the lower triangle
    assert np.array_equal(out["region"][ld * ld:], inj[ld * ld:])  # b | g | dU untouched by the solve
    assert not np.triu(out["Ldiag"], 1).any()             # the factor's diagonal tiles are lower triangular
    pad = np.setdiff1d(np.arange(n), ses.fp)
    assert not out["dpose"][pad].any() and not out["dpose"][n:].any()  # as the model: zero on padding rows, and below
    assert not mo["x"][pad].any()
    assert np.isfinite(L[:n + 1, :n]).all() and np.isfinite(x).all()
    k3.check(e, g, family in kc.FORWARD_GATED)
    return e, L


@pytest.mark.parametrize("family", [f for f in kc.FAMILIES if f != "damped"])
@pytest.mark.parametrize("config,form", RUNS)
def test_factor_and_solve_against_the_reference(gpu_available, config, form, family, monkeypatch):
    """Every structure, plan knob and back-solve form on every matrix family at lambda 0.  pow2_*: also reports whether
    L is bitwise 2^+-200 times mid's and x bitwise mid's (a report, not a gate)."""
    ses = Session(config, form, monkeypatch)
    try:
        m = kc.matrix(kc.CONFIGS[config][0], family)
        D = np.maximum(m["dU"], 1e-12)
        out = ses.solve(m["S"], m["b"], m["dU"], m["g"])
        _, L = _verify(ses, family, out, D)
        if family in ("pow2_up", "pow2_down"):
            mid = kc.matrix(kc.CONFIGS[config][0], "mid")
            o2 = ses.solve(mid["S"], mid["b"], mid["dU"], mid["g"])
            ld, n = ses.pl["ld"], ses.pl["n_aug"]
            L2 = k3.assemble(o2["region"][:ld * ld].reshape(ld, ld), o2["Ldiag"], ld)
            fp = ses.fp
            s = 200 if family == "pow2_up" else -200
            print(f"K3REF config={config} form={ses.form} matrix={family} "
                  f"L_bitwise_scaled={np.array_equal(L[np.ix_(fp, fp)], np.ldexp(L2[np.ix_(fp, fp)], s))} "
                  f"x_bitwise_same={np.array_equal(out['dpose'], o2['dpose'])}")
    finally:
        ses.close()


@pytest.mark.parametrize("config,form", [("one_tile", None), ("nd2_small", "la"), ("nd2_small", "pst"), ("wide", None)])
def test_damping_memory(gpu_available, config, form, monkeypatch):
    """k_chol_prepare's damping: lambda = 1e-3 with a chosen dU, then a second solve on the same handle with dU lowered
    everywhere -- the reference of both is S + lam diag(max(D_prev, dU, 1e-12)) with the FIRST solve's dU
    (tests/test_k3_ref.py shows that forgetting D_prev moves the factor by 1e6 gates)."""
    ses = Session(config, form, monkeypatch)
    try:
        m = kc.matrix(kc.CONFIGS[config][0], "damped")
        D = np.maximum(m["dU"], 1e-12)
        out = ses.solve(m["S"], m["b"], m["dU"], m["g"], m["lam"])
        _verify(ses, "damped", out, D, " solve=1")
        out = ses.solve(m["S"], m["b"], m["dU2"], m["g"], m["lam"])
        _verify(ses, "damped", out, D, " solve=2(dU lowered)")
    finally:
        ses.close()


FLAG_RUNS = [(c, f) for c in ("nd2_small", "one_tile") for f in ("la", "blk", "pst")]


def _indefinite(ses, row=None, nan=False):
    """`well` with -1 on the diagonal at system row `row`, or with one NaN off the diagonal."""
    m = kc.matrix(kc.CONFIGS[ses.config][0], "well")
    S = m["S"].copy()
    if nan:
        k = len(S) // 2
        S[k, k + 1] = S[k + 1, k] = np.nan
    else:
        k = int(np.flatnonzero(ses.fp == row)[0])
        S[k, k] = -1.0
    return ses.solve(S, m["b"], m["dU"], m["g"])


@pytest.mark.parametrize("config,form", FLAG_RUNS)
def test_flag_is_raised_and_cleared(gpu_available, config, form, monkeypatch):
    """An indefinite input -- diagonal -1 at the first row, at both ends of a pivot block (rows 4 s and 4 s + 3 of a
    tile), at the last pose row before padding, in a separator tile and in the last real tile -- or a NaN raises the
    status (read_scalars()[5] != 0) and the call returns; nothing is asserted about the numbers (the clamp to 1e-300 may
    overflow).  The next solve of `well` on the same handle reports 0 and meets every gate: the flag's reset in
    k_chol_prepare, and Ldiag / Minv / the blocked form's r / the persistent form's counters carry nothing over."""
    ses = Session(config, form, monkeypatch)
    try:
        m = kc.matrix(kc.CONFIGS[config][0], "well")
        D = np.maximum(m["dU"], 1e-12)
        rows = kc.indefinite_rows(ses.pl)
        for name, row in rows.items():
            out = _indefinite(ses, row)
            print(f"K3REF config={config} form={ses.form} indefinite at {name} (row {row}): flag={out['flag']:g}")
            assert out["flag"] != 0 and out["info"] != 0, (name, row)
            if name in ("first", "last_tile"):  # cleared after the first and after the last of them
                _verify(ses, "well", ses.solve(m["S"], m["b"], m["dU"], m["g"]), D, f" after indefinite {name}")
        out = _indefinite(ses, nan=True)
        assert out["flag"] != 0 and out["info"] != 0
        _verify(ses, "well", ses.solve(m["S"], m["b"], m["dU"], m["g"]), D, " after NaN")
    finally:
        ses.close()


@pytest.mark.parametrize("config,form", FLAG_RUNS + [("wide", None)])
def test_repeat_is_bitwise(gpu_available, config, form, monkeypatch):
    """Two identical inject + solve rounds on one handle: bitwise the same region, Ldiag, Minv and dpose (the epoch
    counters of k_chol_backsolve_pst; no accumulation into state of the first round), with another system in between."""
    ses = Session(config, form, monkeypatch)
    try:
        st = kc.CONFIGS[config][0]
        m, other = kc.matrix(st, "mid"), kc.matrix(st, "graded")
        a = ses.solve(m["S"], m["b"], m["dU"], m["g"])
        b = ses.solve(m["S"], m["b"], m["dU"], m["g"])
        ses.solve(other["S"], other["b"], other["dU"], other["g"])
        c = ses.solve(m["S"], m["b"], m["dU"], m["g"])
        for o in (b, c):
            assert o["flag"] == 0
            for k in ("region", "Ldiag", "Minv", "dpose"):
                assert np.array_equal(a[k], o[k]), k
    finally:
        ses.close()


def test_fp32_handle_runs_the_same_k3(gpu_available, monkeypatch):
    """K3 is fp64 whatever the handle's precision: an FP32 handle given the same injected system leaves bitwise the
    FP64 handle's factor and dpose."""
    res = []
    for precision in (FP64, FP32):
        ses = Session("nd2_small", None, monkeypatch, precision)
        try:
            m = kc.matrix("nd2_small", "well")
            res.append(ses.solve(m["S"], m["b"], m["dU"], m["g"]))
        finally:
            ses.close()
    ld, n = ses.pl["ld"], ses.pl["n_aug"]
    assert res[0]["flag"] == 0 and res[1]["flag"] == 0
    tiles = np.unique(ses.fp // 32)  # (a tile column without pose rows is never inverted: its Minv tile is never written)
    assert np.array_equal(res[0]["Ldiag"], res[1]["Ldiag"]) and np.array_equal(res[0]["dpose"], res[1]["dpose"])
    assert np.array_equal(res[0]["Minv"][tiles], res[1]["Minv"][tiles])
    L = [k3.assemble(r["region"][:ld * ld].reshape(ld, ld), r["Ldiag"], ld)[:n + 1] for r in res]
    assert np.array_equal(L[0], L[1])
