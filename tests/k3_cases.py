"""The structures and matrices K3 (the tile Cholesky and its back-solves: csrc/chol_kernels.hip) is handed in
tests/test_k3_ref.py (CPU) and tests/test_gpu_k3_reference.py (GPU): systems of the tests' own choosing, written over the
exchange region between ptzba_build_reduced and ptzba_solve_reduced, not what K2 builds from friendly data.

Structures: a coupling window band(n, w)[f] = min(f + w, n - 1), turned into a real problem (three short landmarks per
frame, the first reaching win[f]: test_plan_replay._tree_problem; poses, rays and pixels from k2_cases.build) so that
set_problem accepts it.  A configuration = structure + ordering + the A/B knobs of the plan:

  one_tile   band(12, 3)                 n_aug 33: one real tile and the augmented row's, 2 levels
  chain      band(40, 6), natural        one chain of 4 levels, type-1 trailing; chain_d2: PTZBA_CHOL_DELAY=2 (second pair)
  nd2_small  band(60, 8), nested         n_aug 224, nd_depth 2, 4 chains, task types 0 / 1 / 2 / 3, second pair
  nd2        band(120, 12), nested       n_aug 448, 7 levels, 14 block tasks; nd2_nd1: PTZBA_ND_DEPTH=1 (one-level order),
                                         nd2_d2: PTZBA_CHOL_DELAY=2 (the default period here: the same
                                         plan, under the knob), nd2_b0: PTZBA_CHOL_BLOCKS=0 (per-tile trailing)
  wide       band(300, 140), nested      PTZBA_CHOL_BLOCKS=0: n_aug 928, 254 tasks in one level -- the first CHOL_KT = 240
                                         travel by value in the kernel arguments, the rest through the pointer

Matrices (frame order, support inside k2_ref.written_mask(win)): per frame f one dense "landmark" G G^T, G [rows of
frames f..win[f], 2], scaled to unit diagonal, then 1 + delta on the diagonal; b random.

  well / mid / ill8 / ill11   delta = 1 / 1e-4 / 1e-8 / 1e-11
  graded      well scaled by D = diag(1e4, 1e4, 1e-4 per frame: pan / tilt against f), b alike
  pow2_up / pow2_down   mid times 2^+-400, b alike (every metric is scale-invariant)
  damped      well with lam = 1e-3 and a chosen dU (tests/test_gpu_k3_reference.py lowers it for a second solve)
"""
import numpy as np

import k2_cases as k2c
import k2_ref as kr

NB = 32
CHOL_KT = 240       # csrc/ptzba_kernels.h: a level's tasks that travel by value
AUG_DIAG = 1e300    # csrc/chol_kernels.hip
KNOBS = ("PTZBA_ND_DEPTH", "PTZBA_CHOL_DELAY", "PTZBA_CHOL_BLOCKS", "PTZBA_BACKSOLVE", "PTZBA_BS_PERSIST")


def band(n, w):
    return np.minimum(np.arange(n) + w, n - 1).astype(np.int32)


STRUCTS = {"one_tile": (12, 3), "chain": (40, 6), "nd2_small": (60, 8), "nd2": (120, 12), "wide": (300, 140)}

# configuration -> (structure, natural order?, plan knobs, the shape it is named for)
# shape keys: n_aug, nd_depth, levels, types (the task types present), second_pair, blocks (type-3 tasks), chains,
# max_level_tasks_gt (a lower bound); read from ptzba.plan_summary / plan_export
CONFIGS = {
    "one_tile": ("one_tile", False, {},
                 dict(n_aug=33, levels=2, nd_depth=0, chains=1, types={0, 2}, second_pair=False, blocks=0)),
    "chain": ("chain", True, {},
              dict(n_aug=117, levels=4, nd_depth=0, chains=1, types={0, 1, 2}, second_pair=False, blocks=0)),
    "chain_d2": ("chain", True, {"PTZBA_CHOL_DELAY": "2"},
                 dict(n_aug=117, levels=4, nd_depth=0, chains=1, types={0, 1, 2}, second_pair=True, blocks=0)),
    "nd2_small": ("nd2_small", False, {},
                  dict(n_aug=224, levels=4, nd_depth=2, chains=4, types={0, 1, 2, 3}, second_pair=True, blocks=1)),
    "nd2": ("nd2", False, {},
            dict(n_aug=448, levels=7, nd_depth=2, chains=4, types={0, 1, 2, 3}, second_pair=True, blocks=14)),
    "nd2_nd1": ("nd2", False, {"PTZBA_ND_DEPTH": "1"},
                dict(n_aug=416, levels=9, nd_depth=1, chains=2, types={0, 1, 2, 3}, second_pair=True, blocks=6)),
    "nd2_d2": ("nd2", False, {"PTZBA_CHOL_DELAY": "2"},
               dict(n_aug=448, levels=7, nd_depth=2, chains=4, types={0, 1, 2, 3}, second_pair=True, blocks=14)),
    "nd2_b0": ("nd2", False, {"PTZBA_CHOL_BLOCKS": "0"},
               dict(n_aug=448, levels=7, nd_depth=2, chains=4, types={0, 1, 2}, second_pair=True, blocks=0)),
    "wide": ("wide", False, {"PTZBA_CHOL_BLOCKS": "0"},
             dict(n_aug=928, levels=23, nd_depth=1, chains=2, types={0, 1, 2}, second_pair=False, blocks=0,
                  max_level_tasks_gt=CHOL_KT)),
}

# back-solve forms: knobs and what solver_info()["backsolve"] then says
FORMS = {
    "la": ({"PTZBA_BACKSOLVE": "la"}, "lookahead"),
    "ll": ({"PTZBA_BACKSOLVE": "ll"}, "left-looking"),
    "blk": ({"PTZBA_BACKSOLVE": "blk", "PTZBA_BS_PERSIST": "0"}, "blocked"),
    "pst": ({"PTZBA_BACKSOLVE": "blk"}, "blocked"),
}
MODEL_FORM = {"la": "right", "ll": "left", "blk": "block", "pst": "block"}

DELTA = {"well": 1.0, "mid": 1e-4, "ill8": 1e-8, "ill11": 1e-11}
FAMILIES = ("well", "mid", "ill8", "ill11", "graded", "pow2_up", "pow2_down", "damped")
FORWARD_GATED = ("well", "mid", "graded", "pow2_up", "pow2_down", "damped")
DAMPED_LAM = 1e-3

_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def set_env(monkeypatch, env):
    """Exactly the knobs of `env`: every other A/B knob of the plan and the back-solve unset."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _tree_problem(win0, seed):
    """As test_plan_replay._tree_problem: per frame f three landmarks on f plus 1-3 frames of (f, win[f]], the first of
    them reaching win[f] itself, so the records' own window is the given one."""
    rng = np.random.default_rng(seed)
    fr, lm = [], []
    n_lm = 0
    for f in range(len(win0)):
        hi = int(win0[f])
        for q in range(3):
            F = {f}
            if hi > f:
                if q == 0:
                    F.add(hi)
                F |= {int(x) for x in rng.integers(f + 1, hi + 1, size=int(rng.integers(1, 4)))}
            fr += sorted(F)
            lm += [n_lm] * len(F)
            n_lm += 1
    return np.array(fr, np.int32), np.array(lm, np.int32), n_lm


def problem(struct):
    """The structure's problem tuple (k1_cases form) and its coupling window, built once."""
    def make():
        import ptzba
        n, w = STRUCTS[struct]
        win0 = band(n, w)
        frame, landmark, _ = _tree_problem(win0, seed=3)
        segs = [(int(l), int(f), 1) for f, l in zip(frame, landmark)]
        p = k2c.build(n, segs, 70 + n)
        win = ptzba.frame_coupling_window(n, p[4], p[5])
        assert np.array_equal(win[1:], win0[1:])  # the records' own window is the band (frame 0 is fixed)
        return p, win
    return _memo(("problem", struct), make)


def ordering(config):
    import ptzba
    return ptzba.ORDER_NATURAL if CONFIGS[config][1] else ptzba.ORDER_NESTED


def plan(config, monkeypatch):
    """The configuration's plan (host only; the environment is set to the configuration's knobs and left so): dict(win,
    pos, tasks, level_off, n_aug, ld, second_pair, summary, fill = bool [T, T]: the tiles the factorisation may write,
    diagonal tiles and the augmented row's included)."""
    import ptzba
    struct, _, env, _ = CONFIGS[config]
    set_env(monkeypatch, env)

    def make():
        _, win = problem(struct)
        o = ordering(config)
        pos, tasks, off, n_aug, second = ptzba.plan_export(win, 1, o)
        ld = (n_aug + 1 + NB - 1) // NB * NB
        T = ld // NB
        import chol_plan_exec as cpe
        fill = np.eye(T, dtype=bool)
        types = set()
        blocks = 0
        for t in tasks:
            typ, i, j, ups, tmask = cpe.decode(t)
            types.add(typ)
            if typ == 0 and i != j:
                fill[i, j] = True
            elif typ == 1:
                fill[i, j] = True
            elif typ == 3:
                blocks += 1
                for m in range(4):
                    if (tmask >> m) & 1:
                        fill[i + (m >> 1), j + (m & 1)] = True
        return dict(win=win, pos=pos, tasks=tasks, level_off=off, n_aug=n_aug, ld=ld, second_pair=second, fill=fill,
                    types=types, blocks=blocks, summary=ptzba.plan_summary(win, 1, o))
    return _memo(("plan", config), make)


def check_shape(config, pl, solver_info=None):
    """The configuration has the shape it is named for (plan_export / plan_summary, and the handle's solver_info())."""
    want = CONFIGS[config][3]
    s = pl["summary"]
    assert s["n_aug"] == pl["n_aug"] and s["ld"] == pl["ld"] and s["levels"] == len(pl["level_off"]) - 1, (config, s)
    got = dict(n_aug=pl["n_aug"], nd_depth=s["nd_depth"], levels=s["levels"], chains=s["chains"],
               second_pair=pl["second_pair"], blocks=pl["blocks"])
    for k, v in want.items():
        if k == "types":
            assert v == pl["types"], (config, pl["types"])
        elif k == "max_level_tasks_gt":
            assert s["max_level_tasks"] > v, (config, s)
            assert int(np.diff(pl["level_off"]).max()) == s["max_level_tasks"]
        else:
            assert got[k] == v, (config, k, got)
    assert (s["panel_pairs"] == 2) == pl["second_pair"]
    if solver_info is not None:
        assert solver_info["n_aug"] == pl["n_aug"] and solver_info["ld"] == pl["ld"], (config, solver_info)
        assert solver_info["levels"] == s["levels"] and solver_info["nd_depth"] == s["nd_depth"], (config, solver_info)
        assert (solver_info["ordering"] == "natural") == (s["nd_depth"] == 0)


def frame_rows(pos, n_fixed=1):
    """System row of every frame-order index (3 per free frame)."""
    pos = np.asarray(pos, np.int64)
    return np.repeat(pos[n_fixed:], 3) + np.tile(np.arange(3), len(pos) - n_fixed)


def base_matrix(struct, delta):
    """(S, b) in frame order: sum over frames of G G^T scaled to unit diagonal, 1 + delta on the diagonal, b random."""
    def make():
        _, win = problem(struct)
        n = len(win)
        n3 = 3 * (n - 1)
        rng = np.random.default_rng(1000 + n)
        S = np.zeros((n3, n3))
        for f in range(1, n):
            rows = np.arange(3 * (f - 1), 3 * int(win[f]))
            G = rng.standard_normal((len(rows), 2))
            S[np.ix_(rows, rows)] += G @ G.T
        d = 1.0 / np.sqrt(np.diag(S))
        S = S * d[:, None] * d[None, :]
        S = 0.5 * (S + S.T)
        b = rng.standard_normal(n3)
        return S, b
    S, b = _memo(("base", struct), make)
    S = S.copy()
    S[np.diag_indices_from(S)] = 1.0 + delta
    return S, b.copy()


def matrix(struct, family):
    """dict(S, b, g, dU (frame order), lam, dU2 (damped: the lowered dU of the second solve)) -- never modified."""
    def make():
        n3 = 3 * (STRUCTS[struct][0] - 1)
        rng = np.random.default_rng(7)
        g = rng.standard_normal(n3)          # rides along untouched
        dU = np.ones(n3)
        lam, dU2 = 0.0, None
        if family in DELTA:
            S, b = base_matrix(struct, DELTA[family])
        elif family == "graded":
            S, b = base_matrix(struct, 1.0)
            D = np.tile([1e4, 1e4, 1e-4], n3 // 3)
            S, b = S * np.outer(D, D), b * D  # (the outer product first: S stays exactly symmetric)
        elif family in ("pow2_up", "pow2_down"):
            S, b = base_matrix(struct, 1e-4)
            s = 2.0 ** (400 if family == "pow2_up" else -400)
            S, b = S * s, b * s  # exact
        elif family == "damped":
            S, b = base_matrix(struct, 1.0)
            lam = DAMPED_LAM
            dU = rng.uniform(0.5, 50.0, n3)
            dU2 = dU * rng.uniform(0.05, 0.9, n3)  # lower everywhere: the remembered scale must win
        else:
            raise KeyError(family)
        assert np.all(S[~kr.written_mask(problem(struct)[1])] == 0.0)
        return dict(S=S, b=b, g=g, dU=dU, lam=lam, dU2=dU2)
    return _memo(("matrix", struct, family), make)


def indefinite_rows(pl):
    """Where the flag tests put a diagonal of -1 (system rows of pose entries): the first row, a pivot-block boundary
    (rows 4 s and 4 s + 3 inside a tile), the last pose row before padding, a row of a separator tile, the last real
    tile.  {name: system row}."""
    pos, n_aug = pl["pos"], pl["n_aug"]
    fr = np.sort(frame_rows(pos))
    is_pose = np.zeros(pl["ld"], bool)
    is_pose[fr] = True
    out = {"first": int(fr[0])}
    for r in fr:  # a tile-local row 4 s (s >= 1) and the 4 s + 3 of the same block
        if r % NB >= 4 and r % 4 == 0 and is_pose[r + 3]:
            out["block_lo"], out["block_hi"] = int(r), int(r + 3)
            break
    pads = np.flatnonzero(~is_pose[:n_aug])
    out["before_pad"] = int(pads[0] - 1) if len(pads) and pads[0] > 0 and is_pose[pads[0] - 1] else int(fr[-1])
    # the separator is ordered last: its tiles are the last full tiles below the augmented row's
    last_tile = (n_aug - 1) // NB
    out["separator"] = int(fr[fr // NB == max(last_tile - 1, 0)][0])
    out["last_tile"] = int(fr[fr // NB == last_tile][-1])
    return out
