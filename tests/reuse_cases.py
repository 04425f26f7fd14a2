"""Problems and scripts of the handle-reuse tests (test infrastructure, no GPU needed to import; used by
tests/test_reuse_cases.py on the CPU and tests/test_gpu_handle_reuse.py and tests/test_gpu_k1_merge.py on the GPU).

The reuse contract: after set_problem(B) succeeds on a handle that held any problem A, everything
the handle computes is bit for bit what a new handle computes for B.  The problems are tests/k1_cases.py's, so each
has the dense fp64 reference of that module:

  P64, P140, P200   k1_cases.craft(n_pose=64 / 140 / 200)           P150   k1_cases.craft(n_pose=150, seed=8)
  ...w               the same with weighted=True
  M140 / O140        P140 put into pair form (pair_form): runs of repeated records that K1 reads merged ("aaba": three
                     runs in the longer segments) / as one record per segment ("one_run")
  B140               P140 without its every-frame landmarks: a banded coupling window, which takes the nested order

P200 has >= 512 system rows (the blocked persistent back-substitution), P64 and P140 take the lookahead form; P140 ->
P150 grows inside DBuf::alloc's quarter of slack, P64 -> P200 beyond it, and P200 -> P64 shrinks the dense system
buffer below a quarter of its allocation (test_reuse_cases.py restates the rule and checks every regime).

Case: a problem with the options of set_problem and whether the four optional features (pose priors, ray priors, the
marginal factor, the displacement) are set.  apply(h, case) puts it on a handle, dirty(h, case) leaves as much behind
under it as the API allows, observe(h, case) returns everything the comparison reads."""
import dataclasses
import types

import numpy as np

import k1_cases as kc

N_POSE = 140  # pair_form's problems: > K1_SEGW frames, the every-frame landmarks are walked in two windows
DISPLACEMENT = np.array([0.01, -0.02, 0.03, 1e-5, -2e-5, 3e-5])  # disp_ref.LAMBDA: the golden camera's
_cache = {}


def segments(frame, landmark):
    """Sorted order, each sorted record's position in its segment and its segment's first sorted record."""
    n = len(frame)
    o = np.lexsort((np.arange(n), frame, landmark))
    key = landmark[o].astype(np.int64) * N_POSE * 4 + frame[o]
    start = np.concatenate([[True], key[1:] != key[:-1]])
    first = np.maximum.accumulate(np.where(start, np.arange(n), 0))
    size = np.diff(np.flatnonzero(np.concatenate([start, [True]])))[np.cumsum(start) - 1]  # records of its segment
    return o, np.arange(n) - first, first, start, size


def pair_form(shape, extra=0):
    """A k1_cases problem (N_POSE frames, ~2,400 records) put into pair form -- every record of a segment at the
    segment's first keypoint: "one_run" every segment one run; "aaba" the third record of the segments of four and more
    keeps its own observation (A A B A ...); "w_const" one user weight per segment; "w_split" weights that split the
    runs of the longer segments; "below_half" / "above_half" runs == floor(R / 2) / one more."""
    k = ("pair", shape, extra)
    if k in _cache:
        return _cache[k]
    u, v, ptz0, rays0, frame, landmark, xy, _ = kc.craft(n_pose=N_POSE, extra=extra)
    o, pos, first, start, size = segments(frame, landmark)
    rng = np.random.default_rng(11)
    xs = xy[o]
    one = xs[first]  # every record of a segment at the segment's first keypoint
    weight = None
    if shape in ("one_run", "w_const", "w_split", "below_half", "above_half"):
        xs = one.copy()
    elif shape == "aaba":  # segments of four records and more: the third keeps its own observation, A A B A A ...
        xs = np.where(((pos == 2) & (size >= 4))[:, None], xs, one)
    else:
        raise ValueError(shape)
    if shape == "w_const":  # one user weight per segment: the runs stay, their weights are multiplicity x weight
        weight = np.empty(len(frame))
        weight[o] = rng.choice([1.0, 2.0, 3.0, 5.0], len(frame))[first]
    if shape == "w_split":  # weights that differ inside a segment (of four records and more) split its runs
        weight = np.empty(len(frame))
        weight[o] = np.where(((pos == 2) | (pos == 3)) & (size >= 4), 2.0, 1.0)
    if shape in ("below_half", "above_half"):
        # runs = floor(R / 2) (merged) or one more (not merged): the last record of as many multi-record segments as
        # that takes moves by an eighth of a pixel
        n, runs = len(frame), int(start.sum())
        want = n // 2 + (1 if shape == "above_half" else 0)
        last = np.flatnonzero(np.concatenate([start[1:], [True]]) & (pos >= 1))
        assert want - runs <= len(last), (n, runs, len(last))
        xs = xs.copy()
        xs[last[:want - runs], 0] += 0.125
    out = xy.copy()
    out[o] = xs
    _cache[k] = (u, v, ptz0, rays0, frame, landmark, out, weight)
    return _cache[k]


_CRAFT = {"P64": dict(n_pose=64), "P140": dict(n_pose=140), "P150": dict(n_pose=150, seed=8), "P200": dict(n_pose=200)}
NAMES = tuple(_CRAFT) + tuple(k + "w" for k in _CRAFT) + ("M140", "O140", "B140")


def _banded(p):
    """The landmarks of p seen by at most 12 frames, renumbered: a coupling window of 11 frames, which the nested
    dissection order splits (the every-frame landmarks of k1_cases couple all frames and leave only the natural order)."""
    u, v, ptz0, rays0, frame, landmark, xy, _ = p
    seen = np.zeros((len(rays0), len(ptz0)), bool)
    seen[landmark, frame] = True
    keep = np.flatnonzero(seen.sum(1) <= 12)
    new = np.full(len(rays0), -1, np.int64)
    new[keep] = np.arange(len(keep))
    k = new[landmark] >= 0
    return u, v, ptz0, rays0[keep], frame[k], new[landmark[k]].astype(np.int32), xy[k], None


def problem(name):
    """The problem tuple (u, v, ptz0, rays0, frame, landmark, xy, weight) of a name of NAMES, built once."""
    if name not in _cache:
        if name == "M140":
            _cache[name] = pair_form("aaba")
        elif name == "O140":
            _cache[name] = pair_form("one_run")
        elif name == "B140":
            _cache[name] = _banded(problem("P140"))
        else:
            _cache[name] = kc.craft(weighted=name.endswith("w"), **_CRAFT[name.rstrip("w")])
    return _cache[name]


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    precision: int = 0          # ptzba.FP64 / FP32
    loss: str = "linear"        # scipy's name
    f_scale: float = 1.0
    n_fixed: int = 1
    ordering: int = 1           # ptzba.ORDER_NESTED, set_problem's default
    features: bool = False      # pose priors, ray priors, the marginal factor and the displacement
    front: int = -1             # set_setup_front before set_problem: -1 the library's default, 0 the device front

    @property
    def p(self):
        return problem(self.name)

    @property
    def has_reference(self):
        """k1_cases.reference states this case's first step: linear or Huber loss, frame 0 alone fixed, no feature."""
        return self.loss in ("linear", "huber") and self.n_fixed == 1 and not self.features


# ------------------------------------------------------------------------------------------------ the features
def pose_factors(p):
    """A unary factor and a two-frame factor with cross terms, on free frames for n_fixed <= 2."""
    ptz0 = p[2]
    B = np.random.default_rng(3).normal(0, 1.0, (6, 6))
    info2 = B @ B.T * np.outer(np.tile([40.0, 40.0, 0.02], 2), np.tile([40.0, 40.0, 0.02], 2))
    return [([3], ptz0[3] + [0.01, -0.01, 2.0], np.diag([900.0, 900.0, 0.01])),
            ([5, 6], (ptz0[[5, 6]] + [0.005, 0.005, -1.0]).reshape(-1), info2)]


def ray_priors(p):
    """Three priors, two of them on one landmark."""
    rays0 = p[3]
    L = np.array([[400.0, 30.0], [30.0, 250.0]])
    return [(0, rays0[0] + [0.003, -0.002], L), (5, rays0[5], 2.0 * L), (5, rays0[5] - [0.001, 0.001], np.diag([90.0, 0.0]))]


def marginal(p):
    """A dense factor over frames 2 and 4, linearised off the initial state."""
    import ptzba
    ptz0 = p[2]
    B = np.random.default_rng(4).normal(0, 1.0, (6, 4))
    s = np.tile([30.0, 30.0, 0.015], 2)
    info = (B @ B.T) * np.outer(s, s)
    return ptzba.Marginal([2, 4], ptz0[[2, 4]] + [0.004, -0.003, 1.5], info, info @ np.full(6, 1e-3), 0.25)


def window(c):
    """set_problem's frame_win_hi of a case: the records' coupling window raised for the features' frame pairs."""
    import ptzba
    if not c.features:
        return None
    p = c.p
    return ptzba.prior_window(len(p[2]), p[4], p[5], pose_factors(p) + [marginal(p)])


def apply(h, c):
    """set_problem(c) on the handle, then its features and the initial state."""
    import ptzba
    u, v, ptz0, rays0, frame, landmark, xy, weight = c.p
    h.set_setup_front(c.front)
    h.set_problem(len(ptz0), len(rays0), frame, landmark, xy, u, v, weight=weight, precision=c.precision,
                  loss=c.loss, f_scale=c.f_scale, n_fixed=c.n_fixed, ordering=c.ordering, frame_win_hi=window(c))
    if c.features:
        h.set_pose_priors(pose_factors(c.p))
        h.set_ray_priors(ray_priors(c.p))
        h.set_displacement(DISPLACEMENT)
    h.set_state(ptz0, rays0)
    if c.features:
        h.set_marginal_prior(marginal(c.p))
    assert isinstance(h, ptzba.BAHandle)


# ------------------------------------------------------------------------------------------------ the scripts
_TIGHT = dict(ftol=1e-15, xtol=1e-15)  # three iterations run to the end: no early stop


def joint_selection(c):
    n_pose, n_lm = len(c.p[2]), len(c.p[3])
    return [n_pose - 1, c.n_fixed, n_pose // 2], [n_lm - 1, 3, 0, n_lm // 2]


def leaving(c):
    """(leaving frames, record mask) of the marginal_prior call: frames 1 and 2 leave with their records and those of
    frames 3 and 4 (which the marginal then names); the mask is in record order, so the call reads the permutation."""
    frame = c.p[4]
    return [1, 2], np.isin(frame, [1, 2, 3, 4]).astype(np.uint8)


def dirty(h, c):
    """Leave as much behind under c as the API allows: the problem with its weights, loss and features, the reduced
    curvature, a device-driven run of three iterations, both covariances and a marginal (their plans and workspaces), a
    saved state, and last a host-driven trial that is neither accepted nor rejected."""
    import ptzba
    apply(h, c)
    if c.loss != "linear":
        h.set_huber_curvature(0.1)
    ptzba.LMSolver(h, max_iter=3, **_TIGHT).run()
    h.covariance(landmarks="all")
    h.covariance_joint(*joint_selection(c))
    h.marginal_prior(leaving(c)[0], drop_mask=leaving(c)[1])
    h.save_state()
    if c.loss != "linear":
        h.set_huber_curvature(0.1)
    h.linearize()
    h.build_reduced(1e-3)
    h.solve_reduced()  # (no accept: the trial stays open)


def abandon_device_run(h, c):
    """A device-driven run under c stopped after lm_solve, with no lm_decide."""
    import ptzba
    apply(h, c)
    h.lm_start()
    h.lm_init(ptzba.ptzba_lm_opts(1e-15, 1e-15, 0.0, ptzba.LAMBDA0, ptzba.MIN_LAMBDA, 1e16, 3, 30, 0,
                                  ptzba.HUBER_CURVATURE, ptzba.CURVATURE_SWITCH))
    h.lm_build()
    h.lm_solve()


def abandon_host_run(h, c):
    """A host-driven run under c stopped between solve_reduced and accept, at a reduced curvature."""
    apply(h, c)
    if c.loss != "linear":
        h.set_huber_curvature(0.1)
    h.linearize()
    h.step(1e-2)
    h.accept(True)
    h.linearize()
    h.step(1e-1)


def _result(res):
    return np.array([res.status, res.cost, res.initial_cost, res.njev, res.nfev, res.iterations], np.float64)


def observe(h, c, between_solves=True):
    """Everything the comparison reads from a handle that holds c (apply(h, c) has run), as a dict of exact arrays (and
    tuples of them).  Wall-clock fields (device_ms, time) are left out.  between_solves=False stops before the
    covariance and marginal calls (a handle in the caller-exchange mode refuses them)."""
    import ptzba
    u, v, ptz0, rays0, frame, landmark, xy, weight = c.p
    o = {}
    o["info"] = np.array(list(h.info().values()), np.int64)
    o["k1_info"] = np.array(h.k1_info(), np.int64)
    mi = h.k1_merge_info()
    o["k1_merge_info"] = np.array([mi["runs"], mi["merged"], mi["one_record"]], np.int64)
    si = h.solver_info()
    o["solver_info"] = np.array([si["n_aug"], si["ld"], si["levels"], si["ordering"] == "nested", si["nd_depth"],
                                 ("lookahead", "left-looking", "blocked").index(si["backsolve"]), si["n_slot"],
                                 si["schur_items"], si["pattern_tiles"]], np.int64)
    o["pose_prior_info"] = np.array(h.pose_prior_info(), np.float64)
    o["ray_prior_info"] = np.array(h.ray_prior_info(), np.float64)
    o["marginal_prior_info"] = np.array(h.marginal_prior_info(), np.float64)
    active, lam = h.displacement_info()
    o["displacement_info"] = np.concatenate([[float(active)], lam])
    # two host-driven steps: the second reads the damping memory of the first
    h.set_state(ptz0, rays0)
    h.linearize()
    h.build_reduced(1e-2)
    h.solve_reduced()
    o["scalars1"] = np.array(h.read_scalars(), np.float64)
    h.accept(True)
    o["state1"] = h.get_state()
    h.linearize()
    h.build_reduced(1e-1)
    h.solve_reduced()
    o["scalars2"] = np.array(h.read_scalars(), np.float64)
    h.accept(True)
    o["state2"] = h.get_state()
    o["residual"] = h.residual(np.concatenate([ptz0.reshape(-1), rays0.reshape(-1)]))
    # the device loop from a restored snapshot, then the host loop
    h.set_state(ptz0, rays0)
    h.save_state()
    o["resident"] = _result(h.solve_resident(restore=True, max_iter=3, **_TIGHT))
    o["resident_state"] = h.get_state()
    h.set_state(ptz0, rays0)
    o["host_loop"] = _result(ptzba.LMSolver(h, max_iter=3, device_loop=False, **_TIGHT).run())
    o["host_loop_state"] = h.get_state()
    if not between_solves:
        return o
    # the between-solves calls, at the initial state (where cov_ref states the blocks)
    h.set_state(ptz0, rays0)
    pose_cov, ray_cov, ci = h.covariance(landmarks="all")
    o["covariance"] = (pose_cov, ray_cov, np.array([ci["scale"], ci["min_pivot"], ci["n_free"]]))
    cj, cji = h.covariance_joint(*joint_selection(c))
    o["covariance_joint"] = (cj, np.array([cji["scale"], cji["min_pivot"], cji["n_free"]]))
    m, st = h.marginal_prior(leaving(c)[0], drop_mask=leaving(c)[1])
    o["marginal_prior"] = (m.frames, m.lin, m.info, m.grad, np.array([m.offset, st["min_pivot"]]),
                           np.array([st["dropped_records"], st["dropped_landmarks"], st["marginal_absorbed"]] +
                                    st["absorbed"], np.int64))
    return o


def differing(a, b):
    """Names of the items of two observe() results that are not equal bit for bit ([] when all are)."""
    assert a.keys() == b.keys()
    bad = []
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], tuple) else ((a[k],), (b[k],))
        if len(xs) != len(ys) or not all(np.array_equal(x, y) for x, y in zip(xs, ys)):
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------ the references
def first_step_errors(c, o):
    """Relative errors of observe()'s first step (lam 1e-2 from the initial state, IRLS curvature) against
    k1_cases.reference: cost, trial cost, the step per parameter kind, predicted reduction, |delta|^2."""
    assert c.has_reference
    p = c.p
    k = ("ref", c.name, c.loss, c.f_scale)
    if k not in _cache:
        _cache[k] = kc.reference(p, 1e-2, c.loss, 1.0, c.f_scale)
    ref = _cache[k]
    s, (ptz1, rays1) = o["scalars1"], o["state1"]
    dx = np.concatenate([(ptz1 - p[2])[1:].reshape(-1), (rays1 - p[3]).reshape(-1)])
    nf = ref["n_free_pose"]
    kg, kr = kc.split_kinds(dx, nf), kc.split_kinds(ref["dx"], nf)
    rel = lambda a, b: abs(a - b) / abs(b)
    return dict(cost=rel(s[0], ref["cost"]), trial_cost=rel(s[1], kc.cost_at(p, ptz1, rays1, c.loss, c.f_scale)),
                step=max(float(np.abs(kg[q] - kr[q]).max() / np.abs(kr[q]).max()) for q in kr),
                pred=rel(s[2], ref["pred"]), dx2=rel(s[3], ref["dx2"]), info=float(s[5]))


def covariance_errors(c, o):
    """cov_ref.block_err of observe()'s covariance blocks against the dense inverse at the initial state (linear or
    Huber loss, no feature; weighted records enter repeated, k1_cases.expand)."""
    import cov_ref
    assert c.loss in ("linear", "huber") and not c.features
    k = ("cov", c.name, c.loss, c.f_scale, c.n_fixed)
    if k not in _cache:
        u, v, ptz0, rays0, frame, landmark, xy, _ = kc.expand(c.p)
        q = types.SimpleNamespace(n_pose=len(ptz0), n_landmark=len(rays0), frame=frame, landmark=landmark, xy=xy, u=u, v=v)
        _cache[k] = cov_ref.dense_blocks(q, ptz0, rays0, c.loss, c.f_scale, c.n_fixed)
    pose_ref, ray_ref = _cache[k]
    pose_cov, ray_cov, _ = o["covariance"]
    return cov_ref.block_err(pose_cov, pose_ref), cov_ref.block_err(ray_cov, ray_ref)


# ------------------------------------------------------------------------------------------------ DBuf::alloc
# the (A, B) pairs of the size transitions; A carries everything dirty() can leave behind
FULL = dict(loss="cauchy", f_scale=2.5, features=True)
SIZE_PAIRS = {"shrink": (Case("P200w", **FULL), Case("P64")),
              "growth_within_slack": (Case("P140w", **FULL), Case("P150")),
              "growth_beyond_slack": (Case("P64w", **FULL), Case("P200"))}


def dbuf_alloc(cap, n):
    """csrc/host_util.h DBuf::alloc restated: (capacity after alloc(n) on a buffer of capacity `cap` (0: none), whether
    the allocation was kept)."""
    n = n or 16
    if cap and n <= cap <= 4 * n + (1 << 20):
        return cap, True
    return (((n + n // 4 + 4095) & ~4095) if n < (256 << 20) else n), False


def buffer_sizes(c):
    """Bytes set_problem asks for, for the buffers whose sizes follow from info() and solver_info() (csrc/api.hip
    upload_problem): host only, through ptzba.plan_summary."""
    import ptzba
    u, v, ptz0, rays0, frame, landmark, xy, weight = c.p
    n_pose, n_lm, n = len(ptz0), len(rays0), len(frame)
    e = 4 if c.precision else 8
    win = window(c)
    if win is None:
        win = ptzba.frame_coupling_window(n_pose, frame, landmark)
    ld = ptzba.plan_summary(win, c.n_fixed, c.ordering)["ld"]
    n_seg = kc.layout(c.p)["n_segments"]
    return dict(sys=(ld * ld + 3 * ld) * 8, Ldiag=ld * 32 * 8, dpose=ld * 8, ptz=3 * n_pose * 8, rays=2 * n_lm * 8,
                lm_out=n_lm * 64, rec_xy=(2 * n + 16) * e, rec_seg=4 * n, seg_row=4 * n_seg, ft64=n_pose * 64)
