"""The smallest problems at which K2 (the reduced camera system: k_schur*, k_schur_reduce and the tile / list / split
builder of ptzba_set_problem) can go wrong; problems are k1_cases tuples (u, v, ptz0, rays0, frame, landmark, xy, weight).
Free frames start at 1, so the F1 blocks of 32 frames begin at 1, 33, 65, ...

  crafted   k1_cases.craft(): 400 poses, landmarks over every frame (chunks 0-6), ~5,500 records
  tiny      12 landmarks over 100 poses (one-batch lists, chunk 1)
  a         split tiles: 65 poses; block 1 holds 400 landmarks of 2-4 consecutive frames (split weight 256, weight 6 per
            chunk-0 landmark: 10 splits -- the reduce's eight-in-flight loop and its remainder), block 33 holds 98 (3 splits
            of 32 | 33 | 33: the remainder alone, and lists of 16 k + 1 landmarks).  One F1 block cannot hold two tiles
            without a partner chunk, hence 65 poses and not 33
  b34 b65 b161  ragged blocks and far chunks: the last F1 block holds 1 | 32 | 32 frames and its partner range passes
            n_pose; landmarks seen in {f, f + 70} and {f, f + 130} only (chunks 1 and 2 reached at n_pose = 161), neighbour
            pairs {f, f + 1} so that every frame is seen at any n_pose, one landmark seen by every frame
  b161gap   the same without the {f, f + 70} pairs and without the all-frame landmark (which enters every chunk): the
            middle chunk's list is empty and its tile is not built, though the coupling window covers it; and the only
            far-chunk problem that admits a dissected order (mirrored blocks)
  c         full lists: 33 poses and the smallest number of two-record landmarks at which the longest list has
            SCHUR_LMAX = 512 landmarks (32 batches; the cap binds instead of the split weight)
  e_*       operand ranges on the crafted structure at 96 poses: f in {800, 3000, 20000}, a 700-record segment beside
            single records, gross outliers of 300 and 1000 px (Huber weights down to 1e-3)
  grid      synthetic.make_grid_problem: 120 poses, 5,324 landmarks, 1.29M records; lists of 151-206 landmarks (10-13
            batches: more than k_schur_mfp's operand ring holds, so every item re-fills its buffers)
  config2   synthetic.make_problem("config2"): lists of at most 43 landmarks (1-3 batches)
"""
import numpy as np

import k1_cases as kc
from oracle import ptz_oracle as orc


def tiny():
    """12 landmarks over 100 poses (3 seen by every frame, 9 by 12 consecutive frames): every K2 list has at most 16
    landmarks, and the all-frame landmarks reach partner chunk 1.  (A dict; as_tuple gives the k1_cases form.)"""
    rng = np.random.default_rng(11)
    n_pose, u, v = 100, 640.0, 360.0
    frames = [np.arange(n_pose)] * 3 + [np.arange(s, s + 12) for s in range(0, 99, 11)][:9]
    landmark = np.concatenate([np.full(len(f), l) for l, f in enumerate(frames)]).astype(np.int32)
    frame = np.concatenate(frames).astype(np.int32)
    n_lm = len(frames)
    ptz = np.stack([np.linspace(48.0, 56.0, n_pose), -10.0 + rng.normal(0, 0.2, n_pose),
                    3000.0 + rng.normal(0, 40.0, n_pose)], -1)
    rays = np.stack([rng.uniform(50.0, 54.0, n_lm), rng.uniform(-12.0, -8.0, n_lm)], -1)
    px, py = orc.from_ray_to_image(u, v, ptz[frame, 2], ptz[frame, 0], ptz[frame, 1], rays[landmark, 0], rays[landmark, 1])
    xy = np.stack([px, py], -1) + rng.normal(0, 0.5, (len(frame), 2))
    xy[::7] += 6.0  # both Huber branches
    ptz0 = ptz + rng.normal(0, 1.0, (n_pose, 3)) * np.array([0.015, 0.01, 5.0])
    ptz0[0] = ptz[0]
    return dict(n_pose=n_pose, n_landmark=n_lm, frame=frame, landmark=landmark, xy=xy, u=u, v=v, ptz=ptz0,
                rays=rays + rng.normal(0, 0.01, (n_lm, 2)))


def as_tuple(d):
    return d["u"], d["v"], d["ptz"], d["rays"], d["frame"], d["landmark"], d["xy"], None


def synthetic_case(name):
    """The generator's problems as they come (nothing moved away from the Huber unit: the tests run them with f_scale 1
    and curvature 1, where the weights are continuous at the unit)."""
    import synthetic
    p = (synthetic.make_grid_problem(120, 6000, -20.0, 20.0, (-10.0, 0.0, 10.0), seed=3) if name == "grid"
         else synthetic.make_problem(name, seed=0))
    return p.u, p.v, p.init_ptz, p.init_rays, p.frame, p.landmark, p.xy, None


def _away_from_huber_unit(u, v, ptz0, rays0, frame, landmark, xy):
    """As k1_cases.craft(): no (r / f_scale)^2 within 2e-3 of the Huber unit at x0, for either scale the tests use --
    fp32 records must not flip a branch.  Offending observations move 0.02 px away from the threshold."""
    n_pose = len(ptz0)
    for _ in range(8):
        r = orc.compute_residual_records(np.concatenate([ptz0.reshape(-1), rays0.reshape(-1)]), n_pose, u, v,
                                         frame.astype(np.int64), landmark.astype(np.int64), xy).reshape(-1, 2)
        bad = np.zeros(r.shape, bool)
        grow = np.zeros(r.shape, bool)
        for fs in kc.F_SCALES:
            near = np.abs((r / fs) ** 2 - 1.0) < 2e-3
            bad |= near
            grow |= near & (np.abs(r) >= fs)
        if not bad.any():
            break
        xy = xy - np.where(bad, np.where(grow, 1.0, -1.0) * np.sign(r) * 0.02, 0.0)
    return xy


def build(n_pose, segs, seed, f0=3000.0, gross=None):
    """A problem from [(landmark, frame, records)] segments: poses on an arc (pan 48-56 deg, tilt ~ -10, f ~ f0), rays
    within a box whose image stays ~ +-200 px wide at any f0, observations = projection + 0.5 px noise, 15 % of the
    records 8 px further off; gross = (px, every): every `every`-th record that far off instead."""
    rng = np.random.default_rng(seed)
    u, v = 640.0, 360.0
    seg_lm = np.array([s[0] for s in segs])
    seg_fr = np.array([s[1] for s in segs])
    cnt = np.array([s[2] for s in segs])
    n_lm = int(seg_lm.max()) + 1
    landmark = np.repeat(seg_lm, cnt).astype(np.int32)
    frame = np.repeat(seg_fr, cnt).astype(np.int32)
    n = len(frame)
    ptz = np.stack([np.linspace(48.0, 56.0, n_pose) + rng.normal(0, 0.05, n_pose),
                    -10.0 + rng.normal(0, 0.2, n_pose), f0 * (1.0 + rng.normal(0, 0.013, n_pose))], -1)
    rays = np.stack([rng.uniform(50.0, 54.0, n_lm), rng.uniform(-12.0, -8.0, n_lm)], -1)
    px, py = orc.from_ray_to_image(u, v, ptz[frame, 2], ptz[frame, 0], ptz[frame, 1], rays[landmark, 0], rays[landmark, 1])
    xy = np.stack([px, py], -1) + rng.normal(0, 0.5, (n, 2))
    out = rng.random(n) < 0.15
    xy[out] += 8.0 * rng.choice([-1.0, 1.0], (int(out.sum()), 2))
    if gross is not None:
        xy[::gross[1]] += gross[0] * rng.choice([-1.0, 1.0], (len(xy[::gross[1]]), 2))
    ptz0 = ptz + rng.normal(0, 1.0, (n_pose, 3)) * np.array([0.015, 0.01, f0 / 600.0])
    ptz0[0] = ptz[0]
    rays0 = rays + rng.normal(0, 0.01, (n_lm, 2))
    perm = rng.permutation(n)
    frame, landmark, xy = frame[perm], landmark[perm], xy[perm]
    xy = _away_from_huber_unit(u, v, ptz0, rays0, frame, landmark, xy)
    return u, v, ptz0, rays0, frame, landmark, xy, None


def case_a():
    rng = np.random.default_rng(21)
    segs, lm = [], 0
    for f1b, count in ((1, 400), (33, 98)):
        for _ in range(count):
            k = int(rng.integers(2, 5))
            s = int(rng.integers(f1b, f1b + 32 - k + 1))
            segs += [(lm, f, int(rng.integers(1, 3))) for f in range(s, s + k)]
            lm += 1
    return build(65, segs, 22)


def case_b(n_pose, gap=False):
    """gap: only the {f, f + 130} pairs and the neighbours -- no landmark reaches the middle chunk, whose tiles are not
    built at all: their entries inside the coupling window are zeroed by the build's prologue and written by nobody."""
    rng = np.random.default_rng(30 + n_pose)
    segs, lm = [], 0
    for f in range(0, n_pose):
        for d in ((130,) if gap else (70, 130)):
            if f + d < n_pose:
                segs += [(lm, f, int(rng.integers(1, 3))), (lm, f + d, int(rng.integers(1, 3)))]
                lm += 1
    # neighbours, so that every frame is seen at any n_pose (34 has no partner 70 frames on)
    for f in range(0, n_pose - 1):
        segs += [(lm, f, 1), (lm, f + 1, 1)]
        lm += 1
    if not gap:
        segs += [(lm, f, 1) for f in range(n_pose)]  # one landmark seen by every frame
    return build(n_pose, segs, 31 + n_pose)


C_POSES = 33


def case_c(n_lm):
    """n_lm landmarks of one record in each of two neighbouring frames of the one F1 block (1..32)."""
    rng = np.random.default_rng(40)
    s = rng.integers(1, 32, n_lm)
    segs = [(l, int(f) + k, 1) for l, f in enumerate(s) for k in (0, 1)]
    return build(C_POSES, segs, 41)


def c_landmarks():
    """The smallest landmark count at which the builder's longest list has 512 landmarks.  One chunk-0 tile of n
    landmarks weighs 6 n; the item target is min(256, max(64, 512 * 6 n / 480000)) and the split weight the smallest
    that meets it, so the tile is cut into `target` lists: ~156 landmarks each while the target grows with n (n up to
    40,000), then n / 256 -- 512 first at n = 256 * 511 + 1 = 130,817 (261,634 records), where ceil(n / SCHUR_LMAX) = 256
    splits are needed anyway: the cap binds.  tests/test_k2_ref.py checks both sides of the count against tile_plan()."""
    return 256 * 511 + 1


def case_e(f0=3000.0, heavy=False, gross=None, n_pose=96, seed=50):
    """The crafted structure (k1_cases._structure: all-frame, far, local and one-record landmarks, a 700-record segment)
    at 96 poses.  heavy=False trims the 700-record run to 1, so that only the `heavy` variation has it."""
    rng = np.random.default_rng(seed)
    segs, _ = kc._structure(n_pose, 0, rng)
    if not heavy:
        segs = [(l, f, 1 if c == 700 else c) for l, f, c in segs]
    return build(n_pose, segs, seed + 1, f0=f0, gross=gross)


E_VARIANTS = {
    "e_f800": dict(f0=800.0),
    "e_f3000": dict(f0=3000.0),
    "e_f20000": dict(f0=20000.0),
    "e_heavy": dict(heavy=True),
    "e_out300": dict(gross=(300.0, 9)),
    "e_out1000": dict(gross=(1000.0, 9)),
    # the two variations with the largest model error e_S at lambda 0 (4.4e-7 and 3.9e-7), together
    "e_f20000_heavy": dict(f0=20000.0, heavy=True),
}

NAMES = ("crafted", "crafted_w", "tiny", "a", "b34", "b65", "b161", "b161gap", "c") + tuple(E_VARIANTS)
PIPELINE_NAMES = ("tiny", "crafted", "grid", "config2")  # together: every shape of k_schur_mfp's hand-off
_cache = {}


def problem(name):
    """The case's problem tuple, built once."""
    if name not in _cache:
        if name in ("crafted", "crafted_w"):
            p = kc.craft(weighted=name == "crafted_w")
        elif name == "tiny":
            p = as_tuple(tiny())
        elif name in ("grid", "config2"):
            p = synthetic_case(name)
        elif name == "a":
            p = case_a()
        elif name == "b161gap":
            p = case_b(161, gap=True)
        elif name[0] == "b":
            p = case_b(int(name[1:]))
        elif name == "c":
            p = case_c(c_landmarks())
        else:
            p = case_e(**E_VARIANTS[name])
        _cache[name] = p
    return _cache[name]
