"""The run rule of K1's merged record stream, stated in numpy, against the runs ptzba_set_problem's host front forms
(ptzba_k1_merge_runs: the same host passes, no device).

A run is a maximal sequence of adjacent records of one (landmark, frame) segment, in the (landmark, frame, original
index) order, whose STORED records are bit-identical: the delta pair from the segment's first observation, rounded to
the handle's record precision, and the user weight in that precision.  Bits, not values: -0.0 and +0.0 differ; two
observations that differ in fp64 but round to one fp32 delta are one fp32 run and two fp64 runs; a non-adjacent repeat
stays a record of its own.  K1 reads the merged stream when the runs are at most half the records."""
import numpy as np
import pytest

FP64, FP32 = 0, 1


def numpy_runs(n_pose, frame, landmark, xy, weight, precision):
    """(segments, first original index per run, multiplicity per run) by the rule above."""
    real, bits = (np.float32, np.uint32) if precision == FP32 else (np.float64, np.uint64)
    frame, landmark = np.asarray(frame, np.int64), np.asarray(landmark, np.int64)
    n = len(frame)
    if n == 0:
        return 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    o = np.lexsort((np.arange(n), frame, landmark))
    key = landmark[o] * n_pose + frame[o]
    seg_start = np.concatenate([[True], key[1:] != key[:-1]])
    base = np.asarray(xy, np.float64)[o][np.maximum.accumulate(np.where(seg_start, np.arange(n), 0))]
    stored = (np.asarray(xy, np.float64)[o] - base).astype(real).view(bits).reshape(n, 2)
    w = (np.ones(n) if weight is None else np.asarray(weight, np.float64))[o].astype(real).view(bits)
    differ = (stored[1:] != stored[:-1]).any(axis=1) | (w[1:] != w[:-1])
    start = seg_start | np.concatenate([[True], differ])
    first = np.flatnonzero(start)
    return int(seg_start.sum()), o[first], np.diff(np.concatenate([first, [n]]))


def random_set(seed, n_pose=9, n_lm=40, n=1500, weighted=False):
    """Random small record set with forced repeats: per (landmark, frame) one keypoint; a record is that keypoint, or
    it moved by a pixel, by 1 + 1e-9 px (the same fp32 delta as a pixel, another fp64 delta), or to the other sign of a zero delta; weights
    (when given) mostly 1, sometimes 2 -- inside runs as well."""
    rng = np.random.default_rng(seed)
    frame = rng.integers(0, n_pose, n).astype(np.int32)
    landmark = rng.integers(0, n_lm, n).astype(np.int32)
    kp = np.stack([100.0 + 37.0 * frame + landmark, 20.0 + 3.0 * landmark], -1).astype(np.float64)
    xy = kp.copy()
    c = rng.integers(0, 12, n)
    xy[c == 0, 0] += 1.0
    xy[c == 1, 0] += 1.0 + 1e-9
    # a segment whose keypoint x is 0: records at +0.0 and -0.0 (delta bits differ unless the base is -0.0 itself)
    z = landmark == 3
    xy[z, 0] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    weight = np.where(rng.random(n) < 0.85, 1.0, 2.0) if weighted else None
    return n_pose, n_lm, frame, landmark, xy, weight


@pytest.mark.parametrize("precision", [FP64, FP32])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_runs_match_numpy(seed, weighted, precision):
    import ptzba
    n_pose, n_lm, frame, landmark, xy, weight = random_set(seed, weighted=weighted)
    ns, first, mult = numpy_runs(n_pose, frame, landmark, xy, weight, precision)
    g_ns, g_runs, g_halves, g_first, g_mult = ptzba.k1_merge_runs(n_pose, n_lm, frame, landmark, xy, weight, precision)
    assert (g_ns, g_runs) == (ns, len(first))
    assert g_halves == (2 * len(first) <= len(frame))
    np.testing.assert_array_equal(g_first, first)
    np.testing.assert_array_equal(g_mult, mult)
    assert int(mult.sum()) == len(frame) and ns < len(first) < len(frame)  # repeats merged, and runs split


def test_the_forced_cases_split_as_stated():
    """One segment, hand-made: A A B A (adjacent-only), an fp32-equal / fp64-different pair, signed zeros, a weight
    change inside a run."""
    import ptzba

    def runs(xy, w=None, precision=FP64):
        n = len(xy)
        z = np.zeros(n, np.int32)
        got = ptzba.k1_merge_runs(1, 1, z, z, np.asarray(xy, np.float64), w, precision)
        ref = numpy_runs(1, z, z, xy, w, precision)
        np.testing.assert_array_equal(got[3], ref[1])
        np.testing.assert_array_equal(got[4], ref[2])
        return got[4].tolist()

    A, B = (10.0, 20.0), (11.0, 20.0)
    assert runs([A, A, B, A]) == [2, 1, 1]
    assert runs([A, A, A, A]) == [4]
    near = (10.0 + 1e-9, 20.0)  # delta 1e-9 is not 0 in either precision: the records hold deltas, not positions
    assert runs([A, near, near], precision=FP32) == [1, 2]
    assert runs([A, near, near], precision=FP64) == [1, 2]
    far, far_near = (1000.0, 20.0), (1000.0 + 1e-9, 20.0)  # deltas 990 and 990 + 1e-9: one fp32 value, two fp64 values
    assert runs([A, far, far_near], precision=FP32) == [1, 2]
    assert runs([A, far, far_near], precision=FP64) == [1, 1, 1]
    # base +0.0: the deltas of -0.0 are -0.0, of +0.0 are +0.0 -- equal values, different bits
    assert runs([(0.0, 1.0), (-0.0, 1.0), (-0.0, 1.0), (0.0, 1.0)], precision=FP32) == [1, 2, 1]
    assert runs([A, A, A, A], w=np.array([1.0, 1.0, 2.0, 2.0])) == [2, 2]
    assert runs([A, A, A, A], w=np.array([1.0, 1.0 + 1e-12, 1.0, 1.0]), precision=FP32) == [4]
    assert runs([A, A, A, A], w=np.array([1.0, 1.0 + 1e-12, 1.0, 1.0]), precision=FP64) == [1, 1, 2]


def test_halving_rule_and_empty_input():
    import ptzba
    z = np.zeros(4, np.int32)
    A, B, C = (1.0, 2.0), (3.0, 2.0), (5.0, 2.0)
    assert ptzba.k1_merge_runs(1, 1, z, z, np.array([A, A, B, B]))[1:3] == (2, True)    # 2 runs of 4 records
    assert ptzba.k1_merge_runs(1, 1, z, z, np.array([A, A, B, C]))[1:3] == (3, False)   # 3 runs of 4
    e = np.zeros(0, np.int32)
    assert ptzba.k1_merge_runs(2, 3, e, e, np.zeros((0, 2)))[:3] == (0, 0, False)
