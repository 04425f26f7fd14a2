"""CPU checks of tests/reuse_cases.py: the size transitions of the handle-reuse tests reach every regime of
DBuf::alloc's keep / replace rule (csrc/host_util.h, restated in reuse_cases.dbuf_alloc) for the buffers whose sizes
follow from info() and solver_info(), and every problem has its dense reference."""
import dataclasses

import numpy as np
import pytest

import k1_cases as kc
import reuse_cases as rc


def test_dbuf_rule_restated():
    """A first allocation gets a quarter of slack, rounded up to 4 KiB; an allocation is kept while
    n <= cap <= 4 n + 1 MiB and replaced otherwise; zero bytes ask for 16."""
    assert rc.dbuf_alloc(0, 1000) == (4096, False)
    assert rc.dbuf_alloc(0, 100000) == ((125000 + 4095) & ~4095, False)
    cap = rc.dbuf_alloc(0, 100000)[0]
    assert rc.dbuf_alloc(cap, cap) == (cap, True) and rc.dbuf_alloc(cap, cap + 1)[1] is False
    assert rc.dbuf_alloc(cap, 1) == (cap, True)  # 4 n + 1 MiB covers every small buffer
    big = 8 << 20
    assert rc.dbuf_alloc(big, (big - (1 << 20)) // 4) == (big, True)
    assert rc.dbuf_alloc(big, (big - (1 << 20)) // 4 - 1)[1] is False
    assert rc.dbuf_alloc(0, 0) == (4096, False) and rc.dbuf_alloc(0, 256 << 20) == (256 << 20, False)


def _regimes(a, b):
    """{buffer: (bytes under a, bytes under b, kept)} for set_problem(b) on a handle that was created for a."""
    sa, sb = rc.buffer_sizes(a), rc.buffer_sizes(b)
    return {k: (sa[k], sb[k], rc.dbuf_alloc(rc.dbuf_alloc(0, sa[k])[0], sb[k])[1]) for k in sa}


@pytest.mark.parametrize("precision", [0, 1])
def test_size_pairs_reach_every_regime(precision):
    pair = {k: tuple(dataclasses.replace(c, precision=precision) for c in v) for k, v in rc.SIZE_PAIRS.items()}
    shrink = _regimes(*pair["shrink"])
    slack = _regimes(*pair["growth_within_slack"])
    growth = _regimes(*pair["growth_beyond_slack"])
    print(f"precision {precision}: shrink {shrink}\n slack {slack}\n growth {growth}")
    # replaced on a large shrink: the dense system buffer, and only it
    assert [k for k, (na, nb, kept) in shrink.items() if not kept] == ["sys"] and shrink["sys"][1] < shrink["sys"][0]
    # kept on shrink: every other buffer, each strictly smaller under B
    assert all(nb < na for k, (na, nb, kept) in shrink.items() if kept) and len(shrink) >= 9
    assert shrink["Ldiag"][2] and shrink["dpose"][2]  # (the pointers solver_buffers() shows)
    # kept on growth within the quarter of slack: a buffer that really grows
    assert any(kept and nb > na for na, nb, kept in slack.values()), slack
    assert all(kept for na, nb, kept in slack.values()), slack
    # replaced on growth: the system, the factor's diagonal tiles and the records
    for k in ("sys", "Ldiag", "rec_xy", "rec_seg"):
        na, nb, kept = growth[k]
        assert nb > na and not kept, (k, growth[k])


def test_back_substitution_forms_follow_from_the_sizes():
    """P200 has at least 512 system rows (the blocked form), P64 and P140 fewer (the lookahead form)."""
    rows = {n: rc.buffer_sizes(rc.Case(n))["dpose"] // 8 for n in ("P64", "P140", "P150", "P200")}
    assert rows["P200"] >= 512 + 1 and max(rows["P64"], rows["P140"], rows["P150"]) < 512, rows
    assert 3 * (200 - 1) >= 512 > 3 * (150 - 1)


@pytest.mark.parametrize("name", rc.NAMES)
def test_every_problem_has_its_reference(name):
    p = rc.problem(name)
    ref = kc.reference(p, 1e-2)
    assert np.isfinite(ref["dx"]).all() and ref["pred"] > 0 and ref["cost"] > 0
    assert len(p[2]) <= 200 and len(p[4]) <= 5000
    assert (p[7] is not None) == (name.endswith("w"))
    lay = kc.layout(p)
    assert lay["n_records"] == len(p[4]) and min(lay["frames_seen"]) >= 1  # every frame observed: S is definite


def test_features_name_free_frames_inside_the_window():
    """The feature set of a Case: factors on free frames for n_fixed <= 2, valid for the library's host checks, and a
    record mask for marginal_prior that names frames outside the leaving ones."""
    import ptzba
    for name in ("P64", "P200w"):
        c = rc.Case(name, features=True)
        p = c.p
        facs = ptzba.check_pose_priors(rc.pose_factors(p), len(p[2]))
        assert min(int(f[0].min()) for f in facs) >= 2
        lm, mean, info = ptzba.check_ray_priors(rc.ray_priors(p), len(p[3]))
        assert len(lm) == 3 and len(set(lm.tolist())) == 2
        m = rc.marginal(p)
        ptzba.check_marginal(m)
        assert m.frames.min() >= 2 and np.linalg.matrix_rank(m.info) == 4
        E, mask = rc.leaving(c)
        assert mask.sum() > 0 and set(np.unique(p[4][mask != 0])) == {1, 2, 3, 4} and E == [1, 2]
