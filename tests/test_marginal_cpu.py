"""CPU tests of the keyframe marginalisation's definition and of ptzba.Marginal's algebra (no GPU).

tests/marg_ref.py is the dense numpy reference of include/ptzba.h ptzba_marginal_prior.  The identity it must satisfy:
one undamped Gauss-Newton step of the clone problem Q1 (p with the dropped records relabelled to fresh landmarks)
equals the step of Q2 (p without the dropped records) plus the marginal on K, on the kept poses and the rays."""
import functools

import numpy as np
import pytest

import marg_ref
import prior_ref


@functools.lru_cache(maxsize=None)
def _identity(cfg, E):
    p = prior_ref.problem(cfg)
    m = marg_ref.marginal(p, p.init_ptz, p.init_rays, E)[0]
    return m, marg_ref.step_identity(p, E, m)[:3]


@pytest.mark.parametrize("cfg,E,n_k,moved_min", [("config1", (0,), 6, 0.1), ("config1", (3,), 7, 0.005),
                                                 ("config1", (0, 1), 7, 0.1), ("config2", (0,), 21, 0.05),
                                                 ("config2", (24, 25), 45, 0.001)])
def test_step_identity(cfg, E, n_k, moved_min):
    """Q2 + marginal takes Q1's step to 1e-9 relative; without the marginal the step is measurably another one."""
    m, (err, moved, scale) = _identity(cfg, E)
    ev = np.linalg.eigvalsh(m.info)
    print(f"{cfg} E={list(E)}: |K| {len(m.frames)}, identity {err:.2e}, without the marginal {moved:.2e}, "
          f"max|dx| {scale:.3g}, cond(A_EE) {m.cond_EE}, eig(Lambda) [{ev.min():.3g}, {ev.max():.3g}]")
    assert len(m.frames) == n_k
    assert err <= 1e-9, err
    assert moved >= moved_min, moved
    assert ev.min() >= -1e-12 * np.abs(m.info).max() * len(ev)  # PSD up to the elimination's rounding


def _random_marginal(rng, frames):
    import ptzba
    n = 3 * len(frames)
    A = rng.standard_normal((n, max(n - 3, 1)))  # singular on purpose
    return ptzba.Marginal(frames, rng.standard_normal((len(frames), 3)), A @ A.T, rng.standard_normal(n),
                          float(rng.uniform(0, 3)))


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1.0)


def test_marginal_algebra_keeps_q():
    """relinearise, condition, merge_marginals and reindex leave q(x) unchanged at random x (1e-12 relative)."""
    import ptzba
    rng = np.random.default_rng(0)
    a = _random_marginal(rng, [2, 5, 7, 9])
    b = _random_marginal(rng, [1, 5, 9, 11, 12])
    for _ in range(5):
        x = rng.standard_normal((14, 3))
        assert _close(a.relinearise(rng.standard_normal((4, 3))).value(x), a.value(x))
        # condition: frames 5 and 3 held at x's values (3 is not named: ignored)
        c = a.condition([5, 3], x[[5, 3]])
        assert c.frames.tolist() == [2, 7, 9] and _close(c.value(x), a.value(x))
        y = x.copy()
        y[5] += 1.0  # the conditioned factor no longer depends on frame 5
        assert c.value(y) == c.value(x)
        m = ptzba.merge_marginals(a, b)
        assert m.frames.tolist() == [1, 2, 5, 7, 9, 11, 12]
        assert _close(m.value(x), a.value(x) + b.value(x))
        np.testing.assert_array_equal(m.lin[[2, 4]], b.lin[[1, 2]])  # b's point where both name a frame
        mapping = {2: 8, 5: 0, 7: 3, 9: 1}
        r = a.reindex(mapping)
        assert r.frames.tolist() == [0, 1, 3, 8]
        xr = np.zeros((14, 3))
        for f, g in mapping.items():
            xr[g] = x[f]
        assert _close(r.value(xr), a.value(x))
        assert _close(a.value({2: x[2], 5: x[5], 7: x[7], 9: x[9]}), a.value(x))
    assert ptzba.merge_marginals(None, a) is a and ptzba.merge_marginals(a, None) is a
    gone = a.condition(a.frames, np.zeros((4, 3)))
    assert len(gone.frames) == 0 and _close(gone.value(np.zeros((14, 3))), a.value(np.zeros((14, 3))))
    with pytest.raises(ValueError):
        ptzba.Marginal([1, 1], np.zeros((2, 3)), np.eye(6), np.zeros(6), 0.0)
    with pytest.raises(ValueError):
        ptzba.check_marginal(ptzba.Marginal([1], np.zeros((1, 3)), -np.eye(3), np.zeros(3), 0.0))


def test_drop_mask_against_a_loop():
    import ptzba
    p = prior_ref.problem("config1")
    for E in ([0], [3], [0, 1], [9, 2, 4], []):
        got = ptzba.drop_mask(p.frame, E)
        assert got.dtype == np.uint8 and len(got) == len(p.frame)
        np.testing.assert_array_equal(got, marg_ref.drop_mask_loop(p.frame, E))
    assert ptzba.drop_mask(p.frame, [0]).sum() > 0
    with pytest.raises(ValueError):
        ptzba.drop_mask(p.frame[:-1], [0])


@pytest.mark.parametrize("loss,f_scale", [("linear", 1.0), ("huber", 1.0)])
def test_q_is_nonnegative(loss, f_scale):
    """The offset keeps q >= 0: q is the dropped terms' quadratic model minimised over the clones and E, and Huber's
    rho majorises its IRLS quadratic.  Random x up to 20 sigma of the initial noise around lin, and the minimiser."""
    p = prior_ref.problem("config1")
    rng = np.random.default_rng(1)
    for E in ((0,), (3,), (0, 1)):
        m = marg_ref.marginal(p, p.init_ptz, p.init_rays, E, loss=loss, f_scale=f_scale)[0]
        assert m.offset > 0
        scale = 1e-12 * m.offset
        for _ in range(20):
            x = p.init_ptz + rng.standard_normal(p.init_ptz.shape) * np.array([0.5, 0.2, 40.0]) * rng.uniform(0, 20)
            assert m.value(x) >= -scale
        d = -np.linalg.pinv(m.info, rcond=1e-10, hermitian=True) @ m.grad  # (the test may use a pseudo-inverse; the library never does)
        x = p.init_ptz.copy()
        x[m.frames] += d.reshape(-1, 3)
        q = m.value(x)
        print(f"{loss} E={list(E)}: offset {m.offset:.6g}, min q {q:.6g}")
        assert q >= -1e-9 * m.offset, q
