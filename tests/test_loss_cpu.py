"""CPU tests of tests/loss_ref.py, the reference of the robust losses soft_l1, cauchy and arctan: its rho functions
against scipy's own, the crafted case's branch population, the float32 forms on a small-residual case, and the recorded
stationary points of the GPU solve tests (tests/golden/loss_points.npz)."""
import numpy as np
import pytest

import k1_cases as kc
import loss_ref


@pytest.mark.parametrize("f_scale", [1.0, 2.5])
@pytest.mark.parametrize("loss", loss_ref.SMOOTH)
def test_rho_matches_scipy(loss, f_scale):
    """z from 1e-8 to 1e4: 1/2 f^2 sum rho and rho' r equal scipy least_squares' .cost and .grad at x0 (identity
    residual and Jacobian) to 1e-13; the curvature column equals a central difference of rho' r in r to 1e-6."""
    from scipy.optimize import least_squares
    z = np.logspace(-8, 4, 241)
    r = f_scale * np.sqrt(z) * np.where(np.arange(len(z)) % 2, -1.0, 1.0)
    eye = np.eye(len(r))
    res = least_squares(lambda x: x, r, jac=lambda x: eye, loss=loss, f_scale=f_scale, max_nfev=1)
    assert np.array_equal(res.x, r)
    _, rho, w1, w2 = loss_ref.weights(r, loss, 1.0, f_scale)
    cost = 0.5 * f_scale ** 2 * float(np.sum(rho))
    e_cost = abs(cost - res.cost) / res.cost
    e_grad = float(np.max(np.abs(w1 * r - res.grad) / np.abs(res.grad)))
    assert np.array_equal(w2, w1)  # hc = 1: IRLS (rho'' <= 0)
    wn = loss_ref.rho_all((r / f_scale) ** 2, loss)[2]
    assert np.all(wn <= w1)
    h = 1e-5 * np.abs(r)
    g = lambda t: loss_ref.rho_all((t / f_scale) ** 2, loss)[1] * t  # noqa: E731
    fd = (g(r + h) - g(r - h)) / (2.0 * h)
    e_curv = float(np.max(np.abs(fd - wn) / np.maximum(np.abs(wn), w1)))
    print(f"{loss} f_scale {f_scale}: cost {e_cost:.2e} grad {e_grad:.2e} curvature vs central difference {e_curv:.2e}")
    assert e_cost <= 1e-13 and e_grad <= 1e-13, (e_cost, e_grad)
    assert e_curv <= 1e-6, e_curv
    # the floor: w2 = max(wn, hc rho')
    w2f = loss_ref.weights(r, loss, 0.1, f_scale)[3]
    assert np.array_equal(w2f, np.maximum(wn, 0.1 * w1)) and np.all(w2f > 0)


def test_huber_and_linear_are_k1_cases():
    r = np.linspace(-9.0, 9.0, 181)
    for loss in ("linear", "huber"):
        for a, b in zip(loss_ref.weights(r, loss, 0.1, 2.5), kc._weights(r, loss, 0.1, 2.5)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("f_scale", [1.0, 2.5])
@pytest.mark.parametrize("loss", ["cauchy", "arctan"])
def test_crafted_case_populates_both_branches(loss, f_scale):
    """On k1_cases.craft() at x0 the share of scalar residuals with negative Newton curvature lies in [0.1, 0.6]:
    both branches of max(rho' + 2 z rho'', hc rho') are populated."""
    share = loss_ref.negative_curvature_share(kc.craft(), loss, f_scale)
    print(f"{loss} f_scale {f_scale}: negative Newton curvature in {share:.3f} of the residuals")
    assert 0.1 <= share <= 0.6, share


def test_small_residual_case_discriminates():
    """Residuals ~0.005 px at f_scale 2.5: in float32 the direct forms log(1 + z) and 2 (sqrt(1 + z) - 1) miss the fp64
    cost by more than 2e-5, the forms the kernels use are within 2e-7."""
    p = loss_ref.small_residual_case()
    r = loss_ref.residual(p)
    fs = 2.5
    assert 0.003 < np.std(r) < 0.007 and len(r) > 10000
    for loss in loss_ref.SMOOTH + ("linear",):
        c64 = loss_ref.cost_at(p, p[2], p[3], loss, fs)
        good = abs(loss_ref.cost32(r, loss, fs, naive=False) - c64) / c64
        print(f"{loss}: float32 accurate form {good:.2e}", end="")
        assert good <= 2e-7, (loss, good)
        if loss in ("cauchy", "soft_l1"):
            bad = abs(loss_ref.cost32(r, loss, fs, naive=True) - c64) / c64
            print(f", naive form {bad:.2e}", end="")
            assert bad > 2e-5, (loss, bad)
        print()


@pytest.mark.parametrize("name", list(loss_ref.POINTS))
def test_recorded_points_are_stationary(name):
    """Every recorded point is stationary under loss_ref and no worse in cost than what scipy's trf reaches from the
    same start in loss_ref.SCIPY_NFEV (300) evaluations -- recorded with the point by `python tests/loss_ref.py`,
    since those runs take minutes (scipy stops short with robust losses:
    test_gpu_ba.test_config2_ftol_stop_matches_scipy_trf).  That the recorded scipy cost belongs to this problem is
    checked with a short run here: trf's cost only decreases, so after 5 evaluations it is not below the recorded one
    (to 1e-6: scipy's own sums differ in rounding between runs)."""
    p, ptz, rays, c = loss_ref.point(name)
    cfg, loss, fs, _ = loss_ref.POINTS[name]
    s = loss_ref.stationarity(p, ptz, rays, loss, fs)
    assert np.array_equal(ptz[0], p.init_ptz[0])
    c_scipy, nfev, status = loss_ref.scipy_record(name)
    _, _, c_short = loss_ref.scipy_solve(p, p.init_ptz, p.init_rays, loss, fs, max_nfev=5)
    print(f"{name}: relative gradient {s:.2e}, cost {c:.9g}, scipy after {nfev} evaluations (status {status}) "
          f"{c_scipy:.9g}, after 5 {c_short:.9g}")
    assert s < 1e-9, s
    assert nfev <= loss_ref.SCIPY_NFEV and c_short >= c_scipy * (1.0 - 1e-6), (c_short, c_scipy)
    assert c <= c_scipy * (1.0 + 1e-12), (c, c_scipy)
