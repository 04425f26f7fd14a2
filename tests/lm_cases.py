"""Test infrastructure: the cases the LM decision rules are pinned with (tests/test_lm_ref.py on the CPU,
tests/test_gpu_lm_rules.py on the GPU).

TABLE: crafted scalars for one or several decisions in a row, each with the record it must give.  The expected
fields are written out by hand from the rules (tests/lm_ref.py's docstring), not computed by any code: the numbers
are dyadic wherever a product or a quotient is taken, so every expected value is exact (1/3 is the double nearest
to it, the 1/3 floor's own constant).

SCENARIOS: option sets that drive a real problem -- synthetic.make_small_problem(12, 150, -8.0, 8.0, seed=1): 12
poses, 101 landmarks, 3,520 records -- from far_start() through every exit of the rules.  reference(name) is the
reference's run of one of them on the dense fp64 numpy handle, computed once and shared.  Never used by the product."""
import functools
import math

import numpy as np

import lm_ref

INF, NAN = float("inf"), float("nan")
THIRD = 1.0 / 3.0

# options of a table row unless it names others: no test stops a plain step with |dx| = |x| = 1 and max |g| = 1
BASE = dict(ftol=1e-8, xtol=1e-8, gtol=0.0, lambda0=1.0, min_lambda=1e-12, max_lambda=1e16, max_iter=100,
            max_retries=30, gauss_newton=False)


def T(new, pred, dx2=1.0, x2=1.0, info=0, g_pose=1.0, g_ray=1.0):
    """The scalars of one trial: trial cost, predicted reduction, |dx|^2, |x|^2, factorisation status, the free
    poses' max |g| and the rays'."""
    return dict(new=new, pred=pred, dx2=dx2, x2=x2, info=info, g_pose=g_pose, g_ray=g_ray)


def E(accepted, iterations, nfev, trials, retries, status, done, lam, cost, nu):
    """The record after a decision (initial_cost is the row's starting cost throughout), and nu."""
    return dict(accepted=accepted, iterations=iterations, nfev=nfev, trials=trials, retries=retries, status=status,
                done=done, lam=lam, cost=cost, nu=nu)


class Row:
    def __init__(self, name, cost0, steps, needs_info=False, **opts):
        self.name, self.cost0, self.steps, self.needs_info = name, float(cost0), steps, needs_info
        kw = dict(BASE)
        kw.update(opts)
        self.opts = lm_ref.Opts(**kw)

    def __repr__(self):
        return self.name


OK = T(128.0, 256.0)      # from cost 256: actual 128, rho 1/2 -- accepted, lambda factor 1 - 0^3 = 1
BAD = T(512.0, 256.0)     # the cost rises: rho < 0
C = 64.0 - 2.0 ** -30     # a step from cost 64 whose reduction 2^-30 is far below ftol * 64 = 6.4e-7

TABLE = [
    Row("accept_rho_half", 256.0, [(OK, E(1, 1, 2, 1, 0, 0, 0, 1.0, 128.0, 2.0))]),
    # ---- what makes a trial unusable: rho = -1, rejected, lambda * nu, nu doubled
    Row("trial_cost_inf", 256.0, [(T(INF, 256.0), E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0))]),
    Row("trial_cost_nan", 256.0, [(T(NAN, 256.0), E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0))]),
    Row("pred_nan", 256.0, [(T(128.0, NAN), E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0))]),
    Row("pred_inf", 256.0, [(T(128.0, INF), E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0))]),
    Row("pred_zero", 256.0, [(T(128.0, 0.0), E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0))]),
    # pred < 0: a cost decrease is rejected, and so is an increase whose quotient actual / pred would be + 1/2
    Row("pred_negative", 256.0, [(T(128.0, -256.0), E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0)),
                                 (T(384.0, -256.0), E(0, 0, 3, 2, 2, 0, 0, 8.0, 256.0, 8.0))]),
    Row("info_nonzero", 256.0, [(T(128.0, 256.0, info=1), E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0))], needs_info=True),
    # ---- the Gauss-Newton start (lambda == 0): actual >= 0 is enough, lambda stays 0
    Row("gn_actual_zero", 256.0, [(T(256.0, 256.0), E(1, 1, 2, 1, 0, 0, 0, 0.0, 256.0, 2.0))], gauss_newton=True),
    Row("gn_actual_negative", 256.0, [(T(257.0, 256.0), E(0, 0, 2, 1, 1, 0, 0, 1e-9, 256.0, 4.0))],
        gauss_newton=True),
    Row("gn_accepts_without_pred", 256.0, [(T(128.0, 0.0), E(1, 1, 2, 1, 0, 0, 0, 0.0, 128.0, 2.0))],
        gauss_newton=True),
    Row("lm_actual_zero_rejected", 256.0, [(T(256.0, 256.0), E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0))]),
    # once damped, a GN run follows the LM rule: actual == 0 is rejected (lambda 1e-9 * 4), rho = 1 divides by three
    Row("gn_then_damped", 256.0, [(T(257.0, 256.0), E(0, 0, 2, 1, 1, 0, 0, 1e-9, 256.0, 4.0)),
                                  (T(256.0, 256.0), E(0, 0, 3, 2, 2, 0, 0, 4e-9, 256.0, 8.0)),
                                  (T(128.0, 128.0), E(1, 1, 4, 3, 0, 0, 0, 4e-9 * THIRD, 128.0, 2.0))],
        gauss_newton=True),
    # ---- ftol needs rho > 1/4: rho = 1/4 exactly (factor 1 + 1/8) goes on, rho = 1/2 stops
    Row("low_rho_tiny_actual_no_ftol", 64.0, [(T(C, 2.0 ** -28), E(1, 1, 2, 1, 0, 0, 0, 1.125, C, 2.0))]),
    Row("tiny_actual_ftol", 64.0, [(T(C, 2.0 ** -29), E(1, 1, 2, 1, 0, 2, 1, 1.0, C, 2.0))]),
    # ---- the lambda factor 1 - (2 rho - 1)^3 and its floor 1/3 (reached at rho = 0.9368...)
    # rho = 119/128: t = 55/64, t^3 = 166375/262144, factor 0.365329742431640625 > 1/3
    Row("factor_above_floor", 256.0, [(T(137.0, 128.0), E(1, 1, 2, 1, 0, 0, 0, 0.365329742431640625, 137.0, 2.0))]),
    # rho = 15/16: t = 7/8, factor 1 - 343/512 = 0.330078125 < 1/3
    Row("factor_at_floor", 256.0, [(T(136.0, 128.0), E(1, 1, 2, 1, 0, 0, 0, THIRD, 136.0, 2.0))]),
    Row("rho_above_one", 256.0, [(T(64.0, 128.0), E(1, 1, 2, 1, 0, 0, 0, THIRD, 64.0, 2.0))]),   # factor 1 - 8
    # rho = 1/16: t = -7/8, factor 1 + 343/512: a poor accepted step raises lambda
    Row("poor_step_raises_lambda", 256.0, [(T(248.0, 128.0), E(1, 1, 2, 1, 0, 0, 0, 1.669921875, 248.0, 2.0))]),
    Row("min_lambda_floor_default", 256.0, [(T(128.0, 128.0), E(1, 1, 2, 1, 0, 0, 0, 1e-12, 128.0, 2.0))],
        lambda0=1e-12),
    Row("min_lambda_floor_set", 256.0, [(T(128.0, 128.0), E(1, 1, 2, 1, 0, 0, 0, 0.5, 128.0, 2.0))], min_lambda=0.5),
    # ---- nu doubles with every rejection (lambda 1 * 2 * 4 * 8) and an accept resets it: the next rejection doubles
    Row("three_rejections_then_accept", 256.0, [(BAD, E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0)),
                                                (BAD, E(0, 0, 3, 2, 2, 0, 0, 8.0, 256.0, 8.0)),
                                                (BAD, E(0, 0, 4, 3, 3, 0, 0, 64.0, 256.0, 16.0)),
                                                (OK, E(1, 1, 5, 4, 0, 0, 0, 64.0, 128.0, 2.0)),
                                                (BAD, E(0, 1, 6, 5, 1, 0, 0, 128.0, 128.0, 4.0))]),
    # ---- gtol looks at the larger of the two maxima
    Row("gtol_pose_max", 256.0, [(T(128.0, 256.0, g_pose=2e-3, g_ray=1e-5), E(1, 1, 2, 1, 0, 0, 0, 1.0, 128.0, 2.0)),
                                 (T(64.0, 128.0, g_pose=5e-4, g_ray=1e-5), E(1, 2, 3, 2, 0, 1, 1, 1.0, 64.0, 2.0))],
        gtol=1e-3),
    Row("gtol_ray_max", 256.0, [(T(128.0, 256.0, g_pose=1e-5, g_ray=2e-3), E(1, 1, 2, 1, 0, 0, 0, 1.0, 128.0, 2.0)),
                                (T(64.0, 128.0, g_pose=1e-5, g_ray=5e-4), E(1, 2, 3, 2, 0, 1, 1, 1.0, 64.0, 2.0))],
        gtol=1e-3),
    Row("gtol_off", 256.0, [(T(128.0, 256.0, g_pose=0.0, g_ray=0.0), E(1, 1, 2, 1, 0, 0, 0, 1.0, 128.0, 2.0))]),
    # ---- xtol: |dx| = 1e-7 > 1e-8 (1e-8 + 1) goes on, |dx| = 1e-10 stops; then the order ftol, xtol, gtol, max_iter
    Row("xtol", 256.0, [(T(128.0, 256.0, dx2=1e-14), E(1, 1, 2, 1, 0, 0, 0, 1.0, 128.0, 2.0)),
                        (T(64.0, 128.0, dx2=1e-20), E(1, 2, 3, 2, 0, 3, 1, 1.0, 64.0, 2.0))]),
    Row("ftol_before_xtol", 64.0, [(T(C, 2.0 ** -29, dx2=1e-20), E(1, 1, 2, 1, 0, 2, 1, 1.0, C, 2.0))]),
    Row("xtol_before_gtol", 256.0, [(T(128.0, 256.0, dx2=1e-20, g_pose=1e-4, g_ray=1e-4),
                                     E(1, 1, 2, 1, 0, 3, 1, 1.0, 128.0, 2.0))], gtol=1e-3),
    Row("gtol_before_max_iter", 256.0, [(T(128.0, 256.0, g_pose=1e-4, g_ray=1e-4),
                                         E(1, 1, 2, 1, 0, 1, 1, 1.0, 128.0, 2.0))], gtol=1e-3, max_iter=1),
    Row("max_iter", 256.0, [(OK, E(1, 1, 2, 1, 0, 0, 0, 1.0, 128.0, 2.0)),
                            (T(64.0, 128.0), E(1, 2, 3, 2, 0, 0, 1, 1.0, 64.0, 2.0))], max_iter=2),
    # ---- the exits of a rejection: DAMPING is lambda > max_lambda (8 is not above 8), FAILED is max_retries in a row
    Row("failed", 256.0, [(BAD, E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0)),
                          (BAD, E(0, 0, 3, 2, 2, 0, 0, 8.0, 256.0, 8.0)),
                          (BAD, E(0, 0, 4, 3, 3, -1, 1, 64.0, 256.0, 16.0))], max_retries=3),
    Row("damping", 256.0, [(BAD, E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0)),
                           (BAD, E(0, 0, 3, 2, 2, 5, 1, 8.0, 256.0, 8.0))], max_lambda=5.0),
    Row("damping_bound_is_strict", 256.0, [(BAD, E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0)),
                                           (BAD, E(0, 0, 3, 2, 2, 0, 0, 8.0, 256.0, 8.0)),
                                           (BAD, E(0, 0, 4, 3, 3, 5, 1, 64.0, 256.0, 16.0))], max_lambda=8.0),
    # the tie: the rejection that reaches max_retries also pushes lambda past max_lambda -- DAMPING
    Row("tie_damping_over_failed", 256.0, [(BAD, E(0, 0, 2, 1, 1, 0, 0, 2.0, 256.0, 4.0)),
                                           (BAD, E(0, 0, 3, 2, 2, 0, 0, 8.0, 256.0, 8.0)),
                                           (BAD, E(0, 0, 4, 3, 3, 5, 1, 64.0, 256.0, 16.0))],
        max_lambda=10.0, max_retries=3),
    Row("tie_from_gauss_newton", 256.0, [(T(257.0, 256.0), E(0, 0, 2, 1, 1, 0, 0, 1e-9, 256.0, 4.0)),
                                         (T(257.0, 256.0), E(0, 0, 3, 2, 2, 5, 1, 4e-9, 256.0, 8.0))],
        gauss_newton=True, max_lambda=2e-9, max_retries=2),
    # ---- a decision after the final one changes nothing
    Row("decide_after_done", 256.0, [(OK, E(1, 1, 2, 1, 0, 0, 1, 1.0, 128.0, 2.0)),
                                     (T(64.0, 128.0), E(0, 1, 2, 1, 0, 0, 1, 1.0, 128.0, 2.0))], max_iter=1),
]


def scalars8(step, cost):
    """A table step as the eight scalars a handle's read_scalars returns."""
    return np.array([cost, step["new"], step["pred"], step["dx2"], step["x2"], float(step["info"]),
                     max(step["g_pose"], step["g_ray"]), 0.0])


class ScriptedHandle:
    """The host-step protocol over a scripted scalar sequence (a table row's steps): trial k reads step k, an
    accepted trial's cost becomes the current one.  Past its end the script serves a non-finite trial cost, so that
    any loop driving it comes to an end through rejections.  `lams` records the damping of every build."""

    def __init__(self, cost0, steps):
        self.cost0, self.steps = float(cost0), list(steps)
        self.linearize()

    def linearize(self):
        self.cost, self.k, self.lams = self.cost0, -1, []

    def build_reduced(self, lam):
        self.lams.append(float(lam))

    def solve_reduced(self):
        self.k += 1

    def read_scalars(self):
        if self.k < 0:
            return np.array([self.cost, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        return scalars8(self.steps[self.k] if self.k < len(self.steps) else T(NAN, 1.0), self.cost)

    def accept(self, ok):
        if ok:
            self.cost = self.steps[self.k]["new"]

    def sync(self):
        pass


# -------------------------------------------------------------------------------------------------
# real trajectories
# -------------------------------------------------------------------------------------------------
# each with ftol = 1e-10, xtol = 1e-12 unless it says otherwise
SCENARIOS = {
    "recover": dict(gauss_newton=True, max_iter=5),                       # rejections, then recovery
    "failed": dict(gauss_newton=True, max_retries=3),                     # FAILED
    "damping": dict(gauss_newton=True, max_lambda=1e-4),                  # DAMPING
    "tie": dict(gauss_newton=True, max_lambda=1e-4, max_retries=6),       # both at once: DAMPING
    "max_iter": dict(lambda0=1e-4, max_iter=3),                           # MAX_ITER after rejections
    "ftol": dict(lambda0=1e-4, ftol=1e-2),                                # FTOL
    "xtol": dict(lambda0=1e-4, xtol=1e-3, ftol=0.0),                      # XTOL
    "gtol": dict(lambda0=1e-4, gtol=1e3, ftol=0.0, xtol=0.0),             # GTOL
    "floor": dict(lambda0=10.0, min_lambda=1.0, max_iter=6),              # the min_lambda floor
}
EXPECTED_STATUS = {"recover": lm_ref.MAX_ITER, "failed": lm_ref.FAILED, "damping": lm_ref.DAMPING,
                   "tie": lm_ref.DAMPING, "max_iter": lm_ref.MAX_ITER, "ftol": lm_ref.FTOL, "xtol": lm_ref.XTOL,
                   "gtol": lm_ref.GTOL, "floor": lm_ref.MAX_ITER}


def scenario_opts(name):
    kw = dict(ftol=1e-10, xtol=1e-12)
    kw.update(SCENARIOS[name])
    return lm_ref.Opts(**kw)


@functools.lru_cache(maxsize=None)
def problem():
    import synthetic
    return synthetic.make_small_problem(12, 150, -8.0, 8.0, seed=1)


def far_start():
    """The poses the scenarios start from: the problem's initial poses, the free ones moved by 60 times a normal draw
    of sigma (0.3, 0.2, 30) -- the fourth (11, 3) draw of default_rng(0).  From here a Gauss-Newton run accepts
    once, rejects seven times in a row and then recovers."""
    p = problem()
    rng = np.random.default_rng(0)
    for _ in range(3):
        rng.normal(0, 1, (11, 3))
    far = p.init_ptz.copy()
    far[1:] += rng.normal(0, 1, (11, 3)) * [0.3, 0.2, 30.0] * 60
    return far


def numpy_handle():
    from numpy_handle import NumpyBAHandle
    p = problem()
    h = NumpyBAHandle()
    h.set_problem(p.n_pose, p.n_landmark, p.frame, p.landmark, p.xy, p.u, p.v)
    h.set_state(far_start(), p.init_rays)
    return h


@functools.lru_cache(maxsize=None)
def reference(name):
    """(records, final (ptz, rays)) of the reference's run of a scenario on the dense fp64 numpy handle.  Shared:
    do not modify."""
    h = numpy_handle()
    recs = lm_ref.run(h, scenario_opts(name))
    return recs, h.get_state()


def check_reference_margins(recs, opts):
    """What a compared window needs so that rounding cannot flip a decision silently, asserted on the reference alone:
    every decision has |rho| >= 0.1; every termination comparison reachable at an accepted trial differs from its
    threshold by at least a factor of 2 (the rho > 1/4 half of the ftol test included, where its other half holds);
    every accepted trial reduces the cost by at least 1e-3 of it."""
    def apart(a, b):
        assert a >= 0 and b >= 0 and (a >= 2 * b or b >= 2 * a), (a, b)

    for r in recs:
        assert abs(r.rho) >= 0.1, r
        if not r.accepted:
            continue
        assert r.actual >= 1e-3 * r.old_cost, r
        dx, x, gmax = math.sqrt(r.scalars[3]), math.sqrt(r.scalars[4]), r.scalars[6]
        if opts.ftol > 0:
            apart(r.actual, opts.ftol * r.old_cost)
            if r.actual < opts.ftol * r.old_cost:
                apart(r.rho, 0.25)
        if r.status == lm_ref.FTOL:
            continue
        if opts.xtol > 0:
            apart(dx, opts.xtol * (opts.xtol + x))
        if r.status == lm_ref.XTOL:
            continue
        if opts.gtol > 0:
            apart(gmax, opts.gtol)


def lam_gates(recs, opts):
    """Per decision of the reference's run, (relative gate on lambda's value, whether the update is an exact product).

    Where the factor depends on rho -- an accepted trial above the 1/3 floor -- the gate is 20 * 1e-7 * cost / actual:
    the factor's derivative in rho is <= 12 for rho <= 1.2, and rho = actual / pred moves by cost / actual for every
    relative unit the cost moves (the 1e-7 step gate).  Where lambda does not depend on the lambda before it -- the
    min_lambda floor, a GN run's untouched zero, 1e-9 after a rejection from (near) zero -- it is exact: 1e-12.
    Elsewhere the update is one product by a constant (nu after a rejection, 1/3 at the factor's floor): the quotient
    lambda / previous lambda is exact to 1e-12, while the value carries the previous lambda's relative deviation
    unchanged, so its gate is the previous one plus 1e-12."""
    out, prev = [], 1e-12
    for r in recs:
        pinned = r.lam == opts.min_lambda or r.old_lam == 0.0 or (not r.accepted and r.lam == 1e-9)
        product = not r.accepted or (r.factor is not None and r.factor <= THIRD)
        if pinned:
            g, product = 1e-12, False
        elif product:
            g = prev + 1e-12
        else:
            g = 20.0 * 1e-7 * r.old_cost / r.actual
        out.append((g, product))
        prev = g
    return out
