"""Test infrastructure: the Levenberg-Marquardt decision rules as a plain state machine, written from
include/ptzba.h (ptzba_lm_opts, the PTZBA_STATUS_* comment, ptzba_lm_record) and scipy's trf acceptance and
check_termination rules (scipy/optimize/_lsq/common.py).  It is the independent statement that the four loops of
the product (the device decision, stand-alone and fused; ptzba_solve's C driver; ptzba.LMSolver's host and device
drivers) are compared with; it imports nothing of them.  Linear loss only: the curvature switch of the robust
losses is not restated here.  Never used by the product.

One decision, from the state before it and the scalars of the trial:

  ok     = info == 0 and the trial cost and pred are finite
  actual = cost - trial cost;  rho = actual / pred if ok and pred > 0, else -1
  accept = ok and (rho > 0, or a Gauss-Newton run whose lambda is still 0 and actual >= 0)
  accept:  lambda = max(min_lambda, lambda * max(1/3, 1 - (2 rho - 1)^3)), untouched while a GN run has lambda == 0;
           nu = 2, retries = 0, iterations += 1, cost = trial cost; then, in this order,
           FTOL  actual < ftol * old cost and rho > 0.25
           XTOL  sqrt(|dx|^2) < xtol * (xtol + sqrt(|x|^2))
           GTOL  gtol > 0 and max |g| < gtol
           MAX_ITER  iterations >= max_iter
  reject:  lambda = max(lambda * nu, 1e-9), or 1e-9 from zero; nu *= 2, retries += 1; then
           DAMPING  lambda > max_lambda         (first: it wins a tie with FAILED)
           FAILED   retries >= max_retries
  nfev and trials count every decision.  A decision after `done` changes nothing (accepted = 0)."""
import math

FAILED, MAX_ITER, GTOL, FTOL, XTOL, DAMPING = -1, 0, 1, 2, 3, 5

RECORD_FIELDS = ("cost", "initial_cost", "lam", "iterations", "nfev", "trials", "retries", "status", "done",
                 "accepted")
DISCRETE_FIELDS = ("accepted", "iterations", "nfev", "trials", "retries", "status", "done")


class Opts:
    """ptzba_lm_opts without the two robust-loss fields; the defaults are the header's."""

    def __init__(self, ftol=1e-4, xtol=1e-8, gtol=0.0, lambda0=1e-12, min_lambda=1e-12, max_lambda=1e16,
                 max_iter=100, max_retries=30, gauss_newton=False):
        self.ftol, self.xtol, self.gtol = float(ftol), float(xtol), float(gtol)
        self.lambda0 = 0.0 if gauss_newton else float(lambda0)  # (header: gauss_newton = lambda0 0)
        self.min_lambda, self.max_lambda = float(min_lambda), float(max_lambda)
        self.max_iter, self.max_retries = int(max_iter), int(max_retries)
        self.gauss_newton = bool(gauss_newton)

    def solver_kwargs(self):
        """The same options under the keyword names of ptzba.LMSolver / BAHandle.solve / solve_resident."""
        return dict(ftol=self.ftol, xtol=self.xtol, gtol=self.gtol, lambda0=self.lambda0, min_lambda=self.min_lambda,
                    max_lambda=self.max_lambda, max_iter=self.max_iter, max_retries=self.max_retries,
                    gauss_newton=self.gauss_newton)


class State:
    """The fields of ptzba_lm_record plus nu.  A decision also leaves what it was taken from, for the tests' margins
    (never compared with a loop): rho, actual, pred, old_cost, old_lam, factor (the accepted lambda factor before the
    1/3 floor; None on a rejection), scalars (the eight read)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def copy(self):
        return State(**self.__dict__)

    def record(self):
        return {k: getattr(self, k) for k in RECORD_FIELDS}

    def __repr__(self):
        return "State(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in RECORD_FIELDS + ("nu",)) + ")"


def start(cost, opts):
    """The state before the first trial (ptzba_lm_init at a point whose cost is `cost`)."""
    return State(cost=float(cost), initial_cost=float(cost), lam=opts.lambda0, iterations=0, nfev=1, trials=0,
                 retries=0, status=MAX_ITER, done=0, accepted=0, nu=2.0, rho=None, actual=None, pred=None,
                 old_cost=None, old_lam=None, factor=None, scalars=None)


def decide(state, scalars, opts):
    """One decision: `scalars` are the eight read out after a trial (current cost, trial cost, pred, |dx|^2, |x|^2,
    info, max |g|, unused).  The current cost is the state's own (scalars[0] repeats it).  Returns the new state."""
    s = state.copy()
    s.accepted = 0
    if s.done:
        return s
    new_cost, pred, dx2, x2, info, gmax = (float(scalars[k]) for k in range(1, 7))
    s.scalars = [float(v) for v in scalars]
    s.nfev += 1
    s.trials += 1
    ok = info == 0.0 and math.isfinite(new_cost) and math.isfinite(pred)
    actual = s.cost - new_cost
    rho = actual / pred if (ok and pred > 0.0) else -1.0
    gn0 = opts.gauss_newton and s.lam == 0.0
    s.rho, s.actual, s.pred, s.old_cost, s.old_lam, s.factor = rho, actual, pred, s.cost, s.lam, None
    if ok and (rho > 0.0 or (gn0 and actual >= 0.0)):
        s.accepted = 1
        if not gn0:
            t = 2.0 * rho - 1.0
            s.factor = 1.0 - t * t * t
            s.lam = max(opts.min_lambda, s.lam * max(1.0 / 3.0, s.factor))
        s.nu = 2.0
        s.retries = 0
        s.iterations += 1
        old = s.cost
        s.cost = new_cost
        if actual < opts.ftol * old and rho > 0.25:
            s.status, s.done = FTOL, 1
        elif math.sqrt(dx2) < opts.xtol * (opts.xtol + math.sqrt(x2)):
            s.status, s.done = XTOL, 1
        elif opts.gtol > 0.0 and gmax < opts.gtol:
            s.status, s.done = GTOL, 1
        elif s.iterations >= opts.max_iter:
            s.status, s.done = MAX_ITER, 1
    else:
        s.lam = max(s.lam * s.nu, 1e-9) if s.lam > 0.0 else 1e-9
        s.nu *= 2.0
        s.retries += 1
        if s.lam > opts.max_lambda:
            s.status, s.done = DAMPING, 1
        elif s.retries >= opts.max_retries:
            s.status, s.done = FAILED, 1
    return s


def run(handle, opts):
    """Drive a handle of the host-step protocol (linearize, build_reduced, solve_reduced, read_scalars, accept) from
    its current state to termination.  Returns one State per trial (none for max_iter <= 0).  A non-finite start
    raises ValueError, as scipy's least_squares does."""
    handle.linearize()
    cost = float(handle.read_scalars()[0])
    if not math.isfinite(cost):
        raise ValueError("Residuals are not finite in the initial point.")
    s = start(cost, opts)
    recs = []
    if opts.max_iter <= 0:
        return recs
    while not s.done:
        handle.build_reduced(s.lam)
        handle.solve_reduced()
        s = decide(s, handle.read_scalars(), opts)
        handle.accept(bool(s.accepted))
        recs.append(s)
    return recs
