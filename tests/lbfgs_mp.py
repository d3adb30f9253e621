"""A multiprecision reference of the L-BFGS step that knows its own margins (TEST INFRASTRUCTURE ONLY).

`run()` restates lbfgs_optimize and line_search_lewisoverton (lbfgs.hpp:276-384, 434-717) once more, grown out of the
pure-Python restatement behind tests/golden/lbfgs_traces.json (tests/golden/make_lbfgs_traces.py: independent of the C
port oracle/lbfgs_oracle.c), and parameterised on its arithmetic:

    "mp"    mpmath at 50 digits (dot products, the two-loop recursion, every threshold, the objective),
    "f64"   float64 with dot products summed left to right,
    "fsum"  float64 with exactly rounded dot products (math.fsum).

It adds what the kernels add to the reference's loop: the built-in step bound (variables i >= bound_from may not fall
below bound_min within a line search: lbfgs.hpp:557-565 with step_bound_ratio / ls_bound_step of lbfgs_step.h), the
cancel word (non-zero: LBFGS_CANCELED after the first accepted step) and an evaluation budget (LBFGS_RUNNING with exactly
max_evals evaluations).  Where the kernels round on purpose, every mode rounds: the trial point xp + step d is a float64
product and a float64 sum (trial_point in lbfgs_step.h), so the mp mode evaluates its 50-digit objective AT that float64
point; the value of the step bound is a float64 too (the reference's proc_stepbound returns a double), overflow to
infinity included -- that overflow is how a bounded search reaches LBFGSERR_INVALIDPARAMETERS.

Every comparison that decides a branch records its relative margin |lhs - rhs| / max(|lhs|, |rhs|, 1e-300): Armijo,
curvature, the three step tests (min, max, width), g_epsilon, past / delta, the cautious update, `step > 0` and
`dginit > 0` at the entry of a search, and the choice `step < step_max` of a bounded search.  isnan / isinf has no margin.
(`step > 0` can only fail on a step of exactly 0.0 -- half a bound that is one over an overflowed ratio; what is recorded
there is the margin of the overflow, the ratio's exact value against the largest double.)
A run returns (status, k, evals, x, f, min_margin, which_test) and two counters: skipped cautious updates, and uses of the
max_step second chance (`touched`) that did not end the search.

`select_cases()` is the condition that replaces "a few problems may differ": a case is kept only when the mp run, the f64
run and the fsum run return the same (status, k, evals) and the smallest margin of the mp run is at least MIN_MARGIN = 1e-6
-- stated, not measured: many orders above what reordering a float64 sum of n <= 129 terms can move (n * 2^-53 ~ 1.4e-14)
through at most 12 iterations, and far below the margins the designed families have (piecewise-linear families on dyadic
data decide on exactly representable numbers).  A kept case is compared EXACTLY in its counters with every kernel form.

Objective families are written once, as a description (a dict of per-variable coefficient arrays: DESC_FIELDS), with
two evaluators on top: `evaluate()` in the run's arithmetic and `TorchBatch` for the device callback, where every column
of a batch has its own description.  A family's special coordinates sit at seeded positions that always include n - 1; all
other coordinates carry a separable quadratic with dyadic weights and shifts, so every lane (and with two variables per
lane both of them) enters every dot product.

Which family takes which exit (with margin, at every shape of SHAPES):
     0     `quadratic`, `stationary` (k = 0, one evaluation), `flat_then_curved`      1    `quadratic_offset`, `abs` under "past2"
    -1006  `floor_zero` (bounded: the bound is exactly 0)                              -1007  `cliff` under "wide_prec"
    -1008  `rosenbrock`, `nonsmooth`                                                   -1009  `linear`, `abs`, `cliff` under "tight"
    -1010  `linear` under "max_step" and "bounded"                                     -1011  `floor_near` under "bounded_tight"
    -1012  `nan_wall`, `inf_wall` (at evaluation 2, in the middle of a batch)
    2 / RUNNING  every family under the modes "cancel" / "budget"
    a skipped cautious update and an accepted max_step second chance: `flat_then_curved` (under "max_step" both at once)
(`abs` with min_step = 1e-3 alone needs more than the 12 iterations a case may run to reach -1011; the bounded search
of `floor_near` reaches the same test of the same code at its first bisection.)

Codes no family reaches (the "all codes" assertion of tests/test_lbfgs_mp_cpu.py lists exactly the reached ones):
    -1005 LBFGSERR_INCREASEGRADIENT cannot occur in exact arithmetic: every stored pair has y.s > 0 (the cautious test), so
          the two-loop matrix is positive definite and d is a descent direction; with a gradient that lies it can, but that
          is a statement about the lie, not the step, and is not forced here.
    -1007 LBFGSERR_WIDTHTOOSMALL IS reached, by the `cliff` family under the parameter set "wide_prec" (machine_prec = 1/4):
          at the default 1e-16 a bracket halves 53 times before it closes while max_linesearch = 64 trials also pay for the
          doublings in front of it, and at float64 the midpoint stops moving first; with the coarse machine_prec the bracket
          [0.5, 0.75] -> [0.625, 0.75] closes on the fourth trial with margin 1/3.
"""
import functools
import math

import mpmath
import numpy as np

CONVERGENCE, STOP, CANCELED = 0, 1, 2
ERR_INVALID_FUNCVAL, ERR_MINIMUMSTEP, ERR_MAXIMUMSTEP, ERR_MAXIMUMLINESEARCH = -1012, -1011, -1010, -1009
ERR_MAXIMUMITERATION, ERR_WIDTHTOOSMALL, ERR_INVALIDPARAMETERS, ERR_INCREASEGRADIENT = -1008, -1007, -1006, -1005
RUNNING = 2147483647

DEFAULTS = dict(mem_size=8, g_epsilon=1.0e-5, past=3, delta=1.0e-6, max_iterations=0, max_linesearch=64,
                min_step=1.0e-20, max_step=1.0e+20, f_dec_coeff=1.0e-4, s_curv_coeff=0.9, cautious_factor=1.0e-6,
                machine_prec=1.0e-16)          # lbfgs.hpp:25-128
MIN_MARGIN = 1.0e-6
DBL_MAX = 1.7976931348623157e308

_MP = mpmath.mp.clone()
_MP.dps = 50


class _F64:
    name = "f64"
    num = staticmethod(float)
    sqrt = staticmethod(math.sqrt)

    @staticmethod
    def dot(a, b):
        acc = 0.0
        for u, v in zip(a, b):
            acc += u * v
        return acc

    @staticmethod
    def total(a):
        acc = 0.0
        for u in a:
            acc += u
        return acc

    @staticmethod
    def bad(f):
        return math.isinf(f) or math.isnan(f)


class _Fsum(_F64):
    name = "fsum"

    @staticmethod
    def dot(a, b):
        return math.fsum(u * v for u, v in zip(a, b))

    total = staticmethod(math.fsum)


class _Mp:
    name = "mp"
    num = staticmethod(_MP.mpf)
    sqrt = staticmethod(_MP.sqrt)

    @staticmethod
    def dot(a, b):
        return _MP.fdot(a, b)

    @staticmethod
    def total(a):
        return _MP.fsum(a)

    @staticmethod
    def bad(f):
        return bool(_MP.isinf(f) or _MP.isnan(f))


ARITH = {"mp": _Mp, "f64": _F64, "fsum": _Fsum}


# ---- objective descriptions ----------------------------------------------------------------------------------------
# f(x) = const + sum_i [ qw_i (x_i - qs_i)^2 / 2 + lin_i x_i + ac_i |x_i - as_i| + ch_i [x_i > ct_i] + ftc_i phi(x_i) ]
#        + rosen * sum_i (100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2),          and f = bad where any x_i > bt_i with bm_i set;
# the gradient of |.| is +ac where x_i > as_i and -ac otherwise (as the traces' `nonsmooth` has it), a cliff and a wall
# have none, ftc_i is a weight, phi(t) = -t below FTC_X0 and -FTC_X0 - u / 2 + FTC_Q u^2 / 2 with u = t - FTC_X0 above.
DESC_FIELDS = ("qw", "qs", "lin", "ac", "as", "ch", "ct", "ftc", "bm", "bt")
FTC_X0, FTC_Q = 786432.0, 2.0 ** -20           # 1.5 * 2^19: the doubling steps 2^19 -> 2^20 jump across it


def _blank(n):
    d = {k: np.zeros(n) for k in DESC_FIELDS}
    d.update(n=n, const=0.0, rosen=0.0, bad=0.0, x0=np.zeros(n))
    return d


def evaluate(desc, x, ar):
    """f and g of a description at the float64 point x, in the arithmetic `ar`."""
    N = ar.num
    n = desc["n"]
    xs = [N(float(v)) for v in x]
    terms = [N(desc["const"])]
    g = [N(0.0)] * n
    hit = False
    qw, qs, lin, ac, as_, ch, ct, ftc, bm, bt = (desc[k] for k in DESC_FIELDS)
    for i in range(n):
        xi = xs[i]
        gi = N(0.0)
        if qw[i] != 0.0:
            r = xi - N(qs[i])
            terms.append(N(0.5 * qw[i]) * r * r)
            gi = gi + N(qw[i]) * r
        if lin[i] != 0.0:
            terms.append(N(lin[i]) * xi)
            gi = gi + N(lin[i])
        if ac[i] != 0.0:
            terms.append(N(ac[i]) * abs(xi - N(as_[i])))
            gi = gi + (N(ac[i]) if x[i] > as_[i] else -N(ac[i]))
        if ch[i] != 0.0 and x[i] > ct[i]:
            terms.append(N(ch[i]))
        if ftc[i] != 0.0:
            c = N(ftc[i])
            if x[i] < FTC_X0:
                terms.append(-c * xi)
                gi = gi - c
            else:
                u = xi - N(FTC_X0)
                terms.append(c * (-N(FTC_X0) - N(0.5) * u + N(0.5 * FTC_Q) * u * u))
                gi = gi + c * (-N(0.5) + N(FTC_Q) * u)
        if bm[i] != 0.0 and x[i] > bt[i]:
            hit = True
        g[i] = gi
    if desc["rosen"]:
        for i in range(n - 1):
            a, b = xs[i + 1] - xs[i] * xs[i], N(1.0) - xs[i]
            terms.append(N(100.0) * a * a + b * b)
            g[i] = g[i] + N(-400.0) * a * xs[i] - N(2.0) * b
            g[i + 1] = g[i + 1] + N(200.0) * a
    f = ar.total(terms)
    if hit:
        f = N(desc["bad"])
    return f, g


class TorchBatch:
    """The same objective for the device callback: column b of the batch evaluates descs[b]; columns past the batch are NaN."""

    def __init__(self, descs, ld, device):
        import torch
        self.torch = torch
        n, B = descs[0]["n"], len(descs)
        self.n, self.B = n, B

        def col(key):
            a = np.zeros((n, ld))
            for b, d in enumerate(descs):
                a[:, b] = d[key]
            return torch.from_numpy(a).to(device)
        self.t = {k: col(k) for k in DESC_FIELDS}
        row = lambda key: torch.from_numpy(np.array([d[key] for d in descs] + [0.0] * (ld - B))).to(device)
        self.const, self.rosen, self.bad = row("const"), row("rosen"), row("bad")
        self.x0 = col("x0")

    def __call__(self, x, f, g):
        torch, t = self.torch, self.t
        r = x - t["qs"]
        up = x > t["as"]
        fv = 0.5 * t["qw"] * r * r + t["lin"] * x + t["ac"] * (x - t["as"]).abs() + t["ch"] * (x > t["ct"])
        gv = t["qw"] * r + t["lin"] + torch.where(up, t["ac"], -t["ac"])
        u = x - FTC_X0
        low = x < FTC_X0
        fv = fv + t["ftc"] * torch.where(low, -x, -FTC_X0 - 0.5 * u + (0.5 * FTC_Q) * u * u)
        gv = gv + t["ftc"] * torch.where(low, torch.full_like(x, -1.0), -0.5 + FTC_Q * u)
        ftot = self.const + fv.sum(dim=0)
        if self.n > 1:
            a, b = x[:-1], x[1:]
            tt = b - a * a
            ftot = ftot + self.rosen * (100.0 * tt * tt + (1.0 - a) ** 2).sum(dim=0)
            gv[:-1] += self.rosen * (-400.0 * a * tt - 2.0 * (1.0 - a))
            gv[1:] += self.rosen * (200.0 * tt)
        hit = ((x > t["bt"]) & (t["bm"] != 0.0)).any(dim=0)
        f.copy_(torch.where(hit, self.bad, ftot))
        g.copy_(gv)
        f[self.B:] = float("nan")
        g[:, self.B:] = float("nan")


# ---- the restatement -----------------------------------------------------------------------------------------------
class _Margins:
    def __init__(self):
        self.min, self.which = math.inf, None

    def note(self, name, lhs, rhs):
        lhs, rhs = float(lhs), float(rhs)
        if math.isinf(lhs) or math.isinf(rhs):
            m = 1.0 if lhs != rhs else 0.0
        else:
            m = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)
        if m < self.min:
            self.min, self.which = m, name


class _Budget(Exception):
    pass


class Result(dict):
    __getattr__ = dict.__getitem__

    @property
    def counters(self):
        return (self["status"], self["k"], self["evals"])


def _inf_norm(a):
    return max(abs(v) for v in a)


def step_bound(xp, d, bound_from, bound_min):
    """The built-in bound as a float64, the way a proc_stepbound callback returns it (and the kernels compute it), and the
    exact value of the largest ratio -d_i / max(x_i - xmin, 1e-300) it is one over."""
    worst, exact = 0.0, _MP.mpf(0)
    for i in range(bound_from, len(xp)):
        di = float(d[i])
        if di < 0.0:
            room = float(xp[i]) - bound_min
            room = room if room > 1e-300 else 1e-300
            with np.errstate(over="ignore"):
                worst = max(worst, float(np.float64(-di) / np.float64(room)))
            exact = max(exact, _MP.mpf(-di) / _MP.mpf(room))
    return (1.0 / worst if worst > 0.0 else math.inf), exact


def run(desc, mode="mp", bound=None, cancel=0, max_evals=None, x0=None, **over):
    """lbfgs.hpp:434-717 on `desc` -- a description, or a callable (x, arithmetic) -> (f, g) with the start point in x0.
    bound: (bound_from, bound_min) or None.  Returns a Result."""
    ar = ARITH[mode]
    N = ar.num
    prm = dict(DEFAULTS, **over)
    mg = _Margins()
    st = dict(evals=0, skipped=0, second_chance=0)

    def fun(x):
        if max_evals is not None and st["evals"] >= max_evals:
            raise _Budget
        st["evals"] += 1
        return desc(x, ar) if callable(desc) else evaluate(desc, x, ar)

    def trial(xp, step, d):          # two float64 roundings (trial_point in lbfgs_step.h)
        if mode == "mp":
            return [a + float(step * b) for a, b in zip(xp, d)]
        return [a + step * b for a, b in zip(xp, d)]

    def converged(g, x):
        lhs = _inf_norm(g) / max(N(1.0), N(_inf_norm(x)))
        mg.note("g_epsilon", lhs, prm["g_epsilon"])
        return lhs < N(prm["g_epsilon"])

    def search(xp, gp, fx, d, step):
        """lbfgs.hpp:276-384 behind the bound of :557-565.  Returns (code_or_count, x, f, g, step)."""
        smax = N(prm["max_step"])
        if bound is not None:
            bnd, ratio = step_bound(xp, d, *bound)
            bnd = N(bnd)
            smax = bnd if bnd < smax else smax
            mg.note("bound_step", step, smax)
            step = step if step < smax else N(0.5) * smax
            if bnd == 0:
                # a bound of exactly 0 is no near tie of `step > 0`: it is one over a ratio that overflowed float64, and the
                # margin of that decision is the ratio's distance to the largest double
                mg.note("bound_overflow", ratio / _MP.mpf(DBL_MAX), 1.0)
        if step != 0:
            mg.note("step_positive", step, 0.0)
        if not step > 0:
            return ERR_INVALIDPARAMETERS, xp, fx, gp, step
        slope0 = ar.dot(gp, d)
        mg.note("dginit", slope0, 0.0)
        if slope0 > 0:
            return ERR_INCREASEGRADIENT, xp, fx, gp, step
        armijo, wolfe = N(prm["f_dec_coeff"]) * slope0, N(prm["s_curv_coeff"]) * slope0
        lo, hi = N(0.0), smax
        bracketed = tried_max = False
        trials = 0
        while True:
            x = trial(xp, step, d)
            f, g = fun(x)
            trials += 1
            if ar.bad(f):
                return ERR_INVALID_FUNCVAL, x, f, g, step
            rhs = fx + step * armijo
            mg.note("armijo", f, rhs)
            if f > rhs:
                hi, bracketed = step, True
            else:
                dg = ar.dot(g, d)
                mg.note("curvature", dg, wolfe)
                if dg < wolfe:
                    lo = step
                else:
                    return trials, x, f, g, step
            if prm["max_linesearch"] <= trials:
                return ERR_MAXIMUMLINESEARCH, x, f, g, step
            if bracketed:
                mg.note("width", hi - lo, N(prm["machine_prec"]) * hi)
                if (hi - lo) < N(prm["machine_prec"]) * hi:
                    return ERR_WIDTHTOOSMALL, x, f, g, step
            step = N(0.5) * (lo + hi) if bracketed else N(2.0) * step
            mg.note("min_step", step, prm["min_step"])
            if step < N(prm["min_step"]):
                return ERR_MINIMUMSTEP, x, f, g, step
            mg.note("max_step", step, smax)
            if step > smax:
                if tried_max:
                    return ERR_MAXIMUMSTEP, x, f, g, step
                tried_max, step = True, smax
                st["pending_chance"] = True

    def out(status, k, x, f):
        return Result(status=status, k=k, evals=st["evals"], x=np.array([float(v) for v in x]), f=float(f),
                      min_margin=mg.min, which=mg.which, skipped=st["skipped"], second_chance=st["second_chance"])

    x = [float(v) for v in (desc["x0"] if x0 is None else x0)]
    k = 0
    fx = N(0.0)
    try:
        fx, g = fun(x)
        past = prm["past"]
        recent = [fx] + [N(0.0)] * (max(1, past) - 1)
        d = [-v for v in g]
        if converged(g, x):
            return out(CONVERGENCE, k, x, fx)
        step = N(1.0) / ar.sqrt(ar.dot(d, d))
        k = 1
        pairs = []                      # newest first: (s, y, y.s)
        while True:
            xp, gp = x, g
            st["pending_chance"] = False
            ls, x, f_trial, g, step = search(xp, gp, fx, d, step)
            if ls < 0:
                # the point is reverted, the reported value is the last trial's (lbfgs.hpp:570-577)
                return out(ls, k, xp, f_trial)
            if st["pending_chance"]:
                st["second_chance"] += 1
            fx = f_trial
            if cancel:
                return out(CANCELED, k, x, fx)
            if converged(g, x):
                return out(CONVERGENCE, k, x, fx)
            if past > 0:
                slot = k % past
                if past <= k:
                    rate = abs(recent[slot] - fx) / max(N(1.0), abs(fx))
                    mg.note("past_delta", rate, prm["delta"])
                    if rate < N(prm["delta"]):
                        return out(STOP, k, x, fx)
                recent[slot] = fx
            if prm["max_iterations"] != 0 and prm["max_iterations"] <= k:
                return out(ERR_MAXIMUMITERATION, k, x, fx)
            k += 1
            s = [N(a) - N(b) for a, b in zip(x, xp)]
            y = [a - b for a, b in zip(g, gp)]
            ys, yy = ar.dot(y, s), ar.dot(y, y)
            d = [-v for v in g]
            cau = ar.dot(s, s) * ar.sqrt(ar.dot(gp, gp)) * N(prm["cautious_factor"])
            mg.note("cautious", ys, cau)
            if ys > cau:
                pairs.insert(0, (s, y, ys))
                del pairs[prm["mem_size"]:]
                alphas = []
                for (sj, yj, ysj) in pairs:                       # newest to oldest
                    a = ar.dot(sj, d) / ysj
                    alphas.append(a)
                    d = [u + (-a) * v for u, v in zip(d, yj)]
                scale = ys / yy
                d = [u * scale for u in d]
                for (sj, yj, ysj), a in zip(reversed(pairs), reversed(alphas)):   # oldest to newest
                    b = ar.dot(yj, d) / ysj
                    d = [u + (a - b) * v for u, v in zip(d, sj)]
            else:
                st["skipped"] += 1
            step = N(1.0)
    except _Budget:
        return out(RUNNING, k, x, fx)


# ---- families --------------------------------------------------------------------------------------------------------
FAMILIES = ("quadratic", "quadratic_offset", "stationary", "rosenbrock", "nonsmooth", "linear", "abs", "nan_wall", "inf_wall",
            "cliff", "floor_zero", "floor_near", "flat_then_curved")
BOUND_MIN = -1.75                     # the floor of the bounded parameter sets


def _specials(rng, n, count):
    """Seeded positions of a family's special coordinates; the first is always n - 1."""
    rest = [int(i) for i in rng.permutation(n - 1)[:max(0, min(count - 1, n - 1))]]
    return [n - 1] + rest


def make_case(family, n, seed=0):
    """The description of one member of a family with n variables (deterministic in (family, n, seed))."""
    rng = np.random.default_rng([FAMILIES.index(family), n, seed])
    d = _blank(n)
    sp = _specials(rng, n, 2)
    a, b = sp[0], sp[-1]                                   # (n = 1: both are variable 0)
    dy = lambda lo, hi, den: rng.integers(lo * den, hi * den + 1, size=n) / float(den)     # dyadic numbers
    smooth = family in ("quadratic", "quadratic_offset", "stationary", "nan_wall", "inf_wall")
    # the bowl under the piecewise-linear families is small (2^-14): it puts every lane into every dot product without
    # bending a search that runs out to step 10^3 (its curvature times the step stays below 1/4)
    scale = 1.0 if smooth or family in ("rosenbrock", "nonsmooth") else 2.0 ** -14
    d["qw"] = scale * 2.0 ** rng.integers(0, 3, size=n)   # weights 1, 2, 4
    d["qs"] = dy(-1, 1, 8)
    off = dy(-1, 1, 16)
    off[off == 0.0] = 0.5
    d["x0"] = d["qs"] + off
    if family == "quadratic_offset":
        d["const"] = 1000.0
    elif family == "stationary":
        d["x0"] = d["qs"].copy()
    elif family == "rosenbrock":
        d["qw"] = np.zeros(n) if n > 1 else d["qw"]
        d["rosen"] = 1.0 if n > 1 else 0.0
        d["x0"] = dy(-1, 1, 16) * 1.5
    elif family == "nonsmooth":
        d["qw"] = np.ones(n)
        d["qs"] = np.full(n, 0.25)
        d["x0"] = dy(-2, 2, 8) + 0.0625
        d["ac"][a], d["as"][a] = 1.0, 0.0
        if b != a:
            d["ac"][b], d["as"][b] = 3.0, 1.0
    elif family == "linear":
        d["qw"][a] = 0.0
        d["lin"][a] = -1.0
    elif family == "abs":
        d["qw"][a] = 0.0
        d["ac"][a], d["x0"][a] = 1.0, 0.75
        if b != a:
            d["qw"][b] = 0.0
            d["ac"][b], d["x0"][b] = 3.0, -0.5
    elif family in ("nan_wall", "inf_wall"):
        # the wall stands 2^-10 above the start of the steepest variable, on the side its first step goes
        i = a
        d["qw"][i], d["qs"][i], d["x0"][i] = 8.0, 1.0, -1.0
        d["bm"][i], d["bt"][i] = 1.0, d["x0"][i] + 2.0 ** -10
        d["bad"] = math.nan if family == "nan_wall" else math.inf
    elif family == "cliff":
        d["qw"][a] = 0.0
        d["lin"][a], d["x0"][a] = -1.0, 0.0
        d["ch"][a], d["ct"][a] = 100.0, 0.7
    elif family == "floor_zero":
        # the bounded variable starts ON the floor and is pushed down hard: the bound is 1e-300 / 2^30 ... as a ratio 2^30 / 1e-300,
        # which overflows: the bound is 0 and the search is entered with step 0
        d["qw"][a] = 0.0
        d["lin"][a], d["x0"][a] = 2.0 ** 30, BOUND_MIN
    elif family == "floor_near":
        # next to the floor: the bound is 2^-20; |x_b| at its kink rises along the direction its one-sided gradient picks,
        # so a bounded search brackets at once
        d["qw"][a] = 0.0
        d["lin"][a], d["x0"][a] = 1.0, BOUND_MIN + 2.0 ** -20
        d["const"] = -(BOUND_MIN + 2.0 ** -20)
        if b != a:
            d["qw"][b] = 0.0
            d["ac"][b], d["as"][b], d["x0"][b] = 4.0, 0.0, 0.0
    elif family == "flat_then_curved":
        d["qw"][a] = 0.0
        # (slope 1024: at x ~ 2^20 the g_epsilon test, relative to |x|, must not end the run before the update it is here for)
        d["ftc"][a], d["x0"][a] = 1024.0, 0.0
    return d


# ---- parameter sets and selection ----------------------------------------------------------------------------------
FIRI = dict(g_epsilon=0.0, min_step=1.0e-32, past=3, delta=1.0e-7)        # firi.hpp:212-217 (its mem_size 18: shape (128, 18))
TIGHT = dict(max_linesearch=5, min_step=1.0e-3, max_step=1.0e3)
_SMOOTH = ("quadratic", "quadratic_offset", "stationary", "rosenbrock")
_EVERY = _SMOOTH + ("nonsmooth", "linear", "abs", "nan_wall", "inf_wall", "cliff", "flat_then_curved")
# name: (parameters, bounded, the families that run under it).  Parameters are per call, so a batch holds cases of one set.
SETS = {
    "default_it1": (dict(max_iterations=1), False, _EVERY),
    "default_it3": (dict(max_iterations=3), False, _EVERY),
    "default_it12": (dict(max_iterations=12), False, _EVERY),
    "firi": (dict(FIRI, max_iterations=12), False, _EVERY),
    "tight": (dict(TIGHT, max_iterations=6), False, ("linear", "abs", "cliff", "nonsmooth", "rosenbrock", "flat_then_curved")),
    "past0": (dict(past=0, max_iterations=12), False, _SMOOTH + ("nonsmooth", "abs")),
    "past2": (dict(past=2, delta=1.0e-3, max_iterations=12), False, ("quadratic", "quadratic_offset", "abs", "nonsmooth")),
    # machine_prec = 1/4: the one way a bracket closes (LBFGSERR_WIDTHTOOSMALL) before max_linesearch runs out
    "wide_prec": (dict(machine_prec=0.25, max_iterations=6), False, ("cliff", "nonsmooth", "abs", "quadratic")),
    # max_step = 896: the doubling steps of `flat_then_curved` pass it between 512 and 1024, the second chance at 896 lands
    # in the curved part and is accepted
    "max_step": (dict(max_step=896.0, max_iterations=6), False, ("flat_then_curved", "linear", "quadratic", "rosenbrock")),
    "bounded": (dict(max_iterations=12), True, ("floor_zero", "floor_near", "linear", "rosenbrock", "nonsmooth", "quadratic",
                                                "inf_wall")),
    "bounded_tight": (dict(TIGHT, max_iterations=6), True, ("floor_zero", "floor_near", "abs", "quadratic", "cliff")),
    # the two modes that are no lbfgs parameter: the cancel word set from the start, and an evaluation budget of 3
    "cancel": (dict(max_iterations=12), False, _EVERY, dict(cancel=1)),
    "budget": (dict(max_iterations=12), False, _EVERY, dict(max_evals=3)),
}


def seeds_of(n):
    return (0, 1) if n <= 33 else (0,)


def set_params(set_name, mem_size):
    """(lbfgs parameters, bound or None: the last third of the variables may not fall below BOUND_MIN)."""
    p, bounded = SETS[set_name][:2]
    return dict(p, mem_size=mem_size), bounded


def set_mode(set_name):
    """dict(cancel=..) / dict(max_evals=..) of the two mode sets, {} otherwise."""
    return SETS[set_name][3] if len(SETS[set_name]) > 3 else {}


_RUNS = {}


def _run_shared(family, n, seed, set_name, mem_size, mode):
    """run() of a case, shared between the history lengths of one n: a run that ended at iteration k stored at most k - 1
    pairs, so it is the same run for every mem_size >= k - 1."""
    key = (family, n, seed, set_name, mode)
    for mem, res in _RUNS.get(key, ()):
        if mem == mem_size or res["k"] - 1 <= min(mem, mem_size):
            return res
    prm, bounded = set_params(set_name, mem_size)
    res = run(make_case(family, n, seed), mode, bound=bound_of(n) if bounded else None, **set_mode(set_name), **prm)
    _RUNS.setdefault(key, []).append((mem_size, res))
    return res


def bound_of(n):
    return (n - max(1, n // 3), BOUND_MIN)


class Case:
    def __init__(self, family, n, seed, set_name, mem_size, desc, ref):
        self.family, self.n, self.seed, self.set_name, self.mem_size, self.desc, self.ref = family, n, seed, set_name, mem_size, desc, ref
        self.id = "%s-s%d-n%d-m%d-%s" % (family, seed, n, mem_size, set_name)

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=None)
def select_cases(n, mem_size, set_name):
    """Every (family, seed) at this shape and parameter set whose three runs agree in (status, k, evals) and whose mp run keeps
    MIN_MARGIN.  Returns (kept, dropped): lists of Case (ref = the mp Result) and of (id, reason)."""
    kept, dropped = [], []
    for family in SETS[set_name][2]:
        for seed in seeds_of(n):
            tag = "%s-s%d-n%d-m%d-%s" % (family, seed, n, mem_size, set_name)
            try:
                f64 = _run_shared(family, n, seed, set_name, mem_size, "f64")
                fs = _run_shared(family, n, seed, set_name, mem_size, "fsum")
            except ZeroDivisionError:          # a zero gradient that g_epsilon = 0 does not stop: 1 / |d| has no value to pin
                dropped.append((tag, "zero gradient past the g_epsilon test"))
                continue
            if f64.counters != fs.counters:
                dropped.append((tag, "f64 %s / fsum %s" % (f64.counters, fs.counters)))
                continue
            ref = _run_shared(family, n, seed, set_name, mem_size, "mp")
            if ref.counters != f64.counters:
                dropped.append((tag, "mp %s / f64 %s" % (ref.counters, f64.counters)))
            elif not ref.min_margin >= MIN_MARGIN:
                dropped.append((tag, "margin %.3g at %s" % (ref.min_margin, ref.which)))
            else:
                kept.append(Case(family, n, seed, set_name, mem_size, make_case(family, n, seed), ref))
    return kept, dropped


# the shapes of tests/test_lbfgs_forms_gpu.py: (n, mem_size) -> the update kernel lbfgs_drive (api_lbfgs.hip) takes there
SHAPES = {
    (1, 8): "wave<8,1,half>", (32, 8): "wave<8,1,half>", (32, 1): "wave<8,1,half>", (32, 3): "wave<8,1,half>",
    (33, 8): "wave<8,1>", (64, 8): "wave<8,1>",
    (65, 8): "wave<8,2>", (128, 8): "wave<8,2>", (65, 1): "wave<8,2>", (65, 3): "wave<8,2>",
    (64, 9): "wave<20,1>", (64, 20): "wave<20,1>",
    (128, 18): "wave<20,2>",
    (64, 21): "wave<0,1>",
    (128, 64): "wave<0,2>",
    (129, 8): "lane", (16, 65): "lane",
}
# workgroup size in waves and problems per wave of each form (LbfgsWaveShape<MREG>::kWaves in lbfgs_kernels.h; the lane kernel
# has 64 problems in its one wave)
FORM_GROUP = {"wave<8,1,half>": (8, 2), "wave<8,1>": (8, 1), "wave<8,2>": (8, 1), "wave<20,1>": (4, 1), "wave<20,2>": (4, 1),
              "wave<0,1>": (16, 1), "wave<0,2>": (16, 1), "lane": (1, 64)}


def kernel_form(n, mem_size):
    """The (n, mem_size) rule of lbfgs_drive, restated."""
    if n > 128 or mem_size > 64:
        return "lane"
    mreg = 8 if mem_size <= 8 else 20 if mem_size <= 20 else 0
    if mreg == 8 and n <= 32:
        return "wave<8,1,half>"
    return "wave<%d,%d>" % (mreg, 1 if n <= 64 else 2)


# which parameter sets run at which shape: all of them where a problem is small, and at every shape the sets that between
# them take every exit (the reference costs 50-digit arithmetic: n = 128 with all sets would take minutes)
CORE_SETS = ("default_it12", "tight", "wide_prec", "past2", "max_step", "bounded", "bounded_tight")
MORE_SETS = ("default_it1", "default_it3", "past0", "firi")
MODE_SETS = ("default_it1", "cancel", "budget")
MODE_SHAPES = ((32, 8), (33, 8), (65, 8), (64, 9), (128, 18), (64, 21), (128, 64), (129, 8))      # one per kernel form


def sets_of(n, mem_size):
    sets = CORE_SETS
    if (n, mem_size) in ((32, 8), (33, 8)):
        sets = sets + MORE_SETS
    if (n, mem_size) == (128, 18):
        sets = sets + ("firi",)
    if (n, mem_size) in MODE_SHAPES:
        sets = sets + tuple(s for s in MODE_SETS if s not in sets)
    return sets


def selected(n, mem_size):
    """{set name: [Case]} of a shape."""
    return {s: select_cases(n, mem_size, s)[0] for s in sets_of(n, mem_size)}


def all_selected():
    """Every selected case of every shape."""
    return [c for shape in SHAPES for cases in selected(*shape).values() for c in cases]
