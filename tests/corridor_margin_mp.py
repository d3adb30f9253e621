"""TEST INFRASTRUCTURE ONLY -- multiprecision reference for k_traj_row_margin (csrc/corridor_margin_kernels.h) and the
a-priori float64 bound its tests use.

    margin = max over the non-padding rows (a, b), max over tau in [0, 1], of g(tau) = a . u(tau) - b,
    u[ax][k] = ff(k + d, d) c_(k+d) T^k   (p^(d)(T tau) = sum_k u_k tau^k: the d-th derivative in REAL time, normalised argument)

Everything is built on the exact algebra of tests/trajectory_mp.py: `Fraction` from the doubles, the exact derivative, the
square-free part over QQ, the root count by Sturm sequences, `polyroots` at 60 digits.  The maximum of the exact g over
{0, 1} and the roots of g' in [0, 1] is the reference; nothing is rounded to double before the caller asks for it.

The `*_mp` functions need mpmath and sympy; `margin_bound`, `row_scales`, `g_float64`, `margin_float64` need numpy only, so GPU tests can
import this module without mpmath and read the references from tests/golden/corridor_margin_cases.npz
(tests/golden/make_corridor_margin_golden.py writes it).
"""
import math
from fractions import Fraction as Fr

import numpy as np

from tests import bernstein_np as bnp
from tests import trajectory_mp as tmp
from tests.trajectory_mp import _mpf, _pder, _pval, EPS

try:
    import mpmath
    import sympy
except ImportError:      # the bound helpers still work
    mpmath = sympy = None

K_MARGIN = 32
# the kernel's constants (csrc/corridor_margin_kernels.h)
MARGIN_SLACK, MARGIN_DEPTH, MARGIN_MAX_NODES, MARGIN_BISECT = 8.0, 20, 1024, 48


def deriv_exact(cm, T, d):
    """u[ax][k], ascending Fractions: trajectory_mp.normalized_deriv_exact is d^d P / dtau^d = T^d p^(d)(T tau)."""
    Tq = Fr(float(T)) ** d
    return [[c / Tq for c in ua] for ua in tmp.normalized_deriv_exact(cm, T, d)]


def is_padding(row):
    return not np.any(np.asarray(row, dtype=np.float64) != 0.0)


def row_poly_exact(u, row):
    """ascending Fractions of g(tau) = a . u(tau) - b"""
    a = [Fr(float(x)) for x in row[:3]]
    g = [sum((a[ax] * u[ax][k] for ax in range(3)), Fr(0)) for k in range(len(u[0]))]
    g[0] -= Fr(float(row[3]))
    return g


def roots01_mp(poly):
    """Real roots in [0, 1] of an exact polynomial (ascending Fractions), as mpf, each once: the steps of
    trajectory_mp.dq_roots_mp -- square-free part over QQ, the number of roots wanted by Sturm, polyroots."""
    tmp._need_mp()
    poly = list(poly)
    while len(poly) > 1 and poly[-1] == 0:
        poly.pop()
    if len(poly) <= 1:
        return []
    x = sympy.Symbol("x")
    P = sympy.Poly([sympy.Rational(c.numerator, c.denominator) for c in reversed(poly)], x, domain="QQ")
    sq = P.sqf_part()
    want = sq.count_roots(0, 1)
    if sq.degree() < 1 or want == 0:
        return []
    co = [mpmath.mpf(int(c.p)) / mpmath.mpf(int(c.q)) for c in sq.all_coeffs()]
    co = [c / co[0] for c in co]
    with mpmath.workdps(2 * tmp.DPS):
        rts = mpmath.polyroots(co, maxsteps=2000, extraprec=8 * tmp.DPS)
    tol = mpmath.mpf(10) ** (-tmp.DPS + 10)
    real = sorted(mpmath.re(r) for r in map(mpmath.mpmathify, rts)
                  if abs(mpmath.im(r)) <= tol and -tol <= mpmath.re(r) <= 1 + tol)
    real = [min(max(mpmath.mpf(r), mpmath.mpf(0)), mpmath.mpf(1)) for r in real]
    assert len(real) == want, (len(real), want)
    return real


def row_max_mp(u, row):
    """(max over [0, 1] of the exact g, a maximising tau), mpf"""
    tmp._need_mp()
    g = row_poly_exact(u, row)
    gm = [_mpf(c) for c in g]
    cand = [mpmath.mpf(0), mpmath.mpf(1)] + roots01_mp(_pder(g))
    vals = [_pval(gm, t) for t in cand]
    k = max(range(len(cand)), key=lambda j: vals[j])
    return vals[k], cand[k]


def piece_margin_mp(cm, T, d, rows):
    """The reference.  Returns (margin, row, tau, per_row): margin mpf (-inf without a row), row the first maximising row (-1),
    tau its normalised time, per_row the list of (row index, its maximum) over the non-padding rows."""
    tmp._need_mp()
    u = deriv_exact(cm, T, d)
    per = [(r, ) + row_max_mp(u, rows[r]) for r in range(len(rows)) if not is_padding(rows[r])]
    if not per:
        return -mpmath.inf, -1, mpmath.mpf(0), []
    r, m, tau = max(per, key=lambda e: e[1])
    return m, r, tau, [(e[0], e[1]) for e in per]


def row_scales(cm, T, d, rows):
    """sum_ax |a_ax| sum_k |u_ax,k| + |b| per row (0 for padding), float64 from the exact u rounded once per axis"""
    A = np.array([float(sum((abs(c) for c in ua), Fr(0))) for ua in deriv_exact(cm, T, d)])
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    sc = np.abs(rows[:, :3]) @ A + np.abs(rows[:, 3])
    return np.where([is_padding(r) for r in rows], 0.0, sc)


def margin_bound(scale):
    """|margin_float64 - margin| <= K_MARGIN * EPS * scale, scale the largest row_scales of the piece (the issue's
    sum_ax |a_ax| sum_k |u_ax,k| / T^d + |b| with u the derivative in normalised time: the u here carries the 1 / T^d).

    Roundings, each of relative size at most EPS / 2 (round to nearest), counted without fused operations so that a plain
    float64 restatement is covered as well:
      the value of a candidate, always from the components:  u_k = ff * c * T^k: T^k by repeated products <= 6, ff * c 1, the
        product 1 -> 8;  Horner of degree <= 7, a product and a sum per step -> 14;  the dot product with a and the
        subtraction of b: on a term's way 1 product, 2 sums, 1 difference -> 4.                                   26 roundings
      the location of the candidate: the roots of g' are isolated on the Bernstein control values of g, each a sum of <= 8
        terms w * u_k with a weight 0 < w <= 1 rounded once (1 + 1 product + <= 7 sums = 9) and pushed through the row's dot
        product (4): 13 roundings, so the control polygon is that of a polynomial within 13 (EPS / 2) scale of g; the maximum
        of THAT polynomial is what isolation and bisection locate (the location itself to second order), and evaluating g at
        its maximiser loses at most twice the distance between the two.                                            26 roundings
      an interval over which g varies by less than EPS scale is represented by its midpoint.                         2 roundings
    54 roundings of EPS / 2 = 27 EPS, rounded up to the power of two 32.  The scale is taken over the piece's rows because the
    row that wins in float64 need not be the exact winner: each direction of the inequality uses one row's scale.
    Pruning adds nothing: a row is dropped only when its control values, plus their own 13 (EPS / 2) scale_r <= 8 EPS scale_r,
    stay below a candidate value already found, i.e. when its exact maximum does."""
    return K_MARGIN * EPS * np.asarray(scale, dtype=np.float64)


def g_float64(cm, T, d, row, t):
    """a . p^(d)(t) - b in plain float64 at the local time t (Horner on the real-time derivative): the consistency check of
    the kernel's diagnostics (row, t)."""
    cm = np.asarray(cm, dtype=np.float64)
    v = np.array([np.polyval(np.polyder(cm[ax], d) if d else cm[ax], float(t)) for ax in range(3)])
    return float(np.dot(np.asarray(row[:3], dtype=np.float64), v) - float(row[3]))


# ---- the kernel's procedure in plain float64 --------------------------------------------------------------------------------
def _ff(k, d):
    r = 1.0
    for e in range(d):
        r *= (k - e)
    return r


def margin_float64(cm, T, d, rows, prune=True, stats=None):
    """k_traj_row_margin statement by statement in plain float64 (no fused operations): (margin, row, t)."""
    cm = np.asarray(cm, dtype=np.float64)
    D = cm.shape[1]
    n = D - 1
    tk = [1.0]
    for k in range(1, D):
        tk.append(tk[-1] * T)
    asc = np.concatenate([cm[:, ::-1], np.zeros((3, 2))], axis=1)
    u = np.array([[_ff(k + d, d) * asc[ax, k + d] * tk[k] for k in range(D)] for ax in range(3)])
    if not (np.isfinite(T) and np.isfinite(cm).all()):
        return math.nan, -1, 0.0
    A = np.abs(u).sum(axis=1)
    p1 = np.zeros(3)
    bz = np.zeros((3, D))
    for ax in range(3):
        s1 = u[ax, n]
        for k in range(n - 1, -1, -1):
            s1 = s1 + u[ax, k]
        p1[ax] = s1
        bz[ax] = bnp.bernstein(u[ax])
    best, brow, bt = -math.inf, -1, 0.0
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    for r, (ra, rb, rc, rd) in enumerate(rows):                 # first pass: the ends of every row
        if ra == 0.0 and rb == 0.0 and rc == 0.0 and rd == 0.0:
            continue
        if not np.isfinite([ra, rb, rc, rd]).all():
            return math.nan, -1, 0.0
        for tau, p in ((0.0, u[:, 0]), (1.0, p1)):
            g = (rc * p[2] + (rb * p[1] + ra * p[0])) - rd
            if g > best:
                best, brow, bt = g, r, tau
    live = []
    for r, (ra, rb, rc, rd) in enumerate(rows):                 # second pass: mark the rows that may still raise `best`
        if ra == 0.0 and rb == 0.0 and rc == 0.0 and rd == 0.0:
            continue
        ub = max((rc * bz[2, ii] + (rb * bz[1, ii] + ra * bz[0, ii])) - rd for ii in range(D))
        scale = abs(rc) * A[2] + (abs(rb) * A[1] + (abs(ra) * A[0] + abs(rd)))
        if not prune or ub + MARGIN_SLACK * EPS * scale > best:
            live.append(r)
        elif stats is not None:
            stats["pruned"] = stats.get("pruned", 0) + 1
    for r in live:                                              # third pass: the marked rows, tested again
        ra, rb, rc, rd = rows[r]

        def dotrow(x, y, z):
            return (rc * z + (rb * y + ra * x)) - rd

        def candidate(tau):
            nonlocal best, brow, bt
            v = []
            for ax in range(3):
                h = u[ax, n]
                for k in range(n - 1, -1, -1):
                    h = h * tau + u[ax, k]
                v.append(h)
            g = dotrow(*v)
            if g > best:
                best, brow, bt = g, r, tau

        cv = [dotrow(*bz[:, ii]) for ii in range(D)]
        scale = abs(rc) * A[2] + (abs(rb) * A[1] + (abs(ra) * A[0] + abs(rd)))
        if prune and not (max(cv) + MARGIN_SLACK * EPS * scale > best):
            if stats is not None:
                stats["pruned"] = stats.get("pruned", 0) + 1
            continue
        dv = [cv[k + 1] - cv[k] for k in range(n)]
        gd = [(k + 1) * (rc * u[2, k + 1] + (rb * u[1, k + 1] + ra * u[0, k + 1])) for k in range(n)]
        lev, idx = 0, 0
        for _ in range(MARGIN_MAX_NODES):
            var, first, mx = bnp.sign_scan(bnp.descend(dv, lev, idx))
            width = math.ldexp(1.0, -lev)
            lo = idx * width
            mid = lo + 0.5 * width
            split = False
            if var == 0:
                pass
            elif n * mx * width <= EPS * scale:
                candidate(mid)
            elif var == 1:
                if first > 0:
                    lo_, hi_ = lo, lo + width
                    for _it in range(MARGIN_BISECT):
                        mm = 0.5 * (lo_ + hi_)
                        fm = gd[n - 1]
                        for k in range(n - 2, -1, -1):
                            fm = fm * mm + gd[k]
                        if fm > 0.0:
                            lo_ = mm
                        else:
                            hi_ = mm
                    candidate(0.5 * (lo_ + hi_))
            else:
                candidate(mid)
                split = lev < MARGIN_DEPTH
            if stats is not None:
                stats["nodes"] = stats.get("nodes", 0) + 1
            lev, idx, more = bnp.advance(lev, idx, split)
            if not more:
                break
    return best, brow, bt * T
