"""TEST INFRASTRUCTURE ONLY -- multiprecision reference for k_traj_clearance (csrc/clearance_kernels.h), the a-priori bound its
tests use, and a float64 restatement of the kernel's procedure.

    clearance = min over the finite points q, min over tau in [0, 1], of || u(tau) - q ||,   u[ax][k] = c_k T^k  (p(T tau))

Built on the exact algebra of tests/trajectory_mp.py and the root isolation of tests/corridor_margin_mp.py (`Fraction` from the
doubles, square-free part over QQ, root count by Sturm sequences, `polyroots` at 60 digits): per point g = ||u - q||^2 is an exact
polynomial, the real roots of g' in [0, 1] and the two ends are the candidates, the smallest sqrt(g) over them is the point's
distance and the smallest over the points the reference.  The runner-up point's distance is recorded too, so that index ties can
be recognised.

The `*_mp` functions need mpmath and sympy; `clearance_bound`, `scales`, `clearance_float64` need numpy only, so GPU tests read
the references from tests/golden/traj_clearance_cases.npz (tests/golden/make_traj_clearance_golden.py writes it).
"""
from fractions import Fraction as Fr

import numpy as np

from tests import bernstein_np as bnp
from tests import corridor_margin_mp as cmm
from tests import trajectory_mp as tmp
from tests.trajectory_mp import _mpf, _pder, _pmul, _padd, _pval, EPS

try:
    import mpmath
except ImportError:
    mpmath = None

# the kernel's structural constants (csrc/clearance_kernels.h)
CLR_K, CLR_DEPTH, CLR_MAX_NODES, CLR_BISECT, CLR_SLACK = 9, 20, 1024, 64, 16.0
K_CLR, K_LOC = 32.0, 32.0
CAP = 1e-9          # the vacuity cap of the bound on every fixture case, metres


def u_exact(cm, T):
    """u[ax][k], ascending Fractions: the exact coefficients of p(T tau)"""
    cm = np.asarray(cm, dtype=np.float64)
    n = cm.shape[1] - 1
    Tq = Fr(float(T))
    return [[Fr(float(cm[ax, n - k])) * Tq ** k for k in range(n + 1)] for ax in range(3)]


def finite_points(pts):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    return [j for j in range(len(pts)) if np.all(np.isfinite(pts[j]))]


def g_exact(u, q):
    """ascending Fractions of g(tau) = || u(tau) - q ||^2"""
    g = [Fr(0)]
    for ax in range(3):
        d = list(u[ax])
        d[0] = d[0] - Fr(float(q[ax]))
        g = _padd(g, _pmul(d, d))
    return g


def point_min_mp(u, q):
    """(distance, tau, kappa, interior, speed): the smallest || u(tau) - q || over [0, 1] (mpf), a minimiser, kappa = g''(tau) / 2
    there, whether the minimiser is a root of g' strictly inside (0, 1), and || u'(tau) || there"""
    tmp._need_mp()
    g = g_exact(u, q)
    gm = [_mpf(c) for c in g]
    roots = cmm.roots01_mp(_pder(g))
    cand = [mpmath.mpf(0), mpmath.mpf(1)] + roots
    vals = [_pval(gm, t) for t in cand]
    k = min(range(len(cand)), key=lambda j: vals[j])
    g2 = [_mpf(c) for c in _pder(g, 2)]
    speed = mpmath.sqrt(sum(_pval([_mpf(c) for c in _pder(ua)], cand[k]) ** 2 for ua in u))
    return mpmath.sqrt(max(vals[k], 0)), cand[k], _pval(g2, cand[k]) / 2, bool(k >= 2 and 0 < cand[k] < 1), speed


def piece_clearance_mp(cm, T, pts):
    """The reference.  dict: d (mpf; +inf without a finite point), point (-1), tau, kappa, speed, interior, runner (the second smallest
    of the points' distances, +inf with fewer than two finite points), per_point [(index, distance)]."""
    tmp._need_mp()
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    u = u_exact(cm, T)
    per = [(j, ) + point_min_mp(u, pts[j]) for j in finite_points(pts)]
    res = {"d": mpmath.inf, "point": -1, "tau": mpmath.mpf(0), "kappa": mpmath.mpf(0), "speed": mpmath.mpf(0), "interior": False,
           "runner": mpmath.inf,
           "per_point": [(e[0], e[1]) for e in per]}
    if not per:
        return res
    per.sort(key=lambda e: e[1])
    j, d, tau, kappa, interior, speed = per[0]
    res.update(d=d, point=j, tau=tau, kappa=kappa, interior=interior, speed=speed, runner=per[1][1] if len(per) > 1 else mpmath.inf)
    return res


def dist_mp(cm, T, t, q):
    """|| p(t) - q || at 60 digits, t a double in local time: the consistency check of the diagnostics (point, t)"""
    tmp._need_mp()
    cm = np.asarray(cm, dtype=np.float64)
    n = cm.shape[1] - 1
    tq = Fr(float(t))
    s = Fr(0)
    for ax in range(3):
        v = _pval([Fr(float(cm[ax, n - k])) for k in range(n + 1)], tq) - Fr(float(q[ax]))
        s += v * v
    return mpmath.sqrt(_mpf(s))


def dist_exact(cm, T, t, q):
    """|| p(t) - q || with the square formed in exact rational arithmetic (standard library only) and rounded once before the
    root: within two units in the last place of the true distance.  The GPU tests use it for the consistency check of (point, t)
    in place of the 60-digit dist_mp: it is at least as strict (dist_mp rounds at 60 digits, this at no digit before the last
    step) and needs no mpmath where the GPU tests run; test_traj_clearance_cpu.py checks the two against each other."""
    import math
    cm = np.asarray(cm, dtype=np.float64)
    n = cm.shape[1] - 1
    tq = Fr(float(t))
    s = Fr(0)
    for ax in range(3):
        v = _pval([Fr(float(cm[ax, n - k])) for k in range(n + 1)], tq) - Fr(float(q[ax]))
        s += v * v
    # scale by an even power of two so that the rounding of a tiny square is not subnormal
    return math.sqrt(float(s * Fr(2) ** 600)) * 2.0 ** -300 if s < Fr(1, 2 ** 400) else math.sqrt(float(s))


def bound_float64(cm, T, pts, point, t, d):
    """clearance_bound for a result (point, t, d) without the multiprecision reference: scale and a1 from float64 sums, speed =
    ||u'|| and kappa = ||u'||^2 + (u - q) . u'' at the reported time, interior unless t is an end"""
    cm = np.asarray(cm, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = cm.shape[1] - 1
    u = cm[:, ::-1] * np.cumprod(np.r_[1.0, np.full(n, float(T))])[None]
    A, A1 = np.abs(u).sum(axis=1), (np.abs(u) * np.arange(n + 1)[None]).sum(axis=1)
    fin = pts[np.all(np.isfinite(pts), axis=1)]
    if point < 0 or len(fin) == 0:
        return 0.0
    scale = (A[None] + np.abs(fin)).sum(axis=1).max()
    tau = float(t) / float(T) if T > 0 else 0.0
    pw = np.array([np.polyval(u[ax][::-1], tau) for ax in range(3)]) - pts[point]
    d1 = np.array([np.polyval(np.polyder(u[ax][::-1]), tau) for ax in range(3)])
    d2 = np.array([np.polyval(np.polyder(u[ax][::-1], 2), tau) for ax in range(3)])
    kappa = float(d1 @ d1 + pw @ d2)
    interior = 0.0 < tau < 1.0 and kappa > 0.0
    return float(clearance_bound(scale, A1.sum(), np.linalg.norm(d1), kappa, d, interior))


def scales(cm, T, pts):
    """(scale, a1): scale = sum_ax (sum_k |u_ax,k| + |q_ax|), the largest over the finite points of the set (0 without one);
    a1 = sum_ax sum_k k |u_ax,k|;  float64 from the exact u (standard library and numpy only)"""
    u = u_exact(cm, T)
    A = np.array([float(sum((abs(c) for c in ua), Fr(0))) for ua in u])
    a1 = float(sum((k * abs(c) for ua in u for k, c in enumerate(ua)), Fr(0)))
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    fin = finite_points(pts)
    if not fin:
        return 0.0, a1
    return float((A[None] + np.abs(pts[fin])).sum(axis=1).max()), a1


def clearance_bound(scale, a1, speed, kappa, d, interior):
    """|clearance_float64 - clearance| <= K_CLR EPS scale + location term.

    The VALUE of a candidate, in roundings of relative size EPS / 2, counted without fused operations so that a plain float64
    restatement is covered: u_k = c_k T^k, T^k by repeated products <= 6, the product 1, rounded up to 8 as in margin_bound;
    Horner of degree <= 7, a product and a sum per step, 14; the difference with q, 1, on |u| + |q|: 23 roundings on a component,
    11.5 EPS (sum_k |u_ax,k| + |q_ax|).  The Euclidean norm is 1-Lipschitz and at most the sum of the components' moduli, so the
    three component errors enter as 11.5 EPS scale, also where the components cancel; three squares, two sums and the root are
    at most 3 relative roundings of a distance <= scale: 1.5 EPS scale.  t = tau T is rounded once, which moves the curve by at
    most EPS / 2 sum_k k |u_k| <= 3.5 EPS scale (the consistency check of (point, t) evaluates at the rounded t).  16.5 EPS scale,
    rounded up to the power of two 32 = K_CLR.  This part is two-sided and holds for EVERY reported value, because a value is
    always the norm of the difference vector at a time in [0, T]: clearance_float64 >= clearance - K_CLR EPS scale, whatever the
    search did.

    The LOCATION term bounds by how much the candidate time misses the minimiser; it is zero at an end (tau = 0 and 1 are
    candidates exactly) and where the set has no point.  At an interior minimum tau* with kappa = g''(tau*) / 2 > 0 the kernel
    bisects h = g' / 2 = (u - q) . u' from the three components down to neighbouring doubles and takes both as candidates.  Per
    axis the computed factor u - q is within 11.5 EPS (A_ax + |q_ax|) of the exact one (as above) and the computed u' within
    16 EPS sum_k k |u_ax,k| (its Horner recurrence reuses the rounded partial values of u: 8 + 2 x 14 roundings at most), so the
    product errs by 11.5 EPS (A_ax + |q_ax|) |u'_ax| + 16 EPS sum_k k |u_ax,k| |u_ax - q_ax|, and its own rounding and the sums over
    the axes add 1.5 EPS |u_ax - q_ax| |u'_ax|.  At the minimiser |u'_ax| <= speed = ||u'(tau*)|| and |u_ax - q_ax| <= d* <= scale:
        E_h = 16 EPS scale speed + 32 EPS a1 d*,      a1 = sum_ax sum_k k |u_ax,k|
    (13 and 17.5, rounded up to powers of two).  The first term is what a near-touching point sees (d* -> 0), the second what a
    distant one sees; neither carries the product of the two coefficient sums, which no point of the curve attains.  So one of the
    two candidates is within E / kappa of tau*, E = E_h + 2 EPS kappa (the spacing of doubles in [0, 1] against the slope kappa of
    h), g exceeds its minimum there by kappa (E / kappa)^2 to first order, 2 E^2 / kappa with room for the second order, and
    d^ - d* = (g^ - g*) / (d^ + d*) <= min(sqrt(g^ - g*), (g^ - g*) / (2 d*)):
        location = min( sqrt(2) E / sqrt(kappa),  E^2 / (kappa d*) ).
    With d* -> 0, kappa -> speed^2 and the first form is sqrt(2) 16 EPS scale: a near-touching curve is no worse than a distant
    one.  The bound is first order in the location, as hit_bound is: a minimiser with kappa -> 0 (the curve all but stops next to
    the point, the point at a centre of curvature, or a tangential cluster of critical points) drives it up; no fixture case is
    selected by it.  Pruning adds nothing: a point is dropped only when its nine sampled distances less L h / 2, plus their own
    rounding (CLR_SLACK EPS scale_j), stay above a value already found, i.e. when its exact minimum does.  Isolation (sign changes
    of Bernstein control values of h, formed with positive weights from the control values of u - q and u') decides on numbers
    within 2 (2n) EPS scale a1 of the exact control values, subdivision included; a sign it misjudges belongs to an interval on
    which |h| is that small, where g varies by less than 2 |h| width, and the split points and ends are candidates."""
    scale, a1, speed, kappa, d = (np.asarray(x, dtype=np.float64) for x in (scale, a1, speed, kappa, d))
    interior = np.asarray(interior, dtype=bool)
    val = K_CLR * EPS * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        E = 16.0 * EPS * scale * speed + K_LOC * EPS * a1 * d + 2.0 * EPS * kappa
        loc = np.minimum(np.sqrt(2.0) * E / np.sqrt(kappa), E * E / (kappa * d))
    loc = np.where(interior & (a1 > 0.0), loc, 0.0)
    return val + loc


def cap_of(family, s):
    """The vacuity cap of the bound for a fixture family, metres: CAP = 1e-9 everywhere but for the Chebyshev-like family of
    order 4.  Its components are amp T_7(2 tau - 1) + offset with amp <= 3 m, and the moduli of the monomial coefficients of
    T_n(2 tau - 1) sum to T_n(3) = 114 243 for n = 7 (3363 for n = 5, 99 for n = 3).  With |offset| <= 8 and |q| <= 11.5 the scale
    is as large as 3 (3 x 114 243 + 19.5) = 1.03e6, and the value term alone, 32 EPS scale, reaches 7.3e-9 m: no bound of the
    issue's form C EPS scale with this scale can meet 1e-9 (C would have to be below 4.4, and forming u_k = c_k T^k alone costs
    4).  The family is kept with the same derived bound and twice that value term as its cap, which asks the location term to
    stay below the value term."""
    if family == "cheb" and s == 4:
        return 2.0 * K_CLR * EPS * 3.0 * (3.0 * 114243.0 + 19.5)
    return CAP


# ---- the kernel's procedure in plain float64 --------------------------------------------------------------------------------
def _horner(ua, tau):
    v = ua[-1]
    for c in ua[-2::-1]:
        v = v * tau + c
    return v


def _h(u, q, tau):
    hm = 0.0
    for ax in range(3):
        v, dd = u[ax][-1], 0.0
        for c in u[ax][-2::-1]:
            dd = dd * tau + v
            v = v * tau + c
        hm += (v - q[ax]) * dd
    return hm


def clearance_float64(cm, T, pts, count=None, stats=None):
    """The kernel's procedure, step by step, in numpy float64 without fused operations -> (clearance, point, t).  `stats`, a
    dict, receives: survivors (points refined), nodes_out (survivors whose interval budget ran out), depth_out (clusters that
    reached the depth bound)."""
    cm = np.asarray(cm, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    st = {"survivors": 0, "nodes_out": 0, "depth_out": 0}
    if stats is not None:
        stats.update(st)
        st = stats
    D = cm.shape[1]
    n = D - 1
    M = 2 * n
    T = float(T)
    with np.errstate(all="ignore"):
        tk = np.cumprod(np.r_[1.0, np.full(n, T)])
        u = cm[:, ::-1] * tk[None]
    if not np.isfinite(T) or T < 0.0 or not np.all(np.isfinite(cm)) or not np.all(np.isfinite(u)):
        return np.nan, -1, 0.0
    cnt = len(pts) if count is None else min(max(int(count), 0), len(pts))
    A1 = float(np.abs(u).sum())
    bz = np.stack([bnp.bernstein(u[ax]) for ax in range(3)])
    taus = np.arange(CLR_K) / (CLR_K - 1)
    pos = np.stack([[_horner(u[ax], t) for t in taus] for ax in range(3)])           # (3, K)
    Lh2 = float(np.sqrt((np.diff(bz, axis=1) ** 2).sum(axis=0).max())) * (n * 0.5 / (CLR_K - 1))
    valid = [j for j in range(cnt) if np.all(np.isfinite(pts[j]))]
    best2, bp, bt = np.inf, -1, 0.0

    def nearest(q):
        d2 = ((pos - q[:, None]) ** 2).sum(axis=0)
        k = int(np.argmin(d2))
        return float(d2[k]), k

    for j in valid:
        d2, k = nearest(pts[j])
        if d2 < best2:
            best2, bp, bt = d2, j, taus[k]

    def thr2(q):
        sc = A1 + float(np.abs(q).sum())
        thr = np.sqrt(best2) + Lh2 + CLR_SLACK * EPS * sc
        return thr * thr * (1.0 + 8.0 * EPS)

    for j in valid:
        q = pts[j]
        if not nearest(q)[0] < thr2(q):
            continue
        st["survivors"] += 1
        sc = A1 + float(np.abs(q).sum())
        flat = (EPS * sc) ** 2

        def candidate(tau):
            nonlocal best2, bp, bt
            d2 = sum((_horner(u[ax], tau) - q[ax]) ** 2 for ax in range(3))
            if d2 < best2:
                best2, bp, bt = float(d2), j, float(tau)

        dv = bnp.product_cv(bz - q[:, None], bz)
        lev, idx, done = 0, 0, False
        for _ in range(CLR_MAX_NODES):
            var, first, mx = bnp.sign_scan(bnp.descend(dv, lev, idx))
            width = 2.0 ** -lev
            lo = idx * width
            mid = lo + 0.5 * width
            split = False
            if var == 0:
                pass
            elif 2.0 * n * mx * width <= flat:
                candidate(mid)
            elif var == 1:
                if first < 0:
                    l_, h_ = lo, lo + width
                    for _it in range(CLR_BISECT):
                        mm = 0.5 * (l_ + h_)
                        if not (l_ < mm < h_):
                            break
                        if _h(u, q, mm) < 0.0:
                            l_ = mm
                        else:
                            h_ = mm
                    candidate(l_)
                    candidate(h_)
            else:
                candidate(mid)
                split = lev < CLR_DEPTH
                if not split:
                    st["depth_out"] += 1
            lev, idx, more = bnp.advance(lev, idx, split)
            if not more:
                done = True
                break
        if not done:
            st["nodes_out"] += 1
    if bp < 0:
        return np.inf, -1, 0.0
    return float(np.sqrt(best2)), bp, bt * T
