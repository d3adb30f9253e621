"""TEST INFRASTRUCTURE ONLY -- multiprecision reference for k_traj_separation (csrc/separation_kernels.h), the a-priori bound its
tests use, and a float64 restatement of the kernel's procedure.

    sep = min over the common intervals, min over t, of || p_a,i(t - K_i^a) - p_b,j(t - K_j^b) ||

Knots are the float64 sums K_0 = t0, K_(i+1) = K_i + T_i (`knots`); the reference takes these doubles as rationals, so the definition
has no rounding in it.  Built on the exact algebra of tests/trajectory_mp.py and the root isolation of tests/corridor_margin_mp.py:
per interval [lo, hi], g(sigma) = || d(lo + sigma (hi - lo)) ||^2 is an exact polynomial (global time, mapped affinely onto [0, 1]
for the isolation), the real roots of g' in [0, 1] and the two ends are the candidates.  The smallest sqrt(g) over the intervals
is the reference, the smallest over the OTHER intervals the runner-up, recorded so that index ties can be recognised.

The `*_mp` functions need mpmath and sympy; `separation_bound`, `pair_scales`, `dist_exact`, `separation_float64` need numpy only,
so GPU tests read the references from tests/golden/traj_separation_cases.npz (tests/golden/make_traj_separation_golden.py).
"""
import math
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

# the kernel's structural constants (csrc/separation_kernels.h)
SEP_K, SEP_STEPS, SEP_DEPTH, SEP_MAX_NODES, SEP_BISECT, SEP_SLACK = 9, 64, 20, 1024, 64, 64.0
K_SEP, K_TIME = 64.0, 4.0
CAP = 1e-9          # the vacuity cap of the bound on every fixture case, metres


def knots(T, t0=0.0):
    """K_0 .. K_N of one trajectory: float64 sums in piece order"""
    K = [float(t0)]
    for Ti in np.asarray(T, dtype=np.float64):
        K.append(K[-1] + float(Ti))
    return K


def intervals(Ka, Kb):
    """[(lo, hi, i, j)]: the maximal sub-intervals of W of positive length between consecutive distinct knots of either
    trajectory, with the piece of each that spans it"""
    lo_w, hi_w = max(Ka[0], Kb[0]), min(Ka[-1], Kb[-1])
    cuts = sorted({k for k in Ka + Kb if lo_w <= k <= hi_w})
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        i = next(i for i in range(len(Ka) - 1) if Ka[i] <= lo and hi <= Ka[i + 1] and Ka[i] < Ka[i + 1])
        j = next(j for j in range(len(Kb) - 1) if Kb[j] <= lo and hi <= Kb[j + 1] and Kb[j] < Kb[j + 1])
        out.append((lo, hi, i, j))
    return out


def _compose(cm_ax, x0, w):
    """ascending Fractions of p(x0 + w sigma), p given highest power first in doubles"""
    lin = [x0, w]
    r = [Fr(0)]
    for c in cm_ax:
        r = _padd(_pmul(r, lin), [Fr(float(c))])
    return r


def d_exact(cma, cmb, Kai, Kbj, lo, hi):
    """the three components of p_a(t - Kai) - p_b(t - Kbj), t = lo + sigma (hi - lo): ascending Fractions in sigma"""
    lo, hi = Fr(float(lo)), Fr(float(hi))
    w = hi - lo
    return [_padd(_compose(cma[ax], lo - Fr(float(Kai)), w), [-c for c in _compose(cmb[ax], lo - Fr(float(Kbj)), w)]) for ax in range(3)]


def g_of(d):
    g = [Fr(0)]
    for da in d:
        g = _padd(g, _pmul(da, da))
    return g


def interval_min_mp(d):
    """(distance, sigma, kappa = g''/2, interior, speed = ||dd/dsigma||) of one interval, all in sigma"""
    tmp._need_mp()
    g = g_of(d)
    gm = [_mpf(c) for c in g]
    cand = [mpmath.mpf(0), mpmath.mpf(1)] + cmm.roots01_mp(_pder(g))
    vals = [_pval(gm, t) for t in cand]
    k = min(range(len(cand)), key=lambda j: vals[j])
    g2 = [_mpf(c) for c in _pder(g, 2)]
    speed = mpmath.sqrt(sum(_pval([_mpf(c) for c in _pder(da)], cand[k]) ** 2 for da in d))
    return mpmath.sqrt(max(vals[k], 0)), cand[k], _pval(g2, cand[k]) / 2, bool(k >= 2 and 0 < cand[k] < 1), speed


def pair_separation_mp(coa, Ta, t0a, cob, Tb, t0b):
    """The reference for one pair: coa (N, 3, D), Ta (N,), t0a; the same for b.  dict: d (mpf, +inf without an interval), t
    (global, mpf), pa, pb, sigma, kappa, speed (both in sigma of the interval), interior, width, runner (the smallest minimum of
    the other intervals, +inf with fewer than two), n_int."""
    tmp._need_mp()
    Ka, Kb = knots(Ta, t0a), knots(Tb, t0b)
    res = {"d": mpmath.inf, "t": mpmath.mpf(0), "pa": -1, "pb": -1, "sigma": mpmath.mpf(0), "kappa": mpmath.mpf(0),
           "speed": mpmath.mpf(0), "interior": False, "width": 0.0, "runner": mpmath.inf, "n_int": 0}
    per = []
    for lo, hi, i, j in intervals(Ka, Kb):
        per.append((interval_min_mp(d_exact(coa[i], cob[j], Ka[i], Kb[j], lo, hi)), lo, hi, i, j))
    res["n_int"] = len(per)
    if not per:
        return res
    per.sort(key=lambda e: e[0][0])
    (d, sg, kappa, interior, speed), lo, hi, i, j = per[0]
    res.update(d=d, t=_mpf(Fr(lo)) + sg * _mpf(Fr(hi) - Fr(lo)), pa=i, pb=j, sigma=sg, kappa=kappa, speed=speed, interior=interior,
               width=hi - lo, runner=per[1][0][0] if len(per) > 1 else mpmath.inf)
    return res


def _dist2_exact(cma, Kai, cmb, Kbj, t):
    tq = Fr(float(t))
    s = Fr(0)
    for ax in range(3):
        va = _pval([Fr(float(c)) for c in cma[ax][::-1]], tq - Fr(float(Kai)))
        vb = _pval([Fr(float(c)) for c in cmb[ax][::-1]], tq - Fr(float(Kbj)))
        s += (va - vb) ** 2
    return s


def dist_mp(cma, Kai, cmb, Kbj, t):
    """|| p_a(t - Kai) - p_b(t - Kbj) || at 60 digits, t a double in global time"""
    tmp._need_mp()
    return mpmath.sqrt(_mpf(_dist2_exact(cma, Kai, cmb, Kbj, t)))


def dist_exact(cma, Kai, cmb, Kbj, t):
    """The same with the square formed in exact rational arithmetic (standard library only) and rounded once before the root:
    within two units in the last place of the true distance.  The consistency check of (t, pieces) on the GPU, where mpmath
    need not exist; test_traj_separation_cpu.py checks it against dist_mp."""
    s = _dist2_exact(cma, Kai, cmb, Kbj, t)
    return math.sqrt(float(s * Fr(2) ** 600)) * 2.0 ** -300 if s < Fr(1, 2 ** 400) else math.sqrt(float(s))


def piece_sums(cm, T):
    """(A, a1) of one piece from its doubles, exactly: A = sum_ax sum_k |c_k T^k|, a1 = sum_ax sum_k k |c_k T^k|"""
    cm = np.asarray(cm, dtype=np.float64)
    n = cm.shape[1] - 1
    Tq = Fr(float(T))
    u = [[abs(Fr(float(cm[ax, n - k])) * Tq ** k) for k in range(n + 1)] for ax in range(3)]
    return float(sum((c for ua in u for c in ua), Fr(0))), float(sum((k * c for ua in u for k, c in enumerate(ua)), Fr(0)))


def pair_scales(cma, Ta, cmb, Tb):
    """(scale, vmax) of two pieces: scale = A_a + A_b; vmax = a1_a / T_a + a1_b / T_b, which bounds the speed of the difference
    curve in global time over both pieces (|du/dtau| <= sum_k k |u_k| on [0, 1])"""
    Aa, a1a = piece_sums(cma, Ta)
    Ab, a1b = piece_sums(cmb, Tb)
    return Aa + Ab, a1a / float(Ta) + a1b / float(Tb)


def separation_bound(scale, vmax, tabs, n, speed, kappa, d, interior):
    """|separation_float64 - sep| <= K_SEP EPS scale + K_TIME EPS tabs vmax + location term.

    VALUE.  A candidate's value is the norm of the difference vector d at a sigma, and d comes from the doubles as follows, counted
    in roundings of relative size EPS / 2 without fused operations (a plain float64 restatement is covered): u_k = c_k T^k, as in
    clearance_bound, 8; a Bernstein control value is a sum of at most 8 terms weight x u_k with weights C(i,k)/C(n,k) <= 1 (the
    rounded weight, the product, the running sum: 3 for a term, 7 more for the sums behind it), 10, on sum_k |u_k|; each of the two
    de Casteljau subdivisions takes n <= 7 levels of (1 - t) x + t y (1 - t, two products, a sum: 4 a level; convex, so nothing grows
    past sum_k |u_k|), 56; the evaluation at sigma, n more levels, 28; the difference a - b, 1.  103 roundings on a component, 51.5
    EPS (A_ax^a + A_ax^b).  The norm is 1-Lipschitz and at most the sum of the components' moduli, so the three enter as 51.5 EPS
    scale; three squares, two sums and the root are 1.5 EPS scale.  53, rounded up to the power of two 64 = K_SEP.  Two-sided, and
    true of EVERY reported value whatever the search did (budgets, cutoff): a value is always a distance of the two curves.
    TIME.  Where the kernel's sigma lies in global time is not exact: alpha = (lo - K_i) / T_i and beta, two roundings each, move an
    end of the restricted piece by at most EPS x (its local time); w = hi - lo and t = lo + sigma w, three roundings, move the
    reported time by 1.5 EPS tabs.  So the point of curve a the kernel holds at sigma and p_a at the reported t are at most
    2.5 EPS tabs apart in time, likewise b; tabs is the largest modulus among lo, hi and the four knots of the two pieces, and
    vmax (pair_scales) bounds the speeds: 2.5 EPS tabs vmax, rounded up to K_TIME = 4.  This is the term for the rounding of the
    interval ends; the consistency check of (t, pieces) evaluates at the rounded t and needs it too.
    LOCATION.  Zero at an end of an interval (sigma = 0 and 1 are candidates exactly).  At an interior minimum sigma* with kappa =
    g''(sigma*) / 2 > 0 the kernel bisects h = d . d' down to neighbouring doubles, h from the components by de Casteljau: the
    computed d is within 32 EPS scale per the count above without the norm (51.5, of which the part before the evaluation is
    common to both ends of the bisection and is counted all the same), the computed d' = n (v_1 - v_0) within 2 n x that, so
        E = 32 EPS scale speed + 64 n EPS scale d* + 2 EPS kappa
    (speed = ||dd/dsigma|| at sigma*; the last term is the spacing of doubles in [0, 1] against the slope kappa of h), one of the two
    candidates is within E / kappa of sigma*, and as in clearance_bound
        location = min( sqrt(2) E / sqrt(kappa),  E^2 / (kappa d*) ),
    first order in the location.  Pruning adds nothing: an interval is left out only when its nine sampled distances less L h / 2,
    plus SEP_SLACK EPS scale for their own rounding, stay above a value already found or above the cutoff."""
    scale, vmax, tabs, n, speed, kappa, d = (np.asarray(x, dtype=np.float64) for x in (scale, vmax, tabs, n, speed, kappa, d))
    interior = np.asarray(interior, dtype=bool)
    val = K_SEP * EPS * scale + K_TIME * EPS * tabs * vmax
    with np.errstate(divide="ignore", invalid="ignore"):
        E = 32.0 * EPS * scale * speed + 64.0 * n * EPS * scale * d + 2.0 * EPS * kappa
        loc = np.minimum(np.sqrt(2.0) * E / np.sqrt(kappa), E * E / (kappa * d))
    loc = np.where(interior & (kappa > 0.0), loc, 0.0)
    return val + loc


def value_bound(scale, vmax, tabs):
    """the two-sided part of separation_bound that holds for every reported value"""
    return K_SEP * EPS * np.asarray(scale) + K_TIME * EPS * np.asarray(tabs) * np.asarray(vmax)


def cap_of(family, s):
    """The vacuity cap of the bound for a fixture family, metres: CAP everywhere.  (The Chebyshev-like family keeps to degree 5
    and amplitude 1 m, so that its coefficient sums, T_5(3) = 3363 per unit of amplitude, leave the value term below CAP.)"""
    return CAP


def fixture_case(fx, i):
    """case i of tests/golden/traj_separation_cases.npz -> (co (2, N, 3, 2s), T (2, N), t0 (2,), (a, b))"""
    s, N = int(fx["s"][i]), int(fx["n"][i])
    return fx["co"][i][:, :N, :, :2 * s].copy(), fx["T"][i][:, :N].copy(), fx["t0"][i].copy(), (int(fx["pair"][i][0]), int(fx["pair"][i][1]))


def pieces_bound(co, T, t0, pair, pa, pb, t, speed, kappa, d, interior):
    """(bound, value part) for a minimum at global time t in pieces (pa, pb): scale, vmax and tabs are formed here from the case's
    doubles; speed and kappa are in sigma of the interval, as pair_separation_mp returns them"""
    a, b = pair
    Ka, Kb = knots(T[a], t0[a]), knots(T[b], t0[b])
    scale, vmax = pair_scales(co[a, pa], T[a, pa], co[b, pb], T[b, pb])
    tabs = max(abs(x) for x in (Ka[pa], Ka[pa + 1], Kb[pb], Kb[pb + 1], t))
    n = co.shape[3] - 1
    return float(separation_bound(scale, vmax, tabs, n, speed, kappa, d, interior)), float(value_bound(scale, vmax, tabs))


def fixture_bound(fx, i):
    co, T, t0, pair = fixture_case(fx, i)
    if fx["pa"][i] < 0:
        return 0.0, 0.0
    b, v = pieces_bound(co, T, t0, pair, int(fx["pa"][i]), int(fx["pb"][i]), float(fx["t"][i]), fx["speed"][i], fx["kappa"][i],
                        fx["d"][i], fx["interior"][i])
    # a result may come from another interval that ties with the reference's: its value part holds there
    w = worst_value_bound(co, T, t0, pair)
    return max(b, w), max(v, w)


def worst_value_bound(co, T, t0, pair):
    """the largest value part over every pair of pieces that share an interval: what a result in ANY interval may err by"""
    a, b = pair
    Ka, Kb = knots(T[a], t0[a]), knots(T[b], t0[b])
    out = 0.0
    for lo, hi, i, j in intervals(Ka, Kb):
        scale, vmax = pair_scales(co[a, i], T[a, i], co[b, j], T[b, j])
        out = max(out, float(value_bound(scale, vmax, max(abs(x) for x in (Ka[i], Ka[i + 1], Kb[j], Kb[j + 1])))))
    return out


def check_result(fx, i, bound, res, need_pieces=True):
    """the assertions of the issue on one result (sep, t, pa, pb) of case i"""
    co, T, t0, (a, b) = fixture_case(fx, i)
    sep, t, pa, pb = res
    if fx["pa"][i] < 0:
        assert sep == np.inf and t == 0.0 and pa == -1 and pb == -1, (i, res)
        return 0.0
    ref = fx["d"][i]
    assert abs(sep - ref) <= bound[0] and sep >= ref - bound[0], (i, sep, ref, bound)
    Ka, Kb = knots(T[a], t0[a]), knots(T[b], t0[b])
    assert 0 <= pa < T.shape[1] and 0 <= pb < T.shape[1]
    assert max(Ka[0], Kb[0]) <= t <= min(Ka[-1], Kb[-1]) and Ka[pa] <= t <= Ka[pa + 1] and Kb[pb] <= t <= Kb[pb + 1], (i, res)
    assert abs(dist_exact(co[a, pa], Ka[pa], co[b, pb], Kb[pb], t) - sep) <= bound[0], (i, res)
    if need_pieces and fx["runner"][i] - ref > 2.0 * bound[0]:
        assert (pa, pb) == (fx["pa"][i], fx["pb"][i]), (i, res)
    return abs(sep - ref) / bound[0] if bound[0] > 0 else 0.0


# ---- the kernel's procedure in plain float64 --------------------------------------------------------------------------------
def _load(cm, T):
    cm = np.asarray(cm, dtype=np.float64)
    n = cm.shape[1] - 1
    with np.errstate(all="ignore"):
        tk = np.cumprod(np.r_[1.0, np.full(n, float(T))])
        u = cm[:, ::-1] * tk[None]
    ok = bool(np.all(np.isfinite(cm)) and np.all(np.isfinite(u)))
    z = np.stack([bnp.bernstein(u[ax]) for ax in range(3)]) if ok else None
    return ok, z, float(np.abs(u).sum()) if ok else 0.0


def _restrict(z, al, be):
    w = np.array(z, dtype=np.float64)
    n = len(w) - 1
    ob = 1.0 - be
    for r in range(1, n + 1):
        for k in range(n, r - 1, -1):
            w[k] = be * w[k] + ob * w[k - 1]
    ga = al / be
    og = 1.0 - ga
    for r in range(1, n + 1):
        for k in range(0, n - r + 1):
            w[k] = ga * w[k + 1] + og * w[k]
    return w


def _decast(d, sg, stop=0):
    """d (3, D) at sg by de Casteljau; stop = 1: the last two points of every axis"""
    w = np.array(d, dtype=np.float64)
    n = w.shape[1] - 1
    os_ = 1.0 - sg
    for r in range(1, n + 1 - stop):
        w[:, :n - r + 1] = sg * w[:, 1:n - r + 2] + os_ * w[:, :n - r + 1]
    return w[:, :1 + stop]


def separation_float64(co, T, t0, a, b, cutoff=np.inf, stats=None):
    """The kernel's procedure, step by step, in numpy float64 without fused operations, for the pair (a, b) of the batch co
    (B, N, 3, D), T (B, N), t0 (B,) or None -> (sep, t, piece_a, piece_b).  `stats`, a dict, receives: intervals, survivors
    (intervals refined), steps_out (the merge budget ran out), nodes_out, depth_out."""
    co = np.asarray(co, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    st = {"intervals": 0, "survivors": 0, "steps_out": 0, "nodes_out": 0, "depth_out": 0}
    if stats is not None:
        stats.update(st)
        st = stats
    B, N = T.shape
    if not (0 <= a < B and 0 <= b < B):
        return np.nan, 0.0, -1, -1
    D = co.shape[3]
    n = D - 1
    M = 2 * n
    K0a, K0b = (0.0, 0.0) if t0 is None else (float(t0[a]), float(t0[b]))
    with np.errstate(all="ignore"):
        KNa, KNb = knots(T[a], K0a)[-1], knots(T[b], K0b)[-1]
    if not (np.all(np.isfinite(T[[a, b]])) and np.all(T[[a, b]] >= 0.0) and np.all(np.isfinite([K0a, K0b, KNa, KNb]))):
        return np.nan, 0.0, -1, -1
    ia = ib = 0
    la = lb = -1
    Tia, Tib = float(T[a, 0]), float(T[b, 0])
    ka0, ka1, kb0, kb1 = K0a, K0a + Tia, K0b, K0b + Tib
    lo = max(K0a, K0b)
    best2, bestd, bt, bpa, bpb = np.inf, np.inf, 0.0, -1, -1
    za = zb = None
    Aa = Ab = 0.0
    step = 0
    while ia < N and ib < N:
        if step >= SEP_STEPS:
            st["steps_out"] += 1
            break
        step += 1
        if ka1 <= lo:
            ia += 1
            ka0 = ka1
            if ia < N:
                Tia = float(T[a, ia])
                ka1 = ka0 + Tia
            continue
        if kb1 <= lo:
            ib += 1
            kb0 = kb1
            if ib < N:
                Tib = float(T[b, ib])
                kb1 = kb0 + Tib
            continue
        hi = min(ka1, kb1)
        if la != ia:
            ok, za, Aa = _load(co[a, ia], Tia)
            la = ia
            if not ok:
                return np.nan, 0.0, -1, -1
        if lb != ib:
            ok, zb, Ab = _load(co[b, ib], Tib)
            lb = ib
            if not ok:
                return np.nan, 0.0, -1, -1
        st["intervals"] += 1
        ala, bea, alb, beb = (lo - ka0) / Tia, (hi - ka0) / Tia, (lo - kb0) / Tib, (hi - kb0) / Tib
        d = np.stack([_restrict(za[ax], ala, bea) - _restrict(zb[ax], alb, beb) for ax in range(3)])
        wid = hi - lo
        sc = Aa + Ab

        def candidate(sg):
            nonlocal best2, bestd, bt, bpa, bpb
            v = _decast(d, sg)[:, 0]
            d2 = float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            if d2 < best2:
                best2, bestd, bt, bpa, bpb = d2, float(np.sqrt(d2)), min(sg * wid + lo, hi), ia, ib
            return d2

        ub2 = min(candidate(k / (SEP_K - 1)) for k in range(SEP_K))
        Lh2 = float(np.sqrt((np.diff(d, axis=1) ** 2).sum(axis=0).max())) * (n * 0.5 / (SEP_K - 1))
        thr = min(bestd, cutoff) + Lh2 + SEP_SLACK * EPS * sc
        if ub2 < thr * thr * (1.0 + 8.0 * EPS):
            st["survivors"] += 1
            flat = (EPS * sc) ** 2
            dv = bnp.product_cv(d, d)
            lev, idx, done = 0, 0, False
            for _ in range(SEP_MAX_NODES):
                var, first, mx = bnp.sign_scan(bnp.descend(dv, lev, idx))
                width = 2.0 ** -lev
                l0 = idx * width
                mid = l0 + 0.5 * width
                split = False
                if var == 0:
                    pass
                elif 2.0 * n * mx * width <= flat:
                    candidate(mid)
                elif var == 1:
                    if first < 0:
                        l_, h_ = l0, l0 + width
                        for _it in range(SEP_BISECT):
                            mm = 0.5 * (l_ + h_)
                            if not (l_ < mm < h_):
                                break
                            v = _decast(d, mm, stop=1)
                            hm = float((((mm * v[:, 1] + (1.0 - mm) * v[:, 0]) * (v[:, 1] - v[:, 0]))).sum())
                            if hm < 0.0:
                                l_ = mm
                            else:
                                h_ = mm
                        candidate(l_)
                        candidate(h_)
                else:
                    candidate(mid)
                    split = lev < SEP_DEPTH
                    if not split:
                        st["depth_out"] += 1
                lev, idx, more = bnp.advance(lev, idx, split)
                if not more:
                    done = True
                    break
            if not done:
                st["nodes_out"] += 1
        lo = hi
    if bpa < 0:
        return np.inf, 0.0, -1, -1
    return float(np.sqrt(best2)), bt, bpa, bpb
