"""TEST INFRASTRUCTURE ONLY -- multiprecision reference for the trajectory post-processing kernels
(k_piece_max_rate, k_traj_eval, k_traj_cost) and the a-priori float64 error bounds their tests use.

A double is an exact rational, so every reference here starts from `fractions.Fraction(float)`, does its
algebra exactly (polynomial products, derivatives, integrals, square-free parts) and leaves the rationals only
where an irrational number appears: a root of a polynomial, a square root.  Those steps run in mpmath at DPS
digits.  Nothing here is rounded to double before the caller asks for it.

The `*_mp` functions need mpmath and sympy; the bound helpers (`rate_bound`, `eval_bound`, `cost_bound`,
`cost_grad_bound`) need numpy only, so GPU tests can import this module on a machine without mpmath and read
the references from tests/golden/max_rate_cases.npz (tests/golden/make_max_rate_golden.py writes it).

Conventions are the project's: a piece is cm (3, 2s), highest power first, with duration T.
"""
from fractions import Fraction as Fr

import numpy as np

try:
    import mpmath
    import sympy
except ImportError:      # the bound helpers still work
    mpmath = sympy = None

DPS = 60
EPS = float(np.finfo(np.float64).eps)       # DBL_EPSILON, the constant-rate threshold of trajectory.hpp:190
# K of the tolerances K * EPS * (sum of absolute terms); each docstring below derives its own
K_RATE, K_EVAL, K_COST = 32, 16, 32


def _fall(k, j):
    r = 1
    for i in range(j):
        r *= (k - i)
    return r


def _need_mp():
    if mpmath is None:
        raise RuntimeError("trajectory_mp: mpmath and sympy are needed for the multiprecision reference")
    mpmath.mp.dps = DPS


# ---- exact polynomial algebra on ascending lists of Fractions --------------------------------------------
def _pmul(a, b):
    out = [Fr(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def _padd(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else Fr(0)) + (b[i] if i < len(b) else Fr(0)) for i in range(n)]


def _pder(a, times=1):
    for _ in range(times):
        a = [k * a[k] for k in range(1, len(a))] or [Fr(0)]
    return a


def _pval(a, x):
    v = 0
    for c in reversed(a):
        v = v * x + c
    return v


def _mpf(x):
    """Fraction -> mpf at the working precision."""
    return mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator)


# ---- max rate ---------------------------------------------------------------------------------------------
def normalized_deriv_exact(cm, T, which):
    """u[ax][k], k ascending: the exact coefficients of d^which P / dtau^which, P(tau) = p(T tau) -- what
    normalizeVelCoeffMat / normalizeAccCoeffMat (trajectory.hpp:147-175) and the kernel's u[ax][k] round."""
    cm = np.asarray(cm, dtype=np.float64)
    Dg = cm.shape[1] - 1
    Tq = Fr(float(T))
    return [[_fall(k + which, which) * Fr(float(cm[ax, Dg - (k + which)])) * Tq ** (k + which)
             for k in range(Dg - which + 1)] for ax in range(3)]


def _q_exact(cm, T, which):
    q = [Fr(0)]
    for ua in normalized_deriv_exact(cm, T, which):
        q = _padd(q, _pmul(ua, ua))
    return q


def dq_norm_mp(cm, T, which):
    """Squared coefficient norm of d/dtau ||d^which P/dtau^which||^2, exact (a Fraction): the number
    trajectory.hpp:190,239 and the kernel compare with DBL_EPSILON."""
    return sum((c * c for c in _pder(_q_exact(cm, T, which))), Fr(0))


def const_branch_rate_mp(cm, T, which):
    """The rate at t = 0, getVel(0).norm() / getAcc(0).norm(): what the constant-rate branch returns."""
    _need_mp()
    q = _q_exact(cm, T, which)
    return mpmath.sqrt(_mpf(q[0])) / _mpf(Fr(float(T))) ** which


def dq_roots_mp(cm, T, which):
    """Real roots in [0, 1] of dq/dtau, as mpf, each once.  The square-free part is taken over QQ, so a multiple
    root is simple in what polyroots sees (plain polyroots does not converge on a multiple root); the number of
    roots it must deliver in [0, 1] is counted with Sturm sequences on the same exact polynomial."""
    _need_mp()
    dq = _pder(_q_exact(cm, T, which))
    while len(dq) > 1 and dq[-1] == 0:
        dq.pop()
    if len(dq) <= 1:
        return []
    x = sympy.Symbol("x")
    P = sympy.Poly([sympy.Rational(c.numerator, c.denominator) for c in reversed(dq)], x, domain="QQ")
    sq = P.sqf_part()
    want = sq.count_roots(0, 1)
    if sq.degree() < 1 or want == 0:
        return []
    co = [mpmath.mpf(int(c.p)) / mpmath.mpf(int(c.q)) for c in sq.all_coeffs()]
    lead = co[0]
    co = [c / lead for c in co]
    with mpmath.workdps(2 * DPS):
        rts = mpmath.polyroots(co, maxsteps=2000, extraprec=8 * DPS)
    tol = mpmath.mpf(10) ** (-DPS + 10)
    real = sorted(r.real for r in map(mpmath.mpmathify, rts)
                  if abs(mpmath.im(r)) <= tol and -tol <= mpmath.re(r) <= 1 + tol)
    real = [min(max(mpmath.mpf(r), mpmath.mpf(0)), mpmath.mpf(1)) for r in real]
    assert len(real) == want, (len(real), want)
    return real


def piece_max_rate_mp(cm, T, which):
    """max over [0, T] of ||d^which p/dt^which||: sqrt(max q) / T^which over the candidates {0, 1} and the real
    roots of q' in [0, 1] (normalised time; q = T^(2 which) ||.||^2, exact)."""
    _need_mp()
    q = [_mpf(c) for c in _q_exact(cm, T, which)]
    best = max(_pval(q, t) for t in [mpmath.mpf(0), mpmath.mpf(1)] + dq_roots_mp(cm, T, which))
    return mpmath.sqrt(max(best, 0)) / _mpf(Fr(float(T))) ** which


def modelled_max_rate_mp(cm, T, which):
    """What Piece::getMaxVelRate / getMaxAccRate (trajectory.hpp:177-273) returns in exact arithmetic: the true
    maximum, except below the DBL_EPSILON threshold on dq_norm_mp, where it is the rate at t = 0."""
    if dq_norm_mp(cm, T, which) < Fr(EPS):
        return const_branch_rate_mp(cm, T, which)
    return piece_max_rate_mp(cm, T, which)


def rate_A(cm, T, which):
    """A = sqrt(sum_ax (sum_k |u_ax,k|)^2) from the exact u, rounded once: the scale of the max-rate bound."""
    _need_mp()
    u = normalized_deriv_exact(cm, T, which)
    return float(mpmath.sqrt(_mpf(sum((sum((abs(c) for c in ua), Fr(0)) ** 2 for ua in u), Fr(0)))))


def rate_bound(A, T, which):
    """|rate_float64 - rate| <= K_RATE * EPS * A / T^which for a method that evaluates the candidates from the
    component polynomials u_ax (as getVel(t).squaredNorm() does).  Per component the absolute error is at most
    c * EPS * sum_k |u_ax,k|: Horner on degree m <= 6 gives 2m <= 12, forming u_k = c_k * T^k * falling factor at
    most 10 roundings (T^k by repeated products, k <= 7, and two products); the Euclidean norm is 1-Lipschitz, so
    the three component errors enter as c * EPS * A, also where the components cancel; squares, sum, square root
    and the scaling by T^-which add at most 4.  12 + 10 + 4 = 26, rounded up to the power of two 32.  The error of
    a root's location enters to second order only (q' = 0 there)."""
    return K_RATE * EPS * np.asarray(A, dtype=np.float64) / np.asarray(T, dtype=np.float64) ** which


# ---- evaluation -------------------------------------------------------------------------------------------
def locate(T, t):
    """Trajectory::locatePieceIdx (trajectory.hpp:496-514) in the double arithmetic it is written in: which piece
    a query lands in is part of the modelled behaviour (the pieces of a test trajectory need not join)."""
    N = len(T)
    t = float(t)
    idx = 0
    while idx < N and t > float(T[idx]):
        t -= float(T[idx])
        idx += 1
    if idx == N:
        idx -= 1
        t += float(T[idx])
    return idx, t


def traj_eval_mp(coeffs, T, t, d):
    """d-th derivative at absolute time t: piece location as above, then the exact polynomial at the located
    local time (a double, hence exact).  Returns three Fractions."""
    idx, tl = locate(T, t)
    cm = np.asarray(coeffs[idx], dtype=np.float64)
    Dg = cm.shape[1] - 1
    tq = Fr(tl)
    return [sum((_fall(k, d) * Fr(float(cm[ax, Dg - k])) * tq ** (k - d) for k in range(d, Dg + 1)), Fr(0))
            for ax in range(3)]


def eval_bound(coeffs, T, t, d):
    """Per axis K_EVAL * EPS * sum_k |w_k c_k t^(k-d)|, w_k the falling factor.  The kernel and getPos/getVel/...
    accumulate ascending powers with tn *= t: t^j costs j - 1 <= 6 roundings, the falling factor times tn one, the
    product with c_k one, and a term passes through at most 7 additions: 15, rounded up to 16."""
    idx, tl = locate(T, t)
    cm = np.asarray(coeffs[idx], dtype=np.float64)
    Dg = cm.shape[1] - 1
    mag = np.zeros(3)
    for k in range(d, Dg + 1):
        mag += _fall(k, d) * np.abs(cm[:, Dg - k]) * abs(tl) ** (k - d)
    return K_EVAL * EPS * mag


# ---- cost and its duration gradient -----------------------------------------------------------------------
def _piece_cost_exact(cm, T, s, m34):
    cm = np.asarray(cm, dtype=np.float64)
    Dg = cm.shape[1] - 1
    Tq, cost, grad = Fr(float(T)), Fr(0), Fr(0)
    for ax in range(3):
        asc = [Fr(float(cm[ax, Dg - k])) for k in range(Dg + 1)]
        ds = _pder(asc, s)
        sq = _pmul(ds, ds)
        cost += sum((c * Tq ** (k + 1) / (k + 1) for k, c in enumerate(sq)), Fr(0)) / 2
        grad += _pval(sq, Tq) / 2
        if s == 4:
            z2z3 = Fr(float(cm[ax, 2])) * Fr(float(cm[ax, 3]))
            cost += (Fr(float(m34)) - 1440) * Tq ** 2 * z2z3
            grad += 2 * (Fr(float(m34)) - 1440) * Tq * z2z3
    return cost, grad


def traj_cost_mp(coeffs, T, s, m34=1440.0):
    """Trajectory::getTrajCost: sum over the pieces of 1/2 int_0^T ||p^(s)||^2 dt, integrated exactly, plus for s = 4
    the (m34 - 1440) T^2 z_2 z_3 per axis by which the reference's constant 1400 differs from the integral's 1440."""
    return sum((_piece_cost_exact(coeffs[i], T[i], s, m34)[0] for i in range(len(T))), Fr(0))


def traj_cost_grad_T_mp(coeffs, T, s, m34=1440.0):
    """Its exact derivative in each T_i at fixed coefficients: 1/2 ||p_i^(s)(T_i)||^2 (+ the m34 term)."""
    return [_piece_cost_exact(coeffs[i], T[i], s, m34)[1] for i in range(len(T))]


def cost_blocks(s, t, m34):
    """Q and dQ/dt of the s x s cost block on the s highest coefficients, from the integral's own formula (entrywise
    non-negative for t > 0 and m34 > 0, so they are also the |Q|, |dQ| of the bounds; float64 is ample for those)."""
    Q = np.zeros((s, s)); dQ = np.zeros((s, s))
    for j in range(s):
        for k in range(s):
            a, b = 2 * s - 1 - j, 2 * s - 1 - k               # powers of the two coefficients
            e = a + b - 2 * s + 1
            c = _fall(a, s) * _fall(b, s) / e
            if s == 4 and {j, k} == {2, 3}:
                c = float(m34)
            Q[j, k] = c * t ** e
            dQ[j, k] = c * e * t ** (e - 1)
    return Q, dQ


def cost_bound(coeffs, T, s, m34):
    """K_COST * EPS * sum over pieces and axes of 1/2 sum_jk |z_j| |Q_jk| |z_k|.  Roundings a term of the kernel's sum
    passes: the power of t (t7 = t4 * t3: 6), its constant 1, Q z_k 1, the row sum <= 4, z_j times the row 1, the sum
    over rows <= 4, the sum over 3 axes x 3 pieces 9: 26, rounded up to 32."""
    tot = 0.0
    for i in range(len(T)):
        Q, _ = cost_blocks(s, float(T[i]), m34)
        for ax in range(3):
            z = np.abs(np.asarray(coeffs[i], dtype=np.float64)[ax, :s])
            tot += 0.5 * z @ Q @ z
    return K_COST * EPS * tot


def cost_grad_bound(coeffs, T, s, m34):
    """Per piece K_COST * EPS * sum over axes of 1/2 sum_jk |z_j| |dQ_jk| |z_k|: as cost_bound with the power of t one
    lower (5) and the sum over 3 axes only (3): 19, rounded up to 32."""
    out = np.zeros(len(T))
    for i in range(len(T)):
        _, dQ = cost_blocks(s, float(T[i]), m34)
        for ax in range(3):
            z = np.abs(np.asarray(coeffs[i], dtype=np.float64)[ax, :s])
            out[i] += 0.5 * z @ dQ @ z
    return K_COST * EPS * out
