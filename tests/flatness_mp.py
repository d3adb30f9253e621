"""TEST INFRASTRUCTURE ONLY -- multiprecision reference for the flatness kernels of csrc/flatness_kernels.h (k_flat_forward,
k_flat_backward, k_traj_flat_states, k_traj_flat_extrema, k_flat_piece_grad) and the a-priori float64 error bound their
tests use.  Written from the formulas in that header's comment; it shares nothing with tests/flatness_np.py or the product.

    w   = (1 + cp sqrt(|v|^2 + eps)) v
    zu  = a + (dh/m) w + g e3,            z = zu / |zu|
    u   = j + (dh/m) dw/dt,               dz = (I - z z^T) u / |zu|
    thr = z . (m a + dv w + m g e3)
    q   = tilt(z) * yaw(psi),             tilt(z) = (d/2, -z2/d, z1/d, 0), d = sqrt(2 (1 + z3))
    omg = vector part of 2 conj(q) * dq/dt,   dq/dt = dtilt/dt * yaw + tilt * dyaw/dt      (the definition of a body rate)

A double is an exact rational, so every input enters as mpf(double) exactly and all arithmetic runs in mpmath at DPS digits.
No adjoint is derived by hand: every derivative is a central difference at working precision (step H, error about H^2),
and the derivatives of derivatives that the scales need are differences of those with the step H2.

THE SCALE.  For one output y of a map with inputs and parameters x_l
    scale(y) = mag(y) + sum_l |dy/dx_l| |x_l|
mag(y) is the sum of the absolute values of the exact terms whose sum y is (one term: |y|).  An algorithm that rounds its
inputs, its parameters and each term once has the error eps * scale to first order; where y is ill conditioned in an input
(free fall: 1 / |zu|) the scale grows with it.  The scale comes from the reference alone.

THE BOUND.  |got - ref| <= K eps scale (1 + 1/delta), delta = 1 + z3 (the smallest over the samples of a piece or a
trajectory).  The factor 1/delta is the price of forming 1 + z3 from a rounded z3: the sum carries the relative error
eps/delta, and d, 1/(1 + z3) and everything downstream inherit it.  K counts roundings along the longest path of the
kernel (see the K_* below and DESIGN.md 8f, "Accuracy").

The `*_mp` functions need mpmath; `flat_bound`, `load` and the K_* need numpy only, so GPU tests import this module on a
machine without mpmath and read everything else from tests/golden/flatness_cases.npz (tests/golden/make_flatness_golden.py).

Conventions are the project's: a piece is cm (3, 2s), highest power first, with duration T; par = (mass, grav, dh, dv, cp,
eps); pen = (w_thr, w_tilt, w_bdr, mu, thr_min, thr_max, tilt_max, bdr_max, res) as anet_flat_penalty.
"""
import os

import numpy as np

try:
    import mpmath
    from mpmath import mpf
except ImportError:      # the bound helper and the loader still work
    mpmath = mpf = None

DPS = 70
H_EXP, H2_EXP = -25, -15          # steps 10^H_EXP of the derivatives, 10^H2_EXP of the derivatives of derivatives
EPS = float(np.finfo(np.float64).eps)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flatness_cases.npz")

# Roundings along the longest path, FMA = 1, a divide, a square root, sincos and atan2 = 1 each (correctly rounded or 1 ulp):
#   flat_forward   v -> |v|^2 (3) + eps (1), sqrt (1), wt (1), w (1), zu (1), + g (1), |zu|^2 (3), sqrt, 1/ (2), z (1): 16;
#                  z -> z.u (3), dz (2): 21; 1 + z3, 1/ (2), ot (1): 24; A ot, o0 (4): 28.  The path through dwt
#                  (s: 5, v.a cp / s: 5, u: 3) joins z.u at 13 < 16.  thr and q end earlier (20, 22).        28 -> K = 32
#   flat_adjoint   the forward's 24 to (z, dz, ot, iod), then ob -> otb (3), dzb (1), rb (1), rb.z (3), ub (1), dwb (1),
#                  dwb.v (3), vab / sb (2), sb fma (1), sbs (1), vb (4): 21.                                 45 -> K = 64
#   states/extrema the query's v, a, j as k_traj_eval (15, trajectory_mp.eval_bound), the forward (28), the tilt from q
#                  (squares and sums 3 + 3, two square roots, atan2, the doubling: 10 from q at 22 = 32 < 43).  43 -> K = 64
#   piece penalty  c~ = c T^k (7 + 1), a state row (8 fmas) times T^-d (rT3: 3, product 1): 20; forward and adjoint (45);
#                  the penalty row between them (argument 2, smoothed_l1 5, weight 2): 9; one sample's gradient update 3,
#                  res <= 4 samples: + 3; (T / res) T^k (8) and the product (1): 9; accumulate 1.            90 -> K = 128
K_FWD, K_ADJ, K_TRAJ, K_PIECE = 32, 64, 64, 128

OUT_NAMES = ("thr", "q0", "q1", "q2", "q3", "o0", "o1", "o2", "z0", "z1", "z2", "tilt", "speed", "bdr")
N_MAP = 8                 # thr, quat, omg: the outputs the adjoint takes upstream gradients of
IN_NAMES = ("v0", "v1", "v2", "a0", "a1", "a2", "j0", "j1", "j2", "psi", "dpsi")
PAR_NAMES = ("mass", "grav", "dh", "dv", "cp", "eps")
LAUNCH = (1.0, 9.8, 0.7, 0.8, 0.01, 1e-4)      # the launch file's vehicle


# ---- numpy only ---------------------------------------------------------------------------------------------
def flat_bound(scale, delta, K):
    """K eps scale (1 + 1/delta), elementwise; delta broadcasts against scale."""
    return K * EPS * np.asarray(scale, dtype=np.float64) * (1.0 + 1.0 / np.asarray(delta, dtype=np.float64))


def load(path=FIXTURE):
    """The fixture as a dict of arrays (family names as str)."""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def spare(got, ref, scale, delta, K):
    """Worst |got - ref| / bound over the entries; entries with a zero bound must be equal (then 0, else inf)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bnd = np.broadcast_to(flat_bound(scale, delta, K), ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0.0, err / bnd, np.where(err == 0.0, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max()) if r.size else 0.0


# ---- the map ------------------------------------------------------------------------------------------------
def _need_mp():
    if mpmath is None:
        raise RuntimeError("flatness_mp: mpmath is needed for the multiprecision reference")
    mpmath.mp.dps = DPS


def _m(x):
    return [mpf(float(t)) for t in np.asarray(x, dtype=np.float64).ravel()]


def _dot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def _qmul_terms(p, q):
    """Hamilton product as its sixteen signed products, four per component."""
    return [[p[0] * q[0], -p[1] * q[1], -p[2] * q[2], -p[3] * q[3]],
            [p[0] * q[1], p[1] * q[0], p[2] * q[3], -p[3] * q[2]],
            [p[0] * q[2], -p[1] * q[3], p[2] * q[0], p[3] * q[1]],
            [p[0] * q[3], p[1] * q[2], -p[2] * q[1], p[3] * q[0]]]


def _sum_terms(terms):
    return [sum(t) for t in terms], [sum(abs(x) for x in t) for t in terms]


def forward_mp(x, par):
    """x: the 11 inputs (IN_NAMES) as mpf, par the 6 parameters as mpf -> (Y, mag, delta): the 14 outputs OUT_NAMES, the sums
    of their absolute terms, and delta = 1 + z3.  The tilt is atan2(|z_xy|, z3), exact at hover and at inversion."""
    v, a, j, psi, dpsi = x[0:3], x[3:6], x[6:9], x[9], x[10]
    mass, grav, dh, dv, cp, eps = par
    dhm = dh / mass
    vv = _dot(v, v)
    s = mpmath.sqrt(vv + eps)
    wt = 1 + cp * s
    w = [wt * t for t in v]
    dwt = cp * _dot(v, a) / s
    dw = [wt * a[k] + dwt * v[k] for k in range(3)]
    zu = [a[k] + dhm * w[k] for k in range(3)]
    zu[2] += grav
    L = mpmath.sqrt(_dot(zu, zu))
    z = [t / L for t in zu]
    u = [j[k] + dhm * dw[k] for k in range(3)]
    zdu = _dot(z, u)
    dz = [(u[k] - z[k] * zdu) / L for k in range(3)]
    f = [mass * a[k] + dv * w[k] for k in range(3)]
    f[2] += mass * grav
    thr_terms = [z[k] * f[k] for k in range(3)]
    delta = 1 + z[2]
    d = mpmath.sqrt(2 * delta)
    tl = [d / 2, -z[1] / d, z[0] / d, mpf(0)]
    dtl = [dz[2] / (2 * d), -dz[1] / d + z[1] * dz[2] / d ** 3, dz[0] / d - z[0] * dz[2] / d ** 3, mpf(0)]
    ch, sh = mpmath.cos(psi / 2), mpmath.sin(psi / 2)
    yw = [ch, mpf(0), mpf(0), sh]
    dyw = [-sh * dpsi / 2, mpf(0), mpf(0), ch * dpsi / 2]
    q, qmag = _sum_terms(_qmul_terms(tl, yw))
    qd = [p + r for p, r in zip(*[_sum_terms(_qmul_terms(*pr))[0] for pr in ((dtl, yw), (tl, dyw))])]
    conj = [q[0], -q[1], -q[2], -q[3]]
    om, ommag = _sum_terms([[2 * t for t in row] for row in _qmul_terms(conj, qd)])
    tilt = mpmath.atan2(mpmath.sqrt(z[0] * z[0] + z[1] * z[1]), z[2])
    bdr = mpmath.sqrt(_dot(om[1:], om[1:]))
    Y = [sum(thr_terms)] + q + om[1:] + z + [tilt, mpmath.sqrt(vv), bdr]
    mag = [sum(abs(t) for t in thr_terms)] + qmag + ommag[1:] + [abs(t) for t in z] + [abs(tilt), mpmath.sqrt(vv), bdr]
    return Y, mag, delta


def _step(exp):
    return mpf(10) ** exp


def jacobian_mp(x, par, n_out=N_MAP, cols=None):
    """d Y_i / d x_l, i < n_out, by central differences; cols: which of the 11 inputs (default all)."""
    h = _step(H_EXP)
    cols = range(len(x)) if cols is None else cols
    J = [[mpf(0)] * len(x) for _ in range(n_out)]
    for l in cols:
        xp, xm = list(x), list(x)
        xp[l] += h
        xm[l] -= h
        Yp, Ym = forward_mp(xp, par)[0], forward_mp(xm, par)[0]
        for i in range(n_out):
            J[i][l] = (Yp[i] - Ym[i]) / (2 * h)
    return J


def adjoint_mp(x, par, g):
    """J^T g for the upstream gradients g of (thr, q0..q3, o0..o2) -> (gx, mag): the 11 gradients w.r.t. IN_NAMES and the sums
    of the absolute values of their terms g_i dY_i/dx_l."""
    J = jacobian_mp(x, par)
    gx = [sum(g[i] * J[i][l] for i in range(N_MAP)) for l in range(len(x))]
    mag = [sum(abs(g[i] * J[i][l]) for i in range(N_MAP)) for l in range(len(x))]
    return gx, mag


def _scale_of(fun, xs, vals, mags, h):
    """mags + sum_l |d fun / d xs_l| |xs_l| by central differences with the step h; entries of xs that are zero add nothing."""
    sc = list(mags)
    for l, xl in enumerate(xs):
        if xl == 0:
            continue
        xp, xm = list(xs), list(xs)
        xp[l] += h
        xm[l] -= h
        fp, fm = fun(xp), fun(xm)
        for i in range(len(sc)):
            sc[i] += abs((fp[i] - fm[i]) / (2 * h)) * abs(xl)
    return sc


def pointwise_mp(v, a, j, psi, dpsi, par, g):
    """One pointwise case in doubles -> dict of doubles: the 14 forward outputs `fwd` with their scales `fwd_scale`, the 11
    adjoint outputs `adj` (J^T g) with `adj_scale`, and delta.  psi = dpsi = None is psi = dpsi = 0."""
    _need_mp()
    x = _m(v) + _m(a) + _m(j) + [mpf(float(psi or 0.0)), mpf(float(dpsi or 0.0))]
    p = _m(par)
    gm = _m(g)
    Y, mag, delta = forward_mp(x, p)
    gx, gmag = adjoint_mp(x, p, gm)
    n = len(x)
    fsc = _scale_of(lambda xs: forward_mp(xs[:n], xs[n:])[0], x + p, Y, mag, _step(H_EXP))
    asc = _scale_of(lambda xs: adjoint_mp(xs[:n], xs[n:], gm)[0], x + p, gx, gmag, _step(H2_EXP))
    f = lambda t: np.array([float(u) for u in t])
    return dict(fwd=f(Y), fwd_scale=f(fsc), adj=f(gx), adj_scale=f(asc), delta=float(delta))


# ---- along a polynomial piece -------------------------------------------------------------------------------
def _fall(k, d):
    r = 1
    for i in range(d):
        r *= (k - i)
    return r


def _basis(D, t, d):
    """row of d^d/dt^d (t^k), column col holds the power k = D - 1 - col"""
    return [(_fall(D - 1 - col, d) * t ** (D - 1 - col - d)) if D - 1 - col >= d else mpf(0) for col in range(D)]


def _derivs(cm, t, dmax):
    """cm[ax][col] mpf -> [p, v, a, ...][d][ax] at local time t, and the basis rows"""
    D = len(cm[0])
    rows = [_basis(D, t, d) for d in range(dmax + 1)]
    return [[sum(c * b for c, b in zip(cm[ax], rows[d])) for ax in range(3)] for d in range(dmax + 1)], rows


def state_mp(cm, t, par):
    """The 14 outputs at local time t of one piece (psi = dpsi = 0), their scales and delta.  The perturbed quantities are
    the 6s coefficients, t and the parameters; the chain through the polynomial is exact, the map's part by differences."""
    _need_mp()
    cmm = [_m(r) for r in np.asarray(cm, dtype=np.float64)]
    tm, p = (t if isinstance(t, mpf) else mpf(float(t))), _m(par)
    d, rows = _derivs(cmm, tm, 4)
    x = d[1] + d[2] + d[3] + [mpf(0), mpf(0)]
    Y, mag, delta = forward_mp(x, p)
    n_out = len(Y)
    J = jacobian_mp(x, p, n_out=n_out, cols=range(9))
    sc = _scale_of(lambda ps: forward_mp(x, ps)[0], p, Y, mag, _step(H_EXP))
    for i in range(n_out):
        for ax in range(3):
            for col in range(len(cmm[0])):
                sc[i] += abs(sum(J[i][3 * k + ax] * rows[k + 1][col] for k in range(3)) * cmm[ax][col])
        sc[i] += abs(sum(J[i][3 * k + ax] * d[k + 2][ax] for k in range(3) for ax in range(3)) * tm)
    f = lambda u: np.array([float(w) for w in u])
    return f(Y), f(sc), float(delta)


# ---- the penalty of one piece -------------------------------------------------------------------------------
def smoothed_l1_mp(x, mu):
    """firi::smoothedL1: 0 below 0, (mu - x/2) (x/mu)^3 up to mu, x - mu/2 above."""
    if x < 0:
        return mpf(0)
    if x > mu:
        return x - mu / 2
    return (mu - x / 2) * (x / mu) ** 3


def _sample_penalty(xs, par, w, lim, mu, knobs):
    """Phi of one sample: xs = v, a, j (9); lim = (thr_min, thr_max, cos_tilt_max, bdr_max^2); knobs multiply thr, cos tilt and
    |omg|^2 (all 1: the relative perturbations of the three quantities the rows compare with their limits)."""
    Y, _, delta = forward_mp(list(xs) + [mpf(0), mpf(0)], par)
    thr, ct, b2 = knobs[0] * Y[0], knobs[1] * Y[10], knobs[2] * _dot(Y[5:8], Y[5:8])
    phi = (w[0] * (smoothed_l1_mp(thr - lim[1], mu) + smoothed_l1_mp(lim[0] - thr, mu))
           + w[1] * smoothed_l1_mp(lim[2] - ct, mu) + w[2] * smoothed_l1_mp(b2 - lim[3], mu))
    return phi, delta, (thr, ct, b2)


def _piece_core(cm, T, par, w, lim, mu, knobs, res):
    """(values, mags, delta_min, samples): values = [pc, gC (3 D, axis-major), gT]."""
    D = len(cm[0])
    h = _step(H_EXP)
    step = T / res
    pc, gC, gCm = mpf(0), [mpf(0)] * (3 * D), [mpf(0)] * (3 * D)
    gT_terms, dmin, samples = [], None, []
    for jj in range(res):
        tau = mpf(jj) / res
        d, rows = _derivs(cm, tau * T, 4)
        xs = d[1] + d[2] + d[3]
        phi, delta, vals = _sample_penalty(xs, par, w, lim, mu, knobs)
        dmin = delta if dmin is None or delta < dmin else dmin
        samples.append(vals)
        pc += step * phi
        gT_terms.append(phi / res)
        if phi == 0:
            # phi is identically zero in a neighbourhood (all four arguments negative) unless an argument is exactly 0
            continue
        grad = []
        for l in range(9):
            xp, xm = list(xs), list(xs)
            xp[l] += h
            xm[l] -= h
            grad.append((_sample_penalty(xp, par, w, lim, mu, knobs)[0] - _sample_penalty(xm, par, w, lim, mu, knobs)[0]) / (2 * h))
        for k in range(3):
            for ax in range(3):
                gb = grad[3 * k + ax]
                for col in range(D):
                    t = step * gb * rows[k + 1][col]
                    gC[ax * D + col] += t
                    gCm[ax * D + col] += abs(t)
                gT_terms.append(step * tau * gb * d[k + 2][ax])
    vals = [pc] + gC + [sum(gT_terms)]
    mags = [pc] + gCm + [sum(abs(t) for t in gT_terms)]
    return vals, mags, dmin, samples


def pen_limits_mp(pen):
    """(w, lim, mu, res) in mpf from the API's penalty tuple: the kernel compares with cos(tilt_max) and bdr_max^2."""
    w_thr, w_tilt, w_bdr, mu, thr_min, thr_max, tilt_max, bdr_max, res = pen
    m = lambda t: mpf(float(t))
    return [m(w_thr), m(w_tilt), m(w_bdr)], [m(thr_min), m(thr_max), mpmath.cos(m(tilt_max)), m(bdr_max) ** 2], m(mu), int(res)


def piece_penalty_mp(cm, T, par, pen, scales=True):
    """J_flat of one piece as defined at k_flat_piece_grad (samples at tau_j = j / res, j < res, psi = dpsi = 0, cos tilt = z3)
    and its exact partials at fixed coefficients -> dict of doubles: pc, gC (3, D), gT, their scales, delta (smallest over
    the samples) and `samples` (res, 3): thr, cos tilt, |omg|^2.  The scale perturbs the coefficients, T, the parameters, the
    four limits the kernel holds, mu, and the three compared quantities themselves."""
    _need_mp()
    cmm = [_m(r) for r in np.asarray(cm, dtype=np.float64)]
    D = len(cmm[0])
    w, lim, mu, res = pen_limits_mp(pen)
    ones = [mpf(1)] * 3
    vals, mags, dmin, samples = _piece_core(cmm, mpf(float(T)), _m(par), w, lim, mu, ones, res)
    f = lambda u: np.array([float(t) for t in u])
    out = dict(pc=float(vals[0]), gC=f(vals[1:-1]).reshape(3, D), gT=float(vals[-1]), delta=float(dmin),
               samples=np.array([[float(t) for t in s] for s in samples]))
    if scales:
        flat = [c for r in cmm for c in r] + [mpf(float(T))] + _m(par) + lim + [mu] + ones

        def fun(xs):
            c = [xs[ax * D:(ax + 1) * D] for ax in range(3)]
            o = 3 * D
            return _piece_core(c, xs[o], xs[o + 1:o + 7], w, xs[o + 7:o + 11], xs[o + 11], xs[o + 12:o + 15], res)[0]
        sc = f(_scale_of(fun, flat, vals, mags, _step(H2_EXP))) if vals[0] != 0 else np.zeros(len(vals))
        out.update(pc_scale=float(sc[0]), gC_scale=sc[1:-1].reshape(3, D), gT_scale=float(sc[-1]))
    return out
