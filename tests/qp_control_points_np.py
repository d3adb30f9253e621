"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the control-point row form of the inequality QP
(ANET_QP_ROWS_CONTROL_POINTS), written independently of the kernels: exact rational arithmetic
(fractions / math.comb) for the functionals, the shifted monomial expanded outright -- what the device code must not do in
floating point is harmless in exact arithmetic -- and floats only at the very end.

Group j = q D + r of a piece (D = 2s, res = K D): segment q = [q T / K, (q + 1) T / K], control index r.  beta^d_r is the r-th
of the D values obtained from the Bernstein control values of p^(d) on that segment (degree D - 1 - d) by d degree elevations."""
import functools
from fractions import Fraction
from math import comb

import numpy as np


def _falling(k, d):
    v = 1
    for e in range(d):
        v *= k - e
    return v


@functools.lru_cache(maxsize=None)
def functional_exact(s, d, q, K):
    """W[r][k] (Fractions): beta^d_r on segment q of K, in normalised time, of the monomial tau^k."""
    D = 2 * s
    n = D - 1 - d
    a, h = Fraction(q, K), Fraction(1, K)
    W = [[Fraction(0)] * D for _ in range(D)]
    for k in range(d, D):
        e = k - d
        # d-th derivative of tau^k at tau = a + h sigma, ascending in the segment's own parameter sigma in [0, 1]
        mono = [_falling(k, d) * comb(e, j) * a ** (e - j) * h ** j for j in range(e + 1)] + [Fraction(0)] * (n - e)
        bern = [sum(Fraction(comb(i, j), comb(n, j)) * mono[j] for j in range(i + 1)) for i in range(n + 1)]
        for nn in range(n, D - 1):          # degree nn -> nn + 1
            bern = ([bern[0]] + [Fraction(i, nn + 1) * bern[i - 1] + (1 - Fraction(i, nn + 1)) * bern[i] for i in range(1, nn + 1)]
                    + [bern[nn]])
        for r in range(D):
            W[r][k] = bern[r]
    return W


@functools.lru_cache(maxsize=None)
def functional(s, d, q, K):
    """functional_exact as a float (D, D) array [r, k]."""
    return np.array([[float(x) for x in row] for row in functional_exact(s, d, q, K)])


def row_functional(s, d, q, K, r, T):
    """The row on ONE axis' coefficients in the reference's unknowns (real time, highest power first): (D,)."""
    D = 2 * s
    w = functional(s, d, q, K)[r]
    out = np.zeros(D)
    for col in range(D):
        k = D - 1 - col
        if k >= d:
            out[col] = w[k] * float(T) ** (k - d)
    return out


def control_values(coef, T, s, K, d):
    """coef (3, D) highest power first, real time -> beta^d (K D, 3): row j = q D + r."""
    D = 2 * s
    out = np.zeros((K * D, 3))
    for q in range(K):
        for r in range(D):
            out[q * D + r] = np.asarray(coef) @ row_functional(s, d, q, K, r, T)
    return out


BOX_ROWS = [(ax, w) for ax in range(3) for w in range(4)]     # per axis: +v, +a, -v, -a (qp_solver.hpp:280-291)


def dense_G_h(s, polys, T, K, max_vel, max_acc, row_order=0):
    """G (m_g, n), h (m_g,) of the control-point form.  polys: a list of N arrays (m_i, 4) (zero rows are rows like any other,
    as in the sample form); T (N,); row_order 0 = ORDER_CPP (per piece, per group: the corridor rows, then 12 box rows),
    1 = ORDER_PYTHON (all corridor rows, then all box rows)."""
    D = 2 * s
    N = len(polys)
    res = K * D
    n = 3 * D * N

    def corridor(i, j):
        w = row_functional(s, 0, j // D, K, j % D, T[i])
        out = []
        for a in np.asarray(polys[i], dtype=np.float64).reshape(-1, 4):
            g = np.zeros(n)
            for ax in range(3):
                g[i * 3 * D + ax * D:i * 3 * D + (ax + 1) * D] = a[ax] * w
            out.append((g, a[3]))
        return out

    def boxes(i, j):
        out = []
        for ax, w in BOX_ROWS:
            d = 1 + (w & 1)
            g = np.zeros(n)
            g[i * 3 * D + ax * D:i * 3 * D + (ax + 1) * D] = (1.0 if w < 2 else -1.0) * row_functional(s, d, j // D, K, j % D, T[i])
            out.append((g, max_acc if (w & 1) else max_vel))
        return out
    rows = []
    if row_order == 0:
        for i in range(N):
            for j in range(res):
                rows += corridor(i, j) + boxes(i, j)
    else:
        for i in range(N):
            for j in range(res):
                rows += corridor(i, j)
        for i in range(N):
            for j in range(res):
                rows += boxes(i, j)
    G = np.array([g for g, _ in rows]).reshape(len(rows), n)
    h = np.array([hv for _, hv in rows], dtype=np.float64)
    return G, h


def row_groups(polys, res):
    """For ORDER_CPP rows: (piece (m_g,), kind (m_g,)) with kind 0 corridor, 1 velocity box, 2 acceleration box."""
    piece, kind = [], []
    for i, p in enumerate(polys):
        m = np.asarray(p).reshape(-1, 4).shape[0]
        for _ in range(res):
            piece += [i] * (m + 12)
            kind += [0] * m + [1 + (w & 1) for _, w in BOX_ROWS]
    return np.array(piece), np.array(kind)


def bernstein_eval(beta, sigma):
    """sum_r B_r^(D-1)(sigma) beta[r]: beta (D, ...) -> (len(sigma), ...)."""
    D = beta.shape[0]
    sigma = np.asarray(sigma, dtype=np.float64)
    B = np.array([comb(D - 1, r) * sigma ** r * (1.0 - sigma) ** (D - 1 - r) for r in range(D)])      # (D, n)
    return np.tensordot(B.T, beta, axes=(1, 0))


def poly_eval(coef, t, d):
    """coef (3, D) highest power first -> p^(d)(t), (len(t), 3)."""
    D = np.asarray(coef).shape[1]
    t = np.asarray(t, dtype=np.float64)
    out = np.zeros((t.size, 3))
    for col in range(D):
        k = D - 1 - col
        if k >= d:
            out += _falling(k, d) * t[:, None] ** (k - d) * np.asarray(coef)[None, :, col]
    return out


def dense_qp(s, ini, fin, hp, T, K, max_vel, max_acc):
    """The whole QP of one problem in the control-point form, for the dense oracle: Q, A, b as the reference assembles them
    (oracle/minco_np.qp_assemble, untouched by the row form), G, h from dense_G_h in ORDER_CPP with the inert 0.x <= 0 padding
    rows dropped.  ini, fin (3, 3); hp (N, M, 4); T (N,).  Returns Q, A, b, G, h, piece, kind (row_groups of the kept rows)."""
    from oracle import minco_np as onp
    N, M = hp.shape[0], hp.shape[1]
    state = np.zeros((9, 2))
    for ax in range(3):
        state[3 * ax:3 * ax + 3, 0] = ini[ax]
        state[3 * ax:3 * ax + 3, 1] = fin[ax]
    res = K * 2 * s
    Q, A, b = onp.qp_assemble(s, state, np.transpose(hp, (1, 2, 0)), np.full(N, M), T, res, max_vel, max_acc)[:3]
    polys = [hp[i] for i in range(N)]
    G, h = dense_G_h(s, polys, T, K, max_vel, max_acc, 0)
    piece, kind = row_groups(polys, res)
    keep = (np.abs(G).sum(axis=1) > 0) | (h != 0)
    return Q, A, b, G[keep], h[keep], piece[keep], kind[keep]
