#!/usr/bin/env python3
"""Generate tests/golden/corridor_margin_cases.npz: hard inputs for k_traj_row_margin with references from the multiprecision
restatement tests/corridor_margin_mp.py (mpmath + sympy, 60 digits), each rounded once to double.  Deterministic: running it
again reproduces the committed file byte for byte.

    python tests/golden/make_corridor_margin_golden.py [--check]

Keys: cm (3 x 8, zero columns on the right: use cm[:, :2 s]), T, d, s, rows (RMAX x 4, zero rows are padding), family, ref (the
margin), ref_row, ref_tau, scale (of the bound, corridor_margin_mp.margin_bound), gap (reference margin minus the best
maximum of any other row; inf with fewer than two rows).

Families, each for s in {2, 3, 4} and d in {0, 1, 2} (u: the d-th derivative in normalised time, degree 2s-1-d)
  inside    every row slack by more than 0.5.
  endpoint  the maximum is at tau = 0 or 1 with g' != 0 there.
  interior  a single maximum strictly inside.  Not for s = 2, d = 2, where g is linear.
  graze     one axis with p^(d) = b - 420 (t - r)^2 h(t), h > 0, r a dyadic fraction of T, all in exactly representable
            numbers: g touches zero from below with an exact double root, on a split point of the kernel's subdivision for
            r = T/2, T/4 and off every one for r = 3T/8 (depth 3).  Not for s = 2, d = 2: a linear g touches nothing.
  flat      a orthogonal to the motion: g is constant -- once exactly (motion in x, y; a = e_z) and once through cancellation
            (y = 3 x in coefficients of 20 bits, a = (3, -1, 0)), where the float64 control values carry rounding noise.
  cheb      u_x = T_m(2 tau - 1), m = 2s-1-d: values in [-1, 1] from coefficients that sum to 1.1e5 at m = 7 (T_m(3)); the
            maximum 1 is attained at both ends and at every other interior extremum.
  multi     two rows whose maxima differ by less than the bound (mirror rows on a one-axis motion; b and its neighbour).
  between   the violation lies strictly between two neighbouring samples j/20 and g <= 0 at every sample j/20: for d = 0 as a
            corridor row, for d = 1, 2 as the box rows +-e_ax <= limit (five of the six: the sixth, -e_z, is slack and the
            reference with all six is asserted equal here).  Not for s = 2, d = 2 (a linear g).
  pad       zero rows interleaved with real ones.
  empty     no rows.
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import corridor_margin_mp as cmp_  # noqa: E402
from tests.golden.make_max_rate_golden import npz_bytes  # noqa: E402

OUT = os.path.join(HERE, "corridor_margin_cases.npz")
RMAX = 5


def _fall(k, j):
    r = 1.0
    for i in range(j):
        r *= (k - i)
    return r


def cm_from_u(u_asc, T, d, s, low=None):
    """Position row (highest power first, 2s wide) whose d-th derivative in normalised time is u_asc (ascending, degree
    <= 2s-1-d); the d lowest coefficients come from `low` (ascending) or are zero."""
    D = 2 * s
    asc = np.zeros(D)
    if low is not None:
        asc[:d] = low[:d]
    for k, c in enumerate(u_asc):
        asc[k + d] = c / (_fall(k + d, d) * T ** k)
    return asc[::-1].copy()


def u_of(cm, T, d):
    """float64 u[ax] ascending (for designing cases; the reference never uses it)"""
    D = cm.shape[1]
    return np.array([[_fall(k + d, d) * cm[ax, D - 1 - (k + d)] * T ** k for k in range(D - d)] for ax in range(3)])


def gvals(cm, T, d, row, tau):
    u = u_of(cm, T, d)
    return np.asarray(row[:3]) @ np.array([np.polyval(ua[::-1], tau) for ua in u]) - row[3]


def unit(rng):
    a = rng.standard_normal(3)
    return a / np.linalg.norm(a)


def cases():
    rng = np.random.default_rng(20240923)
    out = []
    tau = np.linspace(0.0, 1.0, 4001)

    def add(fam, s, d, cm, T, rows):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
        assert cm.shape == (3, 2 * s) and rows.shape[0] <= RMAX
        out.append((fam, s, d, np.asarray(cm, dtype=np.float64), float(T), rows))

    def slack_row(cm, T, d, by):
        a = unit(rng)
        return np.r_[a, gvals(cm, T, d, np.r_[a, 0.0], tau).max() + by]

    for s, d in itertools.product((2, 3, 4), (0, 1, 2)):
        D = 2 * s
        m = D - 1 - d
        for _ in range(3):
            cm, T = rng.standard_normal((3, D)), rng.uniform(0.4, 2.0)
            add("inside", s, d, cm, T, [slack_row(cm, T, d, rng.uniform(0.6, 3.0)) for _ in range(3)])
        for want_end in (0, 1, int(rng.integers(2))):
            for _ in range(10000):
                cm, T, a = rng.standard_normal((3, D)), rng.uniform(0.2, 0.8), unit(rng)
                g = gvals(cm, T, d, np.r_[a, 0.0], tau)
                k = int(g.argmax())
                slope = abs(g[1] - g[0]) if k == 0 else abs(g[-1] - g[-2])
                if k == (0 if want_end == 0 else len(tau) - 1) and slope * (len(tau) - 1) > 0.2:
                    break
            else:
                raise RuntimeError("endpoint")
            add("endpoint", s, d, cm, T, [np.r_[a, g.max() - rng.uniform(-0.3, 0.3)], slack_row(cm, T, d, 2.0)])
        for _ in range(3 if m >= 2 else 0):
            for _ in range(10000):
                cm, T, a = rng.standard_normal((3, D)), rng.uniform(0.6, 2.0), unit(rng)
                g = gvals(cm, T, d, np.r_[a, 0.0], tau)
                k = int(g.argmax())
                inner = (g[1:-1] > g[:-2]) & (g[1:-1] > g[2:])
                if 400 < k < 3600 and inner.sum() == 1 and g[k] - max(g[0], g[-1]) > 0.05:
                    break
            else:
                raise RuntimeError("interior")
            add("interior", s, d, cm, T, [slack_row(cm, T, d, 1.0), np.r_[a, g.max() - rng.uniform(-0.3, 0.3)]])
        if m >= 2:
            for T, rdiv, hdeg in ((1.0, 2.0, 0), (2.0, 4.0, min(1, m - 2)), (1.0, 8.0 / 3.0, min(1, m - 2))):
                r = T / rdiv
                w = np.polynomial.polynomial.polymul([r * r, -2.0 * r, 1.0], [1.0, 0.5][:hdeg + 1])   # (t - r)^2 h(t), exact
                bq = float(rng.integers(100, 400))
                p_d = -420.0 * w
                p_d[0] += bq                                                  # p^(d)(t) = b - 420 (t - r)^2 h(t), real time
                u = p_d * T ** np.arange(len(p_d))
                cm = rng.standard_normal((3, D)) * 0.5
                cm[0] = cm_from_u(u, T, d, s, low=[1.0, -2.0])
                add("graze", s, d, cm, T, [[1.0, 0.0, 0.0, bq], slack_row(cm, T, d, 5.0)])
        # flat
        cm, T = rng.standard_normal((3, D)), rng.uniform(0.4, 2.0)
        cm[2] = 0.0
        cm[2, -1 - d] = 0.75                                                  # the d-th derivative of z is the constant d! * 0.75
        add("flat", s, d, cm, T, [[0.0, 0.0, 1.0, 0.5], slack_row(cm, T, d, 4.0)])
        cm, T = rng.standard_normal((3, D)), rng.uniform(0.4, 2.0)
        cm[0] = np.round(cm[0] * 2 ** 20) / 2 ** 20
        cm[1] = 3.0 * cm[0]
        add("flat", s, d, cm, T, [[3.0, -1.0, 0.0, -0.25], slack_row(cm, T, d, 4.0)])
        # cheb
        cheb = np.polynomial.chebyshev.Chebyshev.basis(m)(np.polynomial.Polynomial([-1.0, 2.0])).coef
        cm = np.zeros((3, D))
        cm[0] = cm_from_u(cheb, 1.0, d, s)
        add("cheb", s, d, cm, 1.0, [[1.0, 0.0, 0.0, 0.5]])
        cm = cm.copy()
        cm[1] = rng.standard_normal(D) * 1e-3
        add("cheb", s, d, cm, 1.0, [[np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.25], slack_row(cm, 1.0, d, 3.0)])
        # multi
        cm, T = np.zeros((3, D)), rng.uniform(0.4, 2.0)
        cm[0] = rng.standard_normal(D)
        add("multi", s, d, cm, T, [[0.6, 0.8, 0.0, 0.1], [0.6, -0.8, 0.0, 0.1]])
        cm, T, a = rng.standard_normal((3, D)), rng.uniform(0.4, 2.0), unit(rng)
        bq = gvals(cm, T, d, np.r_[a, 0.0], tau).max() - 0.1
        add("multi", s, d, cm, T, [np.r_[a, bq], np.r_[a, np.nextafter(bq, np.inf)]])
        # between
        if m >= 2:
            for j in (3, 11, 17)[:3 if m >= 3 else 2]:
                T, lim, t0 = rng.uniform(0.5, 2.0), 1.5, (j + rng.uniform(0.45, 0.55)) / 20.0
                bump = np.polynomial.polynomial.polymul([t0 * t0, -2.0 * t0, 1.0], [-3.2])
                if m >= 3:
                    bump = np.polynomial.polynomial.polyadd(bump, 0.5 * np.polynomial.polynomial.polypow([-t0, 1.0], 3))
                bump[0] += 0.001 + lim                                        # u_x = lim + 0.001 - 3.2 (tau - t0)^2 + 0.5 (tau - t0)^3
                cm = np.zeros((3, D))
                cm[0] = cm_from_u(bump, T, d, s, low=[0.2, -0.1])
                cm[1] = cm_from_u([0.3, 0.2, -0.1][:m + 1], T, d, s, low=[0.0, 0.1])
                cm[2] = cm_from_u([-0.2, 0.1], T, d, s, low=[1.0, 0.0])
                if d == 0:
                    rows = [[1.0, 0.0, 0.0, lim], [0.0, 1.0, 0.0, 2.0], [0.0, 0.0, -1.0, 1.0]]
                else:
                    rows = [[1.0, 0, 0, lim], [-1.0, 0, 0, lim], [0, 1.0, 0, lim], [0, -1.0, 0, lim], [0, 0, 1.0, lim]]
                add("between", s, d, cm, T, rows)
        # pad
        for pattern in ((0, 1, 0, 1, 1), (1, 0, 0, 1, 0)):
            cm, T = rng.standard_normal((3, D)), rng.uniform(0.4, 2.0)
            rows = [slack_row(cm, T, d, rng.uniform(-0.5, 0.5)) if p else np.zeros(4) for p in pattern]
            add("pad", s, d, cm, T, rows)
        add("empty", s, d, rng.standard_normal((3, D)), rng.uniform(0.4, 2.0), np.zeros((0, 4)))
    return out


def reference(case):
    fam, s, d, cm, T, rows = case
    m, r, t, per = cmp_.piece_margin_mp(cm, T, d, rows)
    others = [v for (q, v) in per if q != r]
    gap = float(m - max(others)) if others else np.inf
    sc = cmp_.row_scales(cm, T, d, rows)
    if fam == "between" and d > 0:      # the sixth box row changes nothing
        full = np.vstack([rows, [[0.0, 0.0, -1.0, rows[0, 3]]]])
        assert cmp_.piece_margin_mp(cm, T, d, full)[0] == m
    return float(m), int(r), float(t), float(sc.max()) if len(sc) else 0.0, gap


def generate():
    cs = cases()
    refs = [reference(c) for c in cs]
    cm = np.zeros((len(cs), 3, 8))
    rows = np.zeros((len(cs), RMAX, 4))
    for i, c in enumerate(cs):
        cm[i, :, :2 * c[1]] = c[3]
        rows[i, :len(c[5])] = c[5]
    return dict(cm=cm, T=np.array([c[4] for c in cs]), d=np.array([c[2] for c in cs], dtype=np.int8),
                s=np.array([c[1] for c in cs], dtype=np.int8), family=np.array([c[0] for c in cs]), rows=rows,
                ref=np.array([r[0] for r in refs]), ref_row=np.array([r[1] for r in refs], dtype=np.int32),
                ref_tau=np.array([r[2] for r in refs]), scale=np.array([r[3] for r in refs]),
                gap=np.array([r[4] for r in refs]))


if __name__ == "__main__":
    data = generate()
    if "--check" in sys.argv:
        with open(OUT, "rb") as f:
            assert f.read() == npz_bytes(data), "the generator no longer reproduces " + OUT
        print("fixture reproduced byte for byte:", len(data["T"]), "cases")
    else:
        with open(OUT, "wb") as f:
            f.write(npz_bytes(data))
        fam, cnt = np.unique(data["family"], return_counts=True)
        print(len(data["T"]), "cases", dict(zip(fam.tolist(), cnt.tolist())), os.path.getsize(OUT), "bytes")
