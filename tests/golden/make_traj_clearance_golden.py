#!/usr/bin/env python3
"""Fixtures of the exact trajectory-to-points clearance, made on the CPU by this project's own multiprecision reference
(tests/traj_clearance_mp.py).  Writes data only: tests/golden/traj_clearance_cases.npz.

    python tests/golden/make_traj_clearance_golden.py [--check]

Families, PER_FAMILY cases for each order s = 2, 3, 4 (coordinates within +-20 m, durations 0.3 .. 3 s unless the family says
otherwise; at most 48 points per set; the points of most sets on a 2^-10 m lattice and most coefficients float32 values, so that
the file stays small):
  solver      a solver-like piece (control points along a chord, perturbed) against a cloud beside it
  min_t0, min_tT, interior   the minimum at t = 0, at t = T_i, strictly inside (verified on the reference)
  on_curve    one point is p(t0), evaluated exactly and rounded to double
  near_touch  one point 1e-12 .. 1e-6 m beside the curve
  stationary  only the constant term
  straight    a straight constant-speed piece
  cheb        Chebyshev-like components: many local minima per point
  symmetric   a parabola and a point on its axis: two symmetric minima
  duplicates  the cloud holds its points twice or three times
  nonfinite   NaN and infinite coordinates mixed into the cloud
  empty       all points non-finite, or a count of 0
  T0          T_i = 0: the point p_i(0)
  spread      T_i = 1e-3 or 30
A candidate that is not of its family on the reference (the minimum not where the family wants it) is redrawn; nothing else is:
the bound of the tests plays no part in what the file holds.  The redraws are counted per family and order and printed, and
fewer than 5 % of the candidates may be redrawn (asserted).
"""
import os
import sys
from fractions import Fraction as Fr
from math import comb

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import traj_clearance_mp as cm_  # noqa: E402
from tests import traj_voxel_hit_mp as hm  # noqa: E402

OUT = os.path.join(HERE, "traj_clearance_cases.npz")
FAMILIES = ["solver", "min_t0", "min_tT", "interior", "on_curve", "near_touch", "stationary", "straight", "cheb", "symmetric",
            "duplicates", "nonfinite", "empty", "T0", "spread"]
PER_FAMILY = 3
MAXP = 48
LATTICE = 1024.0


def from_control_points(bq, T):
    """Bernstein control points (3, D) in metres over normalised time -> coefficient matrix in local time, highest power first"""
    D = bq.shape[1]
    n = D - 1
    cm = np.zeros((3, D))
    for ax in range(3):
        for k in range(D):
            u = sum(comb(n, k) * comb(k, i) * (-1) ** (k - i) * bq[ax, i] for i in range(k + 1))
            cm[ax, n - k] = u / T ** k if k else u
    return short(cm)


def short(cm):
    """the coefficients rounded to the nearest float32 value (held as doubles): 29 zero bits each, so that the file stays small"""
    return np.asarray(cm, dtype=np.float32).astype(np.float64)


def from_normalised(ua, T, rounded=True):
    """ascending coefficients in tau, (3, <= D) -> coefficient matrix"""
    ua = np.asarray(ua, dtype=np.float64)
    D = ua.shape[1]
    cm = np.zeros((3, D))
    for k in range(D):
        cm[:, D - 1 - k] = ua[:, k] / T ** k if k else ua[:, k]
    return short(cm) if rounded else cm


def solver_piece(s, rng, T):
    D = 2 * s
    a = rng.uniform(-12.0, 12.0, 3)
    d = rng.normal(size=3)
    b = a + d / np.linalg.norm(d) * rng.uniform(1.0, 6.0)
    w = np.linspace(0.0, 1.0, D)[None]
    bq = a[:, None] * (1.0 - w) + b[:, None] * w
    bq[:, 1:-1] += rng.uniform(-0.3, 0.3, (3, D - 2))
    return from_control_points(bq, T)


def pos(cm, t):
    return np.array([np.polyval(cm[ax], t) for ax in range(3)])


def pos_exact_rounded(cm, t):
    """p(t) evaluated exactly on the doubles and rounded once"""
    n = cm.shape[1] - 1
    tq = Fr(float(t))
    return np.array([float(sum((Fr(float(cm[ax, n - k])) * tq ** k for k in range(n + 1)), Fr(0))) for ax in range(3)])


def normal_to(cm, t, rng):
    v = np.array([np.polyval(np.polyder(cm[ax]), t) for ax in range(3)])
    r = rng.normal(size=3)
    if np.linalg.norm(v) > 0:
        v = v / np.linalg.norm(v)
        r = r - v * (r @ v)
    return r / np.linalg.norm(r)


def lattice(p):
    return np.round(np.asarray(p) * LATTICE) / LATTICE


def cloud_beside(cm, T, rng, m, lo=0.3, hi=2.0):
    out = []
    for _ in range(m):
        t = rng.uniform(0.0, T)
        out.append(pos(cm, t) + normal_to(cm, t, rng) * rng.uniform(lo, hi))
    return lattice(out)


def draw(family, s, rng):
    """-> (cm (3, 2s), T, pts (m, 3), count or -1) of a candidate"""
    D = 2 * s
    T = float(rng.uniform(0.3, 3.0))
    m = int(rng.choice([3, 4, 6, 10, MAXP], p=[0.3, 0.3, 0.2, 0.15, 0.05]))
    if family == "spread":
        T = float(rng.choice([1e-3, 30.0]))
    if family == "T0":
        T = 0.0
        cm = solver_piece(s, rng, 1.0)
        return cm, T, lattice(pos(cm, 0.0)[None] + rng.uniform(-2, 2, (m, 3))), -1
    if family == "stationary":
        cm = np.zeros((3, D))
        cm[:, -1] = short(rng.uniform(-15, 15, 3))
        return cm, T, lattice(cm[:, -1][None] + rng.uniform(-2, 2, (m, 3))), -1
    if family == "straight":
        a, v = rng.uniform(-12, 12, 3), rng.uniform(-2, 2, 3)
        cm = np.zeros((3, D))
        cm[:, -1], cm[:, -2] = short(a), short(v)
        return cm, T, cloud_beside(cm, T, rng, m), -1
    if family == "cheb":
        ua = np.zeros((3, D))
        for ax in range(3):
            qa = rng.uniform(0.5, 3.0) * hm.cheb_coeffs(D - 1 - int(rng.integers(0, 2)))
            ua[ax, :len(qa)] = qa
            ua[ax, 0] += rng.uniform(-8, 8)
        cm = from_normalised(ua, T)
        c = ua[:, 0]
        return cm, T, lattice(c[None] + rng.uniform(-3.5, 3.5, (min(m, 16), 3))), -1
    if family == "symmetric":
        # x = a s, y = b s^2, s = 2 tau - 1; the point (0, y0) with y0 = a^2 / (2 b) + b s0^2 has its minima at s = -+ s0
        a, b, s0 = rng.uniform(1.0, 3.0), rng.uniform(1.0, 3.0), rng.uniform(0.2, 0.8)
        c = lattice(rng.uniform(-8, 8, 3))
        ua = np.zeros((3, D))
        ua[0, :2] = [c[0] - a, 2 * a]
        ua[1, :3] = [c[1] + b, -4 * b, 4 * b]
        ua[2, 0] = c[2]
        q = np.array([c[0], c[1] + a * a / (2 * b) + b * s0 * s0, c[2]])
        far = lattice(c[None] + np.array([0.0, -6.0, 0.0]) + rng.uniform(-1, 1, (2, 3)))
        return from_normalised(ua, T, rounded=False), T, np.vstack([far[:1], q[None], far[1:]]), -1
    cm = solver_piece(s, rng, T)
    if family == "empty":
        if rng.random() < 0.5:
            return cm, T, cloud_beside(cm, T, rng, 4), 0
        bad = rng.choice([np.nan, np.inf, -np.inf], (4, 3))
        good = cloud_beside(cm, T, rng, 4)
        keep = rng.random((4, 3)) < 0.5
        keep[np.arange(4), rng.integers(0, 3, 4)] = False
        return cm, T, np.where(keep, good, bad), -1
    if family in ("min_t0", "min_tT"):
        t = 0.0 if family == "min_t0" else T
        v = np.array([np.polyval(np.polyder(cm[ax]), t) for ax in range(3)])
        v = v / np.linalg.norm(v) * (-1.0 if family == "min_t0" else 1.0)
        q = pos(cm, t) + v * rng.uniform(0.3, 1.5) + normal_to(cm, t, rng) * rng.uniform(0.0, 0.2)
        far = cloud_beside(cm, T, rng, m - 1, 3.0, 5.0)
        return cm, T, np.vstack([far[:1], lattice(q)[None], far[1:]]), -1
    if family in ("interior", "on_curve", "near_touch"):
        t = float(rng.uniform(0.15, 0.85) * T)
        if family == "interior":
            q = lattice(pos(cm, t) + normal_to(cm, t, rng) * rng.uniform(0.1, 1.0))
        elif family == "on_curve":
            q = pos_exact_rounded(cm, t)
        else:
            q = pos_exact_rounded(cm, t) + normal_to(cm, t, rng) * 10.0 ** rng.uniform(-12, -6)
        far = cloud_beside(cm, T, rng, m - 1, 2.0, 4.0)
        return cm, T, np.vstack([far[:1], q[None], far[1:]]), -1
    pts = cloud_beside(cm, T, rng, m)
    if family == "duplicates":
        base = pts[:max(2, min(len(pts), 6))]
        pts = np.vstack([base, base[::-1], base[:2]])
    if family == "nonfinite":
        pts = pts.copy()
        k = max(1, len(pts) // 3)
        rows = rng.choice(len(pts), k, replace=False)
        pts[rows, rng.integers(0, 3, k)] = rng.choice([np.nan, np.inf, -np.inf], k)
    return cm, T, pts, -1


def of_family(family, ref, T):
    if family == "min_t0":
        return ref["tau"] == 0
    if family == "min_tT":
        return ref["tau"] == 1
    if family in ("interior", "near_touch", "symmetric"):
        ok = ref["interior"]
        if family == "near_touch":
            ok = ok and 1e-13 < float(ref["d"]) < 2e-6
        return ok
    if family == "on_curve":
        return float(ref["d"]) < 1e-13
    if family == "empty":
        return ref["point"] < 0
    return ref["point"] >= 0


def make_case(task):
    family, s, k = task
    rng = np.random.default_rng([20261019, FAMILIES.index(family), s, k])
    rejected = 0
    while True:
        cm, T, pts, count = draw(family, s, rng)
        use = pts if count < 0 else pts[:count]
        ref = cm_.piece_clearance_mp(cm, T, use)
        if of_family(family, ref, T):        # the only reason to redraw: the bound plays no part in what the file holds
            break
        rejected += 1
        assert rejected < 50, (family, s, k)
    return dict(family=FAMILIES.index(family), s=s, cm=cm, T=T, pts=pts, count=count, d=float(ref["d"]), point=ref["point"],
                tau=float(ref["tau"]), kappa=float(ref["kappa"]), speed=float(ref["speed"]), interior=ref["interior"],
                runner=float(ref["runner"]), rejected=rejected)


def main():
    from multiprocessing import Pool
    tasks = [(f, s, k) for f in FAMILIES for s in (2, 3, 4) for k in range(PER_FAMILY)]
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        cases = pool.map(make_case, tasks, chunksize=1)
    n = len(cases)
    cmat = np.zeros((n, 3, 8))
    for i, c in enumerate(cases):
        cmat[i, :, :2 * c["s"]] = c["cm"]
    data = dict(
        families=np.array(FAMILIES), family=np.array([c["family"] for c in cases], dtype=np.int8),
        s=np.array([c["s"] for c in cases], dtype=np.int8), cm=cmat, T=np.array([c["T"] for c in cases]),
        npts=np.array([len(c["pts"]) for c in cases], dtype=np.int32), pts=np.vstack([c["pts"] for c in cases]),
        count=np.array([c["count"] for c in cases], dtype=np.int32), d=np.array([c["d"] for c in cases]),
        point=np.array([c["point"] for c in cases], dtype=np.int32), tau=np.array([c["tau"] for c in cases]),
        kappa=np.array([c["kappa"] for c in cases]), interior=np.array([c["interior"] for c in cases]),
        runner=np.array([c["runner"] for c in cases]), speed=np.array([c["speed"] for c in cases]))
    rej = sum(c["rejected"] for c in cases)
    per = {}
    for c in cases:
        if c["rejected"]:
            key = "%s s=%d" % (FAMILIES[c["family"]], c["s"])
            per[key] = per.get(key, 0) + c["rejected"]
    print(f"{n} cases, {rej} candidates redrawn {per}, {int(data['npts'].sum())} points")
    assert rej < 0.05 * (n + rej)
    if "--check" in sys.argv:
        old = np.load(OUT)
        for k, v in data.items():
            assert np.array_equal(old[k], v, equal_nan=v.dtype.kind == "f"), k
        print("matches", OUT)
        return
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
