#!/usr/bin/env python3
"""Generate tests/golden/max_rate_cases.npz: hard inputs for k_piece_max_rate, k_traj_eval and k_traj_cost with
references from the multiprecision restatement tests/trajectory_mp.py (mpmath + sympy, 60 digits), each rounded
once to double.  Deterministic: running it again reproduces the committed file byte for byte.

    python tests/golden/make_max_rate_golden.py [--check]

Max-rate cases (keys cm, T, which, s, ref, A, dqn, family): cm is padded with zero columns on the right to 3 x 8
(use cm[:, :2 s]); `A` is the scale of the error bound (trajectory_mp.rate_bound); `dqn` is the exact squared norm
that decides the constant-rate branch, rounded to double.

Families (each for s in {2, 3, 4} and which in {1, 2})
  plain      random normal coefficients, T in [0.4, 2].
  wide_T     T in {0.05, 0.2, 5, 20, 50}: once with unit coefficients, once with the coefficient of t^k scaled by
             T^-k (unit speeds in normalised time).
  scale      plain pieces times 1e-3 and times 1e3.
  rest       zero velocity (s >= 3: and acceleration) at both ends: the only maximum is interior.
  one_axis   motion on one axis whose velocity / acceleration changes sign inside the piece: double roots of q.
  multi_root position (t - r)^k, k = 2 .. 2s-1, r in {T/2, T/4}, T a power of two, a second axis at half amplitude:
             exact multiple roots of dq that fall on the split points of the kernel's subdivision.
  cheb       velocity T_(2s-2) mapped to [0, T], T = 1, with and without a 1e-3 random second axis: q's monomial
             coefficients cancel, so evaluating the candidates from q loses what evaluating them from the
             components keeps.
  const      slow pieces on both sides of the DBL_EPSILON threshold of trajectory.hpp:190.  BELOW the threshold the
             stored reference is the MODELLED behaviour -- the rate at t = 0, const_branch_rate_mp -- and not the true
             maximum, which can be far larger: the one place in this fixture where that is so.  (multi_root has a few
             pieces with constant acceleration, dq = 0, where the two coincide.)
Every case keeps a factor 4 away from the threshold: dqn < DBL_EPSILON / 4 or dqn > 4 DBL_EPSILON.

Trajectory cases (keys tr{s}{N}_*): 7 trajectories for each s in {2, 3, 4} and N in {3, 1}; durations are the
permutations of {0.05, 1, 20} (N = 3) or one of them (N = 1); queries at 0, at every knot exactly, at the end,
beyond the end and between knots.  Stored: coeffs, T, tq, ev (4 derivatives x queries x 3), cost and gradT for
m34 in (1400, 1440).
"""
import itertools
import os
import sys
from fractions import Fraction as Fr

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import trajectory_mp as tmp  # noqa: E402

OUT = os.path.join(HERE, "max_rate_cases.npz")
EPS = tmp.EPS
WIDE_T = (0.05, 0.2, 5.0, 20.0, 50.0)
M34S = (1400.0, 1440.0)
TRAJ_DURS = (0.05, 1.0, 20.0)
N_TRAJ = 7


def margin_ok(cm, T, which):
    n = tmp.dq_norm_mp(cm, T, which)
    return n < Fr(EPS) / 4 or n > 4 * Fr(EPS)


def _integrate_desc(v_asc):
    """ascending velocity coefficients -> position row, highest power first, zero constant."""
    p = [0.0] + [c / (k + 1) for k, c in enumerate(v_asc)]
    return np.array(p[::-1])


def _sign_changes(cm_row, T, which):
    t = np.linspace(0.0, T, 2001)
    v = np.polyval(np.polyder(cm_row, which), t)
    sg = np.sign(v[np.abs(v) > 0])
    return int((sg[1:] != sg[:-1]).sum())


def rate_cases():
    rng = np.random.default_rng(20240611)
    cases = []

    def add(fam, s, which, cm, T):
        cm = np.asarray(cm, dtype=np.float64)
        assert cm.shape == (3, 2 * s)
        cases.append((fam, s, which, cm, float(T)))

    def draw(fam, s, which, make):
        """redraw a random case until it keeps the factor-4 margin from the threshold"""
        for _ in range(100):
            cm, T = make()
            if margin_ok(cm, T, which):
                return add(fam, s, which, cm, T)
        raise RuntimeError("no case with the threshold margin: " + fam)

    for s, which in itertools.product((2, 3, 4), (1, 2)):
        D = 2 * s
        pw = np.arange(D - 1, -1, -1)                                   # power of column i
        for _ in range(3):
            draw("plain", s, which, lambda: (rng.standard_normal((3, D)), rng.uniform(0.4, 2.0)))
        for T in WIDE_T:
            draw("wide_T", s, which, lambda: (rng.standard_normal((3, D)), T))
            draw("wide_T", s, which, lambda: (rng.standard_normal((3, D)) * T ** (-pw.astype(float)), T))
        for sc in (1e-3, 1e-3, 1e3, 1e3):
            draw("scale", s, which, lambda: (rng.standard_normal((3, D)) * sc, rng.uniform(0.4, 2.0)))
        # rest: p = d * smoothstep(t / T) (+ for s = 4 the two free shapes tau^3 (1 - tau)^3 (alpha + beta tau))
        smooth = {2: [0, 0, 3, -2], 3: [0, 0, 0, 10, -15, 6], 4: [0, 0, 0, 0, 35, -84, 70, -20]}[s]
        for _ in range(3):
            def rest():
                T = rng.uniform(0.4, 2.0)
                cm = np.zeros((3, D))
                for ax in range(3):
                    asc = np.array(smooth, dtype=float) * rng.normal() * 2.0
                    if s == 4:
                        bump = np.polynomial.polynomial.polymul([0, 0, 0, 1], [1, -3, 3, -1])
                        asc = asc + np.polynomial.polynomial.polymul(bump, rng.normal(size=2) * 20.0)
                    cm[ax] = (asc * T ** (-np.arange(D, dtype=float)))[::-1]
                    cm[ax, -1] = rng.normal()
                return cm, T
            draw("rest", s, which, rest)
        for _ in range(3):
            def one_axis():
                T = rng.uniform(0.4, 2.0)
                for _ in range(1000):
                    cm = np.zeros((3, D))
                    cm[int(rng.integers(3))] = rng.standard_normal(D)
                    if _sign_changes(cm[np.abs(cm).sum(axis=1) > 0][0], T, which) >= min(2, D - 1 - which):
                        return cm, T
                raise RuntimeError("one_axis")
            draw("one_axis", s, which, one_axis)
        for k in range(2, D):
            for j, rdiv in enumerate((2, 4)):
                T = (1.0, 2.0, 0.5, 4.0)[(k + j) % 4]
                r = T / rdiv
                row = np.zeros(D)
                row[D - 1 - k:] = np.poly([r] * k)                      # (t - r)^k: binomials times powers of two, exact
                cm = np.zeros((3, D))
                cm[k % 3] = row
                cm[(k + 1) % 3] = 0.5 * row
                assert margin_ok(cm, T, which), ("multi_root", s, which, k)
                add("multi_root", s, which, cm, T)
        # cheb: v_x(t) = T_(2s-2)(2 t - 1), T = 1
        cheb = np.polynomial.chebyshev.Chebyshev.basis(2 * s - 2)
        v_asc = cheb(np.polynomial.Polynomial([-1.0, 2.0])).coef
        for pert in (0.0, 1e-3):
            cm = np.zeros((3, D))
            cm[0] = _integrate_desc(v_asc)
            if pert:
                cm[1] = rng.standard_normal(D) * pert
            assert margin_ok(cm, 1.0, which), ("cheb", s, which)
            add("cheb", s, which, cm, 1.0)
        # const: scale a random piece so that the exact dq norm lands at a chosen multiple of DBL_EPSILON
        for target in (0.02, 0.2, 5.0, 50.0):
            def const():
                cm, T = rng.standard_normal((3, D)), rng.uniform(0.4, 2.0)
                n0 = float(tmp.dq_norm_mp(cm, T, which))
                return cm * (target * EPS / n0) ** 0.25, T            # the norm is quartic in the coefficients
            draw("const", s, which, const)
            got = float(tmp.dq_norm_mp(cases[-1][3], cases[-1][4], which)) / EPS
            assert 0.5 * target < got < 2.0 * target, (got, target)
    return cases


def rate_reference(case):
    fam, s, which, cm, T = case
    dqn = tmp.dq_norm_mp(cm, T, which)
    assert dqn < Fr(EPS) / 4 or dqn > 4 * Fr(EPS), (fam, s, which, float(dqn))
    return float(tmp.modelled_max_rate_mp(cm, T, which)), tmp.rate_A(cm, T, which), float(dqn)


def traj_cases(s, N):
    rng = np.random.default_rng(1000 * s + N)
    D = 2 * s
    perms = list(itertools.permutations(TRAJ_DURS))
    T = np.array([perms[i % 6] if N == 3 else (TRAJ_DURS[i % 3],) for i in range(N_TRAJ)], dtype=np.float64)
    coeffs = rng.standard_normal((N_TRAJ, N, 3, D))
    pw = np.arange(D - 1, -1, -1, dtype=float)
    coeffs[1::2] *= T[1::2, :, None, None] ** (-pw)                     # every other one: unit speeds in normalised time
    knots = np.cumsum(T, axis=1)
    total = knots[:, -1]
    tq = np.zeros((N_TRAJ, 8))
    tq[:, 1] = total
    tq[:, 2] = total + 0.37
    if N == 3:
        tq[:, 3] = knots[:, 0]
        tq[:, 4] = knots[:, 1]
        for q, i in ((5, 0), (6, 1), (7, 2)):                           # inside every piece
            tq[:, q] = knots[:, i] - T[:, i] * rng.uniform(0.1, 0.9, size=N_TRAJ)
    else:
        tq[:, 3:] = total[:, None] * rng.uniform(0.02, 0.98, size=(N_TRAJ, 5))
    return coeffs, T, tq


def traj_reference(s, coeffs, T, tq):
    ev = np.array([[[[float(v) for v in tmp.traj_eval_mp(coeffs[b], T[b], tq[b, q], d)]
                     for q in range(tq.shape[1])] for d in range(4)] for b in range(len(T))])
    cost = np.array([[float(tmp.traj_cost_mp(coeffs[b], T[b], s, m)) for b in range(len(T))] for m in M34S])
    grad = np.array([[[float(g) for g in tmp.traj_cost_grad_T_mp(coeffs[b], T[b], s, m)]
                      for b in range(len(T))] for m in M34S])
    return ev, cost, grad


def generate():
    cases = rate_cases()
    refs = [rate_reference(c) for c in cases]
    cm = np.zeros((len(cases), 3, 8))
    for i, c in enumerate(cases):
        cm[i, :, :2 * c[1]] = c[3]
    out = dict(cm=cm, T=np.array([c[4] for c in cases]), which=np.array([c[2] for c in cases], dtype=np.int8),
               s=np.array([c[1] for c in cases], dtype=np.int8), family=np.array([c[0] for c in cases]),
               ref=np.array([r[0] for r in refs]), A=np.array([r[1] for r in refs]), dqn=np.array([r[2] for r in refs]))
    for s, N in itertools.product((2, 3, 4), (3, 1)):
        coeffs, T, tq = traj_cases(s, N)
        ev, cost, grad = traj_reference(s, coeffs, T, tq)
        p = "tr%d%d_" % (s, N)
        out.update({p + "coeffs": coeffs, p + "T": T, p + "tq": tq, p + "ev": ev, p + "cost": cost, p + "gradT": grad})
    return out


def npz_bytes(data):
    """np.savez_compressed with the members' time stamps pinned, so that the same arrays give the same bytes."""
    import io
    import zipfile
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(data):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(data[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue(),
                        compress_type=zipfile.ZIP_DEFLATED)
    return buf.getvalue()


if __name__ == "__main__":
    data = generate()
    if "--check" in sys.argv:
        with open(OUT, "rb") as f:
            assert f.read() == npz_bytes(data), "the generator no longer reproduces " + OUT
        print("fixture reproduced byte for byte:", len(data["T"]), "max-rate cases")
    else:
        with open(OUT, "wb") as f:
            f.write(npz_bytes(data))
        fam, cnt = np.unique(data["family"], return_counts=True)
        print(len(data["T"]), "max-rate cases", dict(zip(fam.tolist(), cnt.tolist())), os.path.getsize(OUT), "bytes")
