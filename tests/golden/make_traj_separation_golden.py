"""Writes tests/golden/traj_separation_cases.npz: pairs of trajectories of orders 2, 3, 4 with N = 1 .. 3 pieces and the 60-digit
reference of tests/traj_separation_mp.py for each (needs mpmath and sympy).  Data only.

    python -m tests.golden.make_traj_separation_golden [--check]

Coordinates stay within +-12 m, durations are 0 (padding) or between 0.05 and 20 s, every time involved is at most 60 s in
modulus.  No case is selected by its bound or by what any implementation returns.
"""
import os
import sys

import numpy as np

from tests import traj_separation_mp as sp

FAMILIES = ["equal", "stagger", "short", "disjoint", "cross", "translated", "self", "knot_min", "end_min", "near_tie", "zero_T",
            "spread", "discont", "cheb"]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "traj_separation_cases.npz")
U = np.array([2.9, 2.0, 1.0, 0.5, 0.3, 0.15, 0.05])     # moduli of u_1 .. u_7; with |u_0| <= 5 a piece stays within 11.9 m
GRID = 2.0 ** -16


def piece_u(rng, s, u0=None, grid=False):
    """u (3, 2s) ascending, normalised time"""
    D = 2 * s
    u = rng.uniform(-1.0, 1.0, (3, D)) * np.r_[5.0, U[:D - 1]][None]
    if u0 is not None:
        u[:, 0] = u0
    return np.round(u / GRID) * GRID if grid else u


def to_cm(u, T, f32=False):
    """coefficient matrix (3, D), highest power first, of p(t) = u(t / T); f32: rounded to float32 values, so that the file
    compresses (the trajectory the case means is the one these doubles describe)"""
    D = u.shape[1]
    cm = (u / float(T) ** np.arange(D)[None])[:, ::-1].copy()
    return cm.astype(np.float32).astype(np.float64) if f32 else cm


def chain(rng, s, Ts, continuous=True, grid=False):
    """(N, 3, D) coefficients of a trajectory with durations Ts; continuous in position (to the float32 rounding of the next
    piece's constant term) unless told otherwise; a piece of zero duration is a constant at the junction"""
    out, end = [], None
    for T in Ts:
        if T == 0.0:
            u = np.zeros((3, 2 * s))
            u[:, 0] = end if end is not None else rng.uniform(-5, 5, 3)
            out.append(u[:, ::-1].copy())
            continue
        for _ in range(200):
            u = piece_u(rng, s, end if continuous else None, grid)
            if np.abs(u.sum(axis=1)).max() <= 5.0:
                break
        out.append(to_cm(u, T, f32=not grid))
        end = np.array([np.polyval(out[-1][ax], T) for ax in range(3)])
    return np.stack(out)


def line(s, p0, p1, T):
    """a straight piece from p0 to p1 in T seconds, (3, D)"""
    u = np.zeros((3, 2 * s))
    u[:, 0], u[:, 1] = p0, np.asarray(p1) - np.asarray(p0)
    return to_cm(u, T)


def const(s, q):
    cm = np.zeros((3, 2 * s))
    cm[:, -1] = q
    return cm


def cheb_piece(rng, s, T):
    """components amp T_m(2 tau - 1) + offset, m = min(2s - 1, 5), amp <= 1 m"""
    D = 2 * s
    m = min(D - 1, 5)
    c = np.polynomial.chebyshev.cheb2poly(np.r_[np.zeros(m), 1.0])
    shifted = np.polynomial.polynomial.Polynomial(c)(np.polynomial.polynomial.Polynomial([-1.0, 2.0])).coef
    u = np.zeros((3, D))
    for ax in range(3):
        u[ax, :m + 1] = rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0]) * shifted
        u[ax, 0] += rng.uniform(-4.0, 4.0)
    return to_cm(u, T, f32=True)


def make_cases():
    rng = np.random.default_rng(20261020)
    cases = []

    def add(fam, s, coa, Ta, t0a, cob, Tb, t0b, pair=(0, 1)):
        N = max(len(Ta), len(Tb))
        co = np.zeros((2, 3, 3, 8))
        T = np.zeros((2, 3))
        for r, (c, t) in enumerate(((coa, Ta), (cob, Tb))):
            for i in range(len(t)):
                co[r, i, :, :2 * s] = c[i]
                T[r, i] = t[i]
        cases.append(dict(family=FAMILIES.index(fam), s=s, n=N, co=co, T=T, t0=np.array([t0a, t0b], dtype=np.float64), pair=pair))

    dur = lambda k: rng.uniform(0.4, 3.0, k)
    for s in (2, 3, 4):
        for rep in range(3):
            N = 1 + rep % 3
            # equal knots
            T = dur(N)
            t0 = float(rng.uniform(-5, 5))
            add("equal", s, chain(rng, s, T), T, t0, chain(rng, s, T), T, t0)
            # staggered knots, start offsets
            Ta, Tb = dur(N), dur(1 + (rep + 1) % 3)
            add("stagger", s, chain(rng, s, Ta), Ta, float(rng.uniform(-20, 20)), chain(rng, s, Tb), Tb, 0.0)
            cases[-1]["t0"][1] = cases[-1]["t0"][0] + rng.uniform(-0.3, 0.3) * Ta[0]
            # one much shorter: the window ends in the middle of a piece
            Ta, Tb = dur(N) + 1.0, rng.uniform(0.05, 0.3, 1 + rep % 2)
            add("short", s, chain(rng, s, Ta), Ta, 2.0, chain(rng, s, Tb), Tb, 2.0 + float(rng.uniform(0.1, 0.8)) * Ta[0])
            # disjoint (rep even) and merely touching (rep odd) windows
            Ta, Tb = dur(N), dur(N)
            t0a = float(rng.uniform(-3, 3))
            endA = sp.knots(Ta, t0a)[-1]
            add("disjoint", s, chain(rng, s, Ta), Ta, t0a, chain(rng, s, Tb), Tb, endA + (0.0 if rep % 2 else float(rng.uniform(0.1, 2))))
            # curves that cross: d(tau) = (tau - 1/2) w exactly in the first piece (dyadic data)
            T = np.array([1.0, 2.0, 0.5])[:N]
            A = chain(rng, s, T, grid=True)
            Bc = chain(rng, s, T, grid=True)
            uA = (A[0][:, ::-1] * T[0] ** np.arange(2 * s)[None])
            w = np.round(rng.uniform(-2, 2, 3) / GRID) * GRID
            uB = uA.copy()
            uB[:, 0] -= 0.5 * w
            uB[:, 1] += w
            Bc[0] = to_cm(uB, T[0])
            add("cross", s, A, T, 1.0, Bc, T, 1.0)
            # the same curve translated: g' = 0 identically
            T = np.array([2.0 if rep else 0.5])
            A = chain(rng, s, T, grid=True)
            Bc = A.copy()
            Bc[:, :, -1] += (np.round(rng.uniform(-3, 3, 3) / GRID) * GRID)[None]
            add("translated", s, A, T, 0.5, Bc, T, 0.5)
            # a trajectory paired with itself
            Ns = 3 if (rep == 2 and s == 3) else 1
            T = dur(Ns)
            A = chain(rng, s, T)
            add("self", s, A, T, float(rng.uniform(-2, 2)), A, T, 0.0, pair=(0, 0))
            # minimum at a window end: b heads for the resting a and the window closes first (rep even), or leaves it (rep odd)
            q = rng.uniform(-4, 4, 3)
            p0 = q + rng.uniform(2, 5, 3) * rng.choice([-1.0, 1.0], 3)
            p1 = q + 0.3 * (p0 - q)
            Tb = np.array([float(rng.uniform(0.5, 2.0))])
            Ta = np.array([Tb[0] * 0.4, Tb[0] * 3.0])
            if rep % 2 == 0:
                add("end_min", s, np.stack([const(s, q)] * 2), Ta, 1.0 - Ta[0] * 1.2, np.stack([line(s, p0, p1, Tb[0])]), Tb, 1.0)
            else:
                add("end_min", s, np.stack([const(s, q)] * 2), Ta, 1.0 - Ta[0] * 0.5, np.stack([line(s, p1, p0, Tb[0])]), Tb, 1.0)
            # zero-duration pieces in the middle and at the end
            T3 = dur(3)
            T3[1 if rep % 2 == 0 else 2] = 0.0
            Tb = dur(2)
            add("zero_T", s, chain(rng, s, T3), T3, 0.0, chain(rng, s, np.r_[Tb, 0.0]), np.r_[Tb, 0.0], float(rng.uniform(-0.5, 0.5)))
            # wide duration spread
            Ta = rng.permutation(np.array([20.0, 0.05, float(rng.uniform(5, 20))]))
            Tb = rng.permutation(np.array([0.05, float(rng.uniform(10, 20)), 0.07]))
            add("spread", s, chain(rng, s, Ta), Ta, 10.0, chain(rng, s, Tb), Tb, float(rng.uniform(10, 25)))
            # discontinuous trajectories
            Ta, Tb = dur(3), dur(2)
            add("discont", s, chain(rng, s, Ta, continuous=False), Ta, 0.0, chain(rng, s, Tb, continuous=False), Tb, 0.5)
            # Chebyshev-like components
            Ta, Tb = rng.uniform(1.0, 2.0, N), rng.uniform(1.0, 2.0, 2)
            add("cheb", s, np.stack([cheb_piece(rng, s, t) for t in Ta]), Ta, 0.0, np.stack([cheb_piece(rng, s, t) for t in Tb]), Tb,
                float(rng.uniform(0.0, 0.5)))
        for rep in range(1):
            # minimum at a knot of one trajectory: b turns away at its knot; a rests, or drifts slowly, in one piece
            q = rng.uniform(-4, 4, 3)
            e1, e2 = np.eye(3)[rng.permutation(3)[:2]]
            r = float(rng.uniform(0.5, 2.0))
            P0, P1, P2 = q - 3.0 * e1 + r * e2, q - 0.5 * e1 + r * e2, q - 2.0 * e1 + (r + 2.0) * e2
            Tb = dur(2)
            Ta = np.array([Tb.sum() + 1.0])
            add("knot_min", s, np.stack([const(s, q)]), Ta, -0.5, np.stack([line(s, P0, P1, Tb[0]), line(s, P1, P2, Tb[1])]), Tb, 0.0)
        for delta in (0.0, 1e-6, 1e-3):
            # two near-equal minima in different intervals: b passes the resting a twice, at distances r and r + delta
            q = rng.uniform(-3, 3, 3)
            r = 1.0
            e1, e2, e3 = np.eye(3)[rng.permutation(3)]
            Tb = np.array([1.0, 0.5, 2.0])
            Bc = np.stack([line(s, q - 2 * e1 + r * e2, q + 2 * e1 + r * e2, 1.0),
                           line(s, q + 2 * e1 + r * e2, q + 2 * e1 + (r + delta) * e3, 0.5),
                           line(s, q + 2 * e1 + (r + delta) * e3, q - 2 * e1 + (r + delta) * e3, 2.0)])
            add("near_tie", s, np.stack([const(s, q)]), np.array([4.0]), 0.0, Bc, Tb, 0.25)
    return cases


def reference(c):
    s, N = c["s"], c["n"]
    co, T, t0 = c["co"][:, :N, :, :2 * s], c["T"][:, :N], c["t0"]
    a, b = c["pair"]
    return sp.pair_separation_mp(co[a], T[a], t0[a], co[b], T[b], t0[b])


def build():
    cases = make_cases()
    refs = [reference(c) for c in cases]
    f = lambda k: np.array([float(r[k]) for r in refs])
    return dict(families=np.array(FAMILIES), family=np.array([c["family"] for c in cases], dtype=np.int32),
                s=np.array([c["s"] for c in cases], dtype=np.int32), n=np.array([c["n"] for c in cases], dtype=np.int32),
                co=np.stack([c["co"] for c in cases]), T=np.stack([c["T"] for c in cases]), t0=np.stack([c["t0"] for c in cases]),
                pair=np.array([c["pair"] for c in cases], dtype=np.int32),
                d=f("d"), t=f("t"), sigma=f("sigma"), kappa=f("kappa"), speed=f("speed"), width=f("width"), runner=f("runner"),
                pa=np.array([r["pa"] for r in refs], dtype=np.int32), pb=np.array([r["pb"] for r in refs], dtype=np.int32),
                interior=np.array([r["interior"] for r in refs]), n_int=np.array([r["n_int"] for r in refs], dtype=np.int32))


if __name__ == "__main__":
    data = build()
    if "--check" in sys.argv:
        old = np.load(OUT)
        for k, v in data.items():
            assert np.array_equal(old[k], v, equal_nan=v.dtype.kind == "f"), k
        print("identical:", OUT)
    else:
        np.savez_compressed(OUT, **data)
        print("wrote", OUT, len(data["d"]), "cases,", os.path.getsize(OUT), "bytes")
