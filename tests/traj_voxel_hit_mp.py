"""TEST INFRASTRUCTURE ONLY -- multiprecision reference for k_traj_voxel_hit (csrc/voxel_hit_kernels.h) and the a-priori bounds
its tests use.

    q_ax(tau) = (p_ax(T tau) - origin_ax) / scale,   cell = trunc(q) where -1 < q < size, outside otherwise
    t* = T inf { tau in [0, 1] : outside, or voxels[cell] != 0 }

Built on the exact algebra of tests/trajectory_mp.py and the root isolation of tests/corridor_margin_mp.py (`Fraction` from the
doubles, square-free part over QQ, root count by Sturm sequences, `polyroots` at 60 digits): per axis every crossing of a cell
plane q = 1 .. size - 1 and of the two map-boundary planes q = -1, q = size is a polynomial root; the roots are sorted, the
midpoint of each gap gives the cell occupied there, and the first blocked gap gives t*, the voxel and the crossing axis.

The `*_mp` functions need mpmath and sympy; `hit_bound`, `tol_pos`, `cells_float64`, `hit_float64` need numpy only, so GPU tests read the
references from tests/golden/traj_voxel_hit_cases.npz (tests/golden/make_traj_voxel_hit_golden.py writes it).
"""
import math
from fractions import Fraction as Fr

import numpy as np

from tests import corridor_margin_mp as cmm
from tests.bernstein_np import advance, bernstein
from tests import trajectory_mp as tmp
from tests.trajectory_mp import _mpf, _pder, _pval, EPS

try:
    import mpmath
except ImportError:
    mpmath = None

# the kernel's structural constants (csrc/voxel_hit_kernels.h)
HIT_DEPTH, HIT_MAX_NODES, HIT_BISECT, HIT_BOX_CELLS, HIT_C = 32, 2048, 56, 8, 32.0
HIT_FREE, HIT_OUTSIDE, HIT_INVALID = -1, -2, -3


class Grid:
    """size (3,) ints, origin (3,), scale: an anet_voxel_grid"""

    def __init__(self, size, origin, scale):
        self.size = tuple(int(x) for x in size)
        self.origin = tuple(float(x) for x in origin)
        self.scale = float(scale)

    def planes(self, ax):
        """every q at which the cell of axis ax changes or the map is left, ascending"""
        return [-1] + list(range(1, self.size[ax])) + [self.size[ax]]


def q_exact(cm, T, grid):
    """q[ax][k], ascending Fractions: the exact coefficients of q_ax in normalised time"""
    cm = np.asarray(cm, dtype=np.float64)
    n = cm.shape[1] - 1
    Tq, sc = Fr(float(T)), Fr(grid.scale)
    q = [[Fr(float(cm[ax, n - k])) * Tq ** k / sc for k in range(n + 1)] for ax in range(3)]
    for ax in range(3):
        q[ax][0] -= Fr(grid.origin[ax]) / sc
    return q


def cell_of(q, size):
    """the cell of a coordinate (any real type): -1 / size stand for the two outsides, as in the kernel"""
    if q <= -1:
        return -1
    if q >= size:
        return size
    return int(q)          # toward zero: (-1, 1) is cell 0


def probe(cell, grid, vox):
    """HIT_FREE, HIT_OUTSIDE or the linear index of a blocked voxel"""
    x, y, z = cell
    sx, sy, sz = grid.size
    if x < 0 or y < 0 or z < 0 or x >= sx or y >= sy or z >= sz:
        return HIT_OUTSIDE
    i = x + sx * (y + sy * z)
    return i if vox[i] != 0 else HIT_FREE


def _reach(qa):
    """[lo, hi] containing qa(tau) on [0, 1]: the constant term -+ the sum of the other moduli"""
    r = sum((abs(c) for c in qa[1:]), Fr(0))
    return qa[0] - r, qa[0] + r


def crossings_mp(q, grid):
    """sorted [(tau mpf, axis, plane)]: every root in [0, 1] of q_ax = plane over the planes of the three axes"""
    tmp._need_mp()
    out = []
    for ax in range(3):
        lo, hi = _reach(q[ax])
        for pl in grid.planes(ax):
            if pl < lo or pl > hi:
                continue
            g = list(q[ax])
            g[0] = g[0] - pl
            out += [(r, ax, pl) for r in cmm.roots01_mp(g)]
    return sorted(out, key=lambda e: e[0])


def piece_hit_mp(cm, T, grid, vox):
    """The reference.  Returns dict: tau (mpf, normalised time of the first blocked point; None when free), voxel, axis (-1 when
    the piece starts blocked or is free), dq (|dq_axis/dtau| at tau, mpf; None), plane, crossings (the sorted list)."""
    tmp._need_mp()
    q = q_exact(cm, T, grid)
    qm = [[_mpf(c) for c in qa] for qa in q]
    at = lambda tau: tuple(cell_of(_pval(qm[ax], tau), grid.size[ax]) for ax in range(3))
    start = probe(tuple(cell_of(q[ax][0], grid.size[ax]) for ax in range(3)), grid, vox)
    cr = crossings_mp(q, grid) if float(T) > 0.0 else []
    res = {"tau": None, "voxel": HIT_FREE, "axis": -1, "dq": None, "plane": 0, "crossings": cr}
    if start != HIT_FREE:
        res.update(tau=mpmath.mpf(0), voxel=start)
        return res
    knots = [mpmath.mpf(0)] + [c[0] for c in cr] + [mpmath.mpf(1)]
    for j in range(len(knots) - 1):
        if knots[j + 1] == knots[j]:
            continue
        v = probe(at((knots[j] + knots[j + 1]) / 2), grid, vox)
        if v != HIT_FREE:
            tau, ax, pl = cr[j - 1]
            dq = abs(_pval([_mpf(c) for c in _pder(q[ax])], tau))
            res.update(tau=tau, voxel=v, axis=ax, dq=dq, plane=pl)
            return res
    return res


def extrema_clearance_mp(q, grid):
    """the smallest distance, in voxels, from an end value or an extremum of a component on [0, 1] to a plane of its axis"""
    tmp._need_mp()
    best = mpmath.inf
    for ax in range(3):
        qm = [_mpf(c) for c in q[ax]]
        for tau in [mpmath.mpf(0), mpmath.mpf(1)] + cmm.roots01_mp(_pder(q[ax])):
            v = _pval(qm, tau)
            best = min(best, min(abs(v - pl) for pl in grid.planes(ax)))
    return best


def axis_scales(cm, T, grid):
    """sum_k |u_ax,k| per axis, float64 from the exact coefficients"""
    return np.array([float(sum((abs(c) for c in qa), Fr(0))) for qa in q_exact(cm, T, grid)])


def hit_bound(T, scale, dq):
    """|t_hit - t*| <= T 2^-HIT_DEPTH + HIT_C EPS scale / |dq| T,  scale = sum_k |u_ax,k| + |q_plane| of the crossed axis, dq =
    |dq_ax/dtau| at the crossing (a piece that starts blocked: dq = inf, the second term vanishes).

    The first term: an interval that is not two cells on one monotone axis is halved down to 2^-HIT_DEPTH and decided there by its
    midpoint, so a hit reported at its start is at most one interval early or late.  The second, in roundings of relative size
    EPS / 2, counted without fused operations so that a plain float64 restatement is covered:
      the coefficients qu_k = c_k T^k / scale: T^k by repeated products <= 6, the product with c_k, the division -> 8 roundings on
        |u_k|, 4 EPS sum |u_k| on a value;
      Horner of degree <= 7, a product and a sum per step -> 14 roundings, 7 EPS sum |u_k|;
      the comparison with the plane is exact; a value error e moves the crossing by e / |dq| to first order;
      bisection stops at neighbouring doubles, 2^-53 <= 7 EPS sum |u_k| / |dq| since |dq| <= 7 sum |u_k|;
      t = tau T, one rounding <= EPS / 2 <= 3.5 EPS sum |u_k| / |dq|.
    21.5 EPS to first order, rounded up to the power of two 32 = HIT_C, which leaves the second-order term room as long as the
    crossing is not a tangency (the golden generator keeps extrema 1e-6 voxels from every plane)."""
    T, scale, dq = (np.asarray(x, dtype=np.float64) for x in (T, scale, dq))
    return T * 2.0 ** -HIT_DEPTH + HIT_C * EPS * scale / dq * T


def tol_pos(cm, T, grid):
    """The band, in voxels, inside which either answer is allowed: max(2^-HIT_DEPTH L, HIT_C EPS scale_i); L the arc-length bound
    n max_k |b_k+1 - b_k| from the derivative control values, scale_i = max over the axes of sum_k |u_ax,k| + the largest |plane| the
    component can reach (at most its size and at most sum_k |u_ax,k|)."""
    q = [[float(c) for c in qa] for qa in q_exact(cm, T, grid)]
    n = len(q[0]) - 1
    d = np.stack([np.diff(bernstein(qa)) for qa in q])
    L = n * np.sqrt((d ** 2).sum(axis=0)).max()
    A = np.abs(np.array(q)).sum(axis=1)
    scale = max(A[ax] + min(A[ax], max(grid.size[ax], 1)) for ax in range(3))
    return max(2.0 ** -HIT_DEPTH * L, HIT_C * EPS * scale)


def cheb_coeffs(n):
    """ascending coefficients in tau of T_n(2 tau - 1)"""
    import numpy.polynomial.chebyshev as C
    import numpy.polynomial.polynomial as P
    c = C.cheb2poly([0] * n + [1])
    out = np.zeros(1)
    for k, ck in enumerate(c):
        out = P.polyadd(out, ck * P.polypow([-1.0, 2.0], k))
    return out


def corner_case(s):
    """The input that exhausts the kernel's node budget: an 8 x 8 x 8 map (origin 0, scale 0.25) whose diagonal cells alone are
    free, and a piece whose three voxel coordinates all equal g(tau) = 4 + 3.4 T_n(2 tau - 1), n = 2s - 1: it runs up and down the
    diagonal and passes through the cells' corners exactly, so it is free, and every corner costs the procedure a descent to the
    depth bound.  Returns (grid, vox, cm, T)."""
    grid = Grid((8, 8, 8), (0.0, 0.0, 0.0), 0.25)
    vox = np.ones(512, dtype=np.uint8)
    for k in range(8):
        vox[k + 8 * (k + 8 * k)] = 0
    D = 2 * s
    g = 3.4 * cheb_coeffs(D - 1)
    g[0] += 4.0
    T = 2.0
    cm = np.zeros((3, D))
    for ax in range(3):
        for k in range(D):
            cm[ax, D - 1 - k] = g[k] * 0.25 / T ** k
    return grid, vox, cm, T


def cells_float64(cm, T, grid, t):
    """the cell triple of p(t) as anet_voxel_query forms it from a float64 Horner value (local time t)"""
    cm = np.asarray(cm, dtype=np.float64)
    p = np.array([np.polyval(cm[ax], float(t)) for ax in range(3)])
    qv = (p - np.array(grid.origin)) / grid.scale
    return tuple(cell_of(float(qv[ax]), grid.size[ax]) for ax in range(3))


# ---- the kernel's procedure in plain float64 --------------------------------------------------------------------------------
def hit_float64(cm, T, grid, vox, max_nodes=HIT_MAX_NODES, stats=None):
    """k_traj_voxel_hit statement by statement in plain float64 (no fused operations): (t_hit, voxel)."""
    cm = np.asarray(cm, dtype=np.float64)
    D = cm.shape[1]
    n = D - 1
    size = grid.size
    if not (T >= 0.0 and T < math.inf and np.isfinite(cm).all()):
        return math.nan, HIT_INVALID
    tk = [1.0]
    for k in range(1, D):
        tk.append(tk[-1] * T)
    qu = np.array([[((cm[ax, n] - grid.origin[ax]) if p == 0 else cm[ax, n - p] * tk[p]) / grid.scale for p in range(D)]
                   for ax in range(3)])
    if not (np.abs(qu).sum(axis=1) < 1e300).all():
        return math.nan, HIT_INVALID
    bz = np.stack([bernstein(qu[ax]) for ax in range(3)])

    def horner(g, tau):
        v = g[n]
        for k in range(n - 1, -1, -1):
            v = v * tau + g[k]
        return v

    look = lambda c: probe(c, grid, vox)
    lev, idx = 0, 0
    for _ in range(max_nodes):
        width = math.ldexp(1.0, -lev)
        aa, bb = idx * width, (idx + 1) * width
        rr = aa / bb
        mn, mx, w0, wn, mono = [], [], [], [], []
        for ax in range(3):
            w = list(bz[ax])
            if bb < 1.0:
                le = [w[0]]
                for q in range(1, D):
                    for k in range(D - q):
                        w[k] = w[k] + bb * (w[k + 1] - w[k])
                    le.append(w[0])
                w = le
            if aa > 0.0:
                ri = [0.0] * D
                ri[n] = w[n]
                for q in range(1, D):
                    for k in range(D - q):
                        w[k] = w[k] + rr * (w[k + 1] - w[k])
                    ri[n - q] = w[n - q]
                w = ri
            mn.append(min(w)); mx.append(max(w)); w0.append(w[0]); wn.append(w[n])
            up = all(w[k] > w[k - 1] for k in range(1, D))
            down = all(w[k] < w[k - 1] for k in range(1, D))
            mono.append(1 if up else -1 if down else 0)
        lo = [cell_of(mn[ax], size[ax]) for ax in range(3)]
        hi = [cell_of(mx[ax], size[ax]) for ax in range(3)]
        cnt = [hi[ax] - lo[ax] + 1 for ax in range(3)]
        count = cnt[0] * cnt[1] * cnt[2]
        split = decided = False
        hit = None
        if stats is not None:
            stats["nodes"] = stats.get("nodes", 0) + 1
        if count <= HIT_BOX_CELLS:
            cells = [(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1) for x in range(lo[0], hi[0] + 1)]
            if stats is not None:
                stats["lookups"] = stats.get("lookups", 0) + len(cells)
            if not any(look(c) != HIT_FREE for c in cells):
                decided = True
            else:
                c0 = [cell_of(w0[ax], size[ax]) for ax in range(3)]
                at = look(tuple(c0))
                if at != HIT_FREE:
                    hit, decided = (aa, at), True
                elif count == 2:
                    ax = cnt.index(2)
                    if mono[ax] != 0:
                        decided = True
                        if cell_of(wn[ax], size[ax]) != c0[ax]:
                            lo_, hi_ = aa, bb
                            for _it in range(HIT_BISECT):
                                m = 0.5 * (lo_ + hi_)
                                if not (lo_ < m < hi_):
                                    break
                                if cell_of(horner(qu[ax], m), size[ax]) != c0[ax]:
                                    hi_ = m
                                else:
                                    lo_ = m
                            other = list(c0)
                            other[ax] = c0[ax] + 1 if c0[ax] == lo[ax] else c0[ax] - 1
                            hit = (hi_, look(tuple(other)))
                            if stats is not None:
                                stats["bisect"] = stats.get("bisect", 0) + 1
        if not decided:
            if lev < HIT_DEPTH:
                split = True
            else:
                m = 0.5 * (aa + bb)
                at = look(tuple(cell_of(horner(qu[ax], m), size[ax]) for ax in range(3)))
                if at != HIT_FREE:
                    hit = (aa, at)
                if stats is not None:
                    stats["depth"] = stats.get("depth", 0) + 1
        if hit is not None:
            return hit[0] * T, hit[1]
        lev, idx, more = advance(lev, idx, split)
        if not more:
            return math.inf, HIT_FREE
    return idx * math.ldexp(1.0, -lev) * T, HIT_INVALID
