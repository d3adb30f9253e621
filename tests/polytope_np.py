"""Independent statement of the vertex enumeration the GPU tests compare anet_polytope_vertices with (test code only).

Two routes that share nothing with the kernel but the definition of a polytope:
  * interior point by scipy.optimize.linprog (HiGHS), vertices by scipy.spatial.HalfspaceIntersection (Qhull on the polar dual),
    merged at 1e-6 -- the positions, the counts and the active rows;
  * a plain numpy enumeration of all row triples in lexicographic order -- the expected ORDER of the vertices, and the smallest
    |det| among the triples that produce a vertex, on which the position tolerance of the tests rests.
Polytopes are in GCOPTER's raw form: rows h0 x + h1 y + h2 z + h3 <= 0, all-zero rows are padding."""
import itertools

import numpy as np
from scipy.optimize import linprog
from scipy.spatial import HalfspaceIntersection

EPS = 1e-6


def unit_rows(hpoly):
    """(normals (m, 3), offsets (m,), original row numbers (m,)) of the non-padding rows, scaled to unit normals."""
    h = np.asarray(hpoly, dtype=np.float64).reshape(-1, 4)
    idx = np.nonzero(np.any(h[:, :3] != 0.0, axis=1))[0]
    h = h[idx]
    nrm = np.sqrt(h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1] + h[:, 2] * h[:, 2])
    return h[:, :3] / nrm[:, None], h[:, 3] / nrm, idx


def interior(hpoly, bound=1e7):
    """(depth, point) of the deepest point: max t s.t. n.x + t <= -d (HiGHS).  depth = -inf without rows or when infeasible,
    +inf when unbounded."""
    n, d, _ = unit_rows(hpoly)
    if len(n) == 0:
        return -np.inf, np.zeros(3)
    res = linprog([0.0, 0.0, 0.0, -1.0], A_ub=np.c_[n, np.ones(len(n))], b_ub=-d, bounds=[(None, None)] * 3 + [(None, bound)],
                  method="highs")
    if res.status == 2:
        return -np.inf, np.zeros(3)
    if res.status == 3 or (res.status == 0 and res.x[3] >= bound * (1.0 - 1e-9)):
        return np.inf, np.zeros(3)
    assert res.status == 0, res.message
    return float(res.x[3]), res.x[:3]


def bounded(hpoly):
    """True when the polytope is bounded: x, y and z each have a finite maximum and minimum over it (six programmes)."""
    n, d, _ = unit_rows(hpoly)
    if len(n) == 0:
        return False
    for u in np.vstack([np.eye(3), -np.eye(3)]):
        if linprog(-u, A_ub=n, b_ub=-d, bounds=[(None, None)] * 3, method="highs").status == 3:
            return False
    return True


def merge(points, res=EPS):
    """Greedy merge in the given order: a point is dropped when a kept one lies within res (max-norm)."""
    kept = []
    for p in points:
        if not any(np.max(np.abs(p - q)) <= res for q in kept):
            kept.append(p)
    return np.array(kept).reshape(-1, 3)


def vertices_qhull(hpoly, res=EPS):
    """Vertices by Qhull's half-space intersection about the deepest point, merged at res.  None when the polytope has no interior
    point or is unbounded."""
    depth, x = interior(hpoly)
    if not (depth > 0.0 and np.isfinite(depth)) or not bounded(hpoly):
        return None
    n, d, _ = unit_rows(hpoly)
    hs = HalfspaceIntersection(np.c_[n, d], x)
    pts = hs.intersections
    return merge(pts[np.all(np.isfinite(pts), axis=1)], res)


def active_rows(hpoly, verts, eps=EPS):
    """(k, 2) uint64 masks: bit r % 64 of word r // 64 is set when row r of hpoly has |n.v + d| <= eps at vertex v."""
    n, d, idx = unit_rows(hpoly)
    out = np.zeros((len(verts), 2), dtype=np.uint64)
    r = np.abs(np.asarray(verts) @ n.T + d)
    for v in range(len(verts)):
        for j in np.nonzero(r[v] <= eps)[0]:
            out[v, idx[j] // 64] |= np.uint64(1) << np.uint64(idx[j] % 64)
    return out


def enumerate_triples(hpoly, eps=EPS, min_det=1e-8):
    """All triples i < j < k of the unit rows in lexicographic order: the feasible intersections, merged in that order.
    Returns (verts (k, 3), smallest |det| among the triples whose point is feasible)."""
    n, d, _ = unit_rows(hpoly)
    m = len(n)
    if m < 3:
        return np.zeros((0, 3)), np.inf
    tri = np.array(list(itertools.combinations(range(m), 3)))
    a, b, c = n[tri[:, 0]], n[tri[:, 1]], n[tri[:, 2]]
    da, db, dc = d[tri[:, 0]], d[tri[:, 1]], d[tri[:, 2]]
    u, v, w = np.cross(b, c), np.cross(c, a), np.cross(a, b)
    det = np.einsum("ij,ij->i", a, u)
    ok = np.abs(det) >= min_det
    det, u, v, w, da, db, dc = det[ok], u[ok], v[ok], w[ok], da[ok], db[ok], dc[ok]
    x = -(da[:, None] * u + db[:, None] * v + dc[:, None] * w) / det[:, None]
    feas = np.ones(len(x), dtype=bool)
    for s in range(0, len(x), 1 << 16):
        feas[s:s + (1 << 16)] = np.all(x[s:s + (1 << 16)] @ n.T + d <= eps, axis=1)
    if not feas.any():
        return np.zeros((0, 3)), np.inf
    return merge(x[feas], eps), float(np.abs(det[feas]).min())


def hausdorff(a, b):
    """max-norm Hausdorff distance of two point sets."""
    dist = np.max(np.abs(a[:, None, :] - b[None, :, :]), axis=2)
    return float(max(dist.min(1).max(), dist.min(0).max()))


def match(a, b):
    """For every point of a the index of the nearest point of b (max-norm)."""
    return np.argmin(np.max(np.abs(a[:, None, :] - b[None, :, :]), axis=2), axis=1)


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------
def box(lo, hi):
    h = np.zeros((6, 4))
    for ax in range(3):
        h[2 * ax, ax] = 1.0; h[2 * ax, 3] = -hi[ax]
        h[2 * ax + 1, ax] = -1.0; h[2 * ax + 1, 3] = lo[ax]
    return h


def cube():
    return box([-1.0] * 3, [1.0] * 3)


def tetrahedron():
    return np.array([[-1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 1.0, 1.0, -1.0]])


def octahedron():
    return np.array([[sx, sy, sz, -1.0] for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)])


def dressed_cube():
    """The cube with two rows repeated at another scale, a row through the corner (1, 1, 1), a redundant row, padded to 16 rows."""
    h = np.zeros((16, 4))
    h[:6] = cube()
    h[6] = 3.0 * h[0]
    h[7] = 0.25 * h[3]
    h[9] = [1.0, 1.0, 1.0, -3.0]
    h[12] = [1.0, 0.0, 0.0, -5.0]
    return h


def cone(shift=(0.0, 0.0, 0.0)):
    """40 planes cos(th) x + sin(th) y + z / 2 <= 1 through the apex (0, 0, 2), and z >= 0: 41 vertices."""
    th = 2.0 * np.pi * (np.arange(40) + 0.3) / 40.0
    h = np.vstack([np.c_[np.cos(th), np.sin(th), np.full(40, 0.5), -np.ones(40)], [[0.0, 0.0, -1.0, 0.0]]])
    h[:, 3] -= h[:, :3] @ np.asarray(shift, dtype=np.float64)
    return h


def split_apex_pyramid(delta=2.2e-6):
    """A square pyramid (sides +-x + 2 z <= 2, +-y + 2 z <= 2, base z >= 0) with one side moved in by delta: the four sides no
    longer meet in the apex (0, 0, 1).  At epsilon = 1e-6 their four triples give four feasible points more than 1e-6 apart
    (two true vertices, two that violate the fourth side by delta / sqrt(5) = 0.98e-6): 8 vertices from 5 rows, more than
    2 * rows - 4 = 6."""
    return np.array([[1.0, 0.0, 2.0, -2.0 + delta], [-1.0, 0.0, 2.0, -2.0], [0.0, 1.0, 2.0, -2.0], [0.0, -1.0, 2.0, -2.0],
                     [0.0, 0.0, -1.0, 0.0]])


def sphere_tangents(H, seed):
    n = np.random.default_rng(seed).normal(size=(H, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return np.c_[n, -np.ones(H)]


def corridor_polytopes():
    """128 random corridor polytopes of 16 rows (6 to 12 of them set) in raw form."""
    from allocnet_amd.synth import corridor_problem
    hp = corridor_problem(np.random.default_rng(11), 32, 4, 3, 16)[4].reshape(128, 16, 4).copy()
    hp[:, :, 3] *= -1.0
    return hp
