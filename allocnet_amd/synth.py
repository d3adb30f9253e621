"""Synthetic problem generators of SURVEY.md section 8(d): random-walk waypoints (config 2), random SFC-like
corridors around the segments (configs 3-5), single corridor QPs and FIRI scenes.  Shared by bench.py, tools/ and
tests/ (tests/util.py re-exports them); no arithmetic of the solver lives here."""
import numpy as np


def random_problem(rng, B, N, c, rest=False):
    """Random-walk waypoints (SURVEY.md 8(d) config 2 generator)."""
    d = rng.normal(size=(B, N, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    d *= rng.uniform(1.0, 3.0, size=(B, N, 1))
    pts = np.concatenate([np.zeros((B, 1, 3)), np.cumsum(d, axis=1)], axis=1)
    pts[:, :, 2] = np.clip(pts[:, :, 2] + 1.0, 0.0, 5.0)
    head = np.zeros((B, 3, c)); tail = np.zeros((B, 3, c))
    head[:, :, 0] = pts[:, 0]; tail[:, :, 0] = pts[:, N]
    if not rest:
        head[:, :, 1:] = rng.normal(size=(B, 3, c - 1)) * 0.5
        tail[:, :, 1:] = rng.normal(size=(B, 3, c - 1)) * 0.5
    wps = pts[:, 1:N].copy()
    T = rng.uniform(0.5, 2.0, size=(B, N))
    return head, tail, wps, T


def corridor_problem(rng, B, N, c, M):
    """SURVEY 8(d) config 3 generator: random-walk waypoints, axis-aligned box around each segment
    inflated by U(0.5,3) plus k~U{0,6} random tangent half-spaces, rows normalised, a.x <= b, padded to M."""
    head, tail, wps, T = random_problem(rng, B, N, c, rest=True)
    pts = np.concatenate([head[:, None, :, 0], wps, tail[:, None, :, 0]], axis=1)
    hp = np.zeros((B, N, M, 4))
    lo = np.minimum(pts[:, :-1], pts[:, 1:]) - rng.uniform(0.5, 3.0, size=(B, N, 3))
    hi = np.maximum(pts[:, :-1], pts[:, 1:]) + rng.uniform(0.5, 3.0, size=(B, N, 3))
    for ax in range(3):
        hp[:, :, 2 * ax, ax] = 1.0; hp[:, :, 2 * ax, 3] = hi[:, :, ax]
        hp[:, :, 2 * ax + 1, ax] = -1.0; hp[:, :, 2 * ax + 1, 3] = -lo[:, :, ax]
    k = rng.integers(0, min(6, M - 6) + 1, size=(B, N))
    mid = 0.5 * (pts[:, :-1] + pts[:, 1:])
    for r in range(min(6, M - 6)):
        a = rng.normal(size=(B, N, 3)); a /= np.linalg.norm(a, axis=2, keepdims=True)
        b = np.einsum("bnk,bnk->bn", a, mid) + rng.uniform(1.0, 3.0, size=(B, N))
        use = (k > r)[..., None]
        hp[:, :, 6 + r, :3] = np.where(use, a, 0.0)
        hp[:, :, 6 + r, 3] = np.where(use[..., 0], b, 0.0)
    return head, tail, wps, T, hp


def qp_corridor_problem(rng, N, M, margin=1.0):
    pts = np.cumsum(np.vstack([np.zeros(3), rng.normal(size=(N, 3)) * 1.5]), axis=0)
    hp = np.zeros((N, M, 4))
    for i in range(N):
        lo = np.minimum(pts[i], pts[i + 1]) - margin
        hi = np.maximum(pts[i], pts[i + 1]) + margin
        for ax in range(3):
            hp[i, 2 * ax, ax] = 1.0; hp[i, 2 * ax, 3] = hi[ax]
            hp[i, 2 * ax + 1, ax] = -1.0; hp[i, 2 * ax + 1, 3] = -lo[ax]
        mid = 0.5 * (pts[i] + pts[i + 1])
        for r in range(6, M - 1):
            a = rng.normal(size=3); a /= np.linalg.norm(a)
            hp[i, r, :3] = a; hp[i, r, 3] = max(a @ pts[i], a @ pts[i + 1]) + rng.uniform(0.3, 1.5)
    ini = np.zeros((3, 3)); fin = np.zeros((3, 3))
    ini[:, 0] = pts[0]; fin[:, 0] = pts[-1]
    T = rng.uniform(1.5, 2.5, size=N)
    return ini, fin, hp, T


def firi_scene(rng, n_pts, clearance=0.5, box=3.0):
    a = rng.uniform(-2, 2, size=3)
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    b = a + d * rng.uniform(0.5, 2.5)
    lo = np.minimum(a, b) - box; hi = np.maximum(a, b) + box
    bd = np.zeros((6, 4))
    for ax in range(3):
        bd[2 * ax, ax] = 1.0; bd[2 * ax, 3] = -hi[ax]
        bd[2 * ax + 1, ax] = -1.0; bd[2 * ax + 1, 3] = lo[ax]
    pts = rng.uniform(lo + 1e-3, hi - 1e-3, size=(4 * n_pts, 3))
    dd = b - a
    t = np.clip(((pts - a) @ dd) / (dd @ dd), 0, 1)
    dist = np.linalg.norm(pts - (a + t[:, None] * dd), axis=1)
    pts = pts[dist > clearance][:n_pts]
    return bd, pts, a, b


def firi_pack(cases):
    B = len(cases)
    Np = max(1, max(len(c[1]) for c in cases))
    bd = np.array([c[0] for c in cases]); a = np.array([c[2] for c in cases]); b = np.array([c[3] for c in cases])
    pc = np.zeros((B, Np, 3)); npts = np.zeros(B, dtype=np.int32)
    for i, c in enumerate(cases):
        pc[i, :len(c[1])] = c[1]; npts[i] = len(c[1])
    return bd, pc, npts, a, b


def forest_cloud(rng, n_points=1_000_000, size=(40.0, 40.0, 5.0), origin=(-20.0, -20.0, 0.0), n_trees=120, n_boxes=20,
                 nan_frac=0.01, clear_route=None, clearance=1.0, point_step=16):
    """A synthetic scan of a forest: vertical cylinders (trees, radius U(0.15, 0.5), full height) and boxes sampled on
    their surfaces, as PointCloud2 float32 records of `point_step` bytes (x, y, z, then padding) -- an (n, point_step / 4)
    float32 array.  About nan_frac of the records are NaN (dropped returns).  clear_route: an optional polyline (m, 3)
    no obstacle comes within `clearance` of, so a corridor along it exists."""
    o = np.asarray(origin, dtype=np.float64); ext = np.asarray(size, dtype=np.float64)

    def clear(c, r):
        if clear_route is None:
            return True
        P = np.asarray(clear_route, dtype=np.float64)[:, :2]
        for a, b in zip(P[:-1], P[1:]):
            d = b - a
            t = np.clip((c - a) @ d / max(d @ d, 1e-12), 0.0, 1.0)
            if np.linalg.norm(c - (a + t * d)) < r + clearance:
                return False
        return True
    trees, boxes = [], []
    while len(trees) < n_trees:
        c = o[:2] + rng.uniform(0.0, 1.0, 2) * ext[:2]; r = rng.uniform(0.15, 0.5)
        if clear(c, r):
            trees.append((c, r))
    while len(boxes) < n_boxes:
        c = o[:2] + rng.uniform(0.0, 1.0, 2) * ext[:2]; h = rng.uniform(0.3, 1.5, 3)
        if clear(c, np.linalg.norm(h[:2])):
            boxes.append((c, h))
    n_tree_pts = int(n_points * 0.8); n_box_pts = n_points - n_tree_pts
    k = rng.integers(0, len(trees), n_tree_pts)
    cen = np.array([t[0] for t in trees])[k]; rad = np.array([t[1] for t in trees])[k]
    th = rng.uniform(0.0, 2.0 * np.pi, n_tree_pts)
    tree_pts = np.stack([cen[:, 0] + rad * np.cos(th), cen[:, 1] + rad * np.sin(th),
                         o[2] + rng.uniform(0.0, 1.0, n_tree_pts) * ext[2]], axis=1)
    k = rng.integers(0, len(boxes), n_box_pts)
    cen = np.array([b[0] for b in boxes])[k]; half = np.array([b[1] for b in boxes])[k]
    u = rng.uniform(-1.0, 1.0, (n_box_pts, 3))
    face = rng.integers(0, 3, n_box_pts)
    u[np.arange(n_box_pts), face] = np.sign(u[np.arange(n_box_pts), face])   # onto a face
    box_pts = np.stack([cen[:, 0], cen[:, 1], o[2] + half[:, 2]], axis=1) + u * half
    pts = np.concatenate([tree_pts, box_pts])[rng.permutation(n_points)]
    rec = np.zeros((n_points, point_step // 4), dtype=np.float32)
    rec[:, :3] = pts
    rec[rng.uniform(size=n_points) < nan_frac, :3] = np.nan
    return rec


def forest_route(origin=(-20.0, -20.0, 0.0), size=(40.0, 40.0, 5.0), z=1.5):
    """A five-leg polyline across the forest_cloud map (its clear_route)."""
    o = np.asarray(origin, dtype=np.float64); e = np.asarray(size, dtype=np.float64)
    f = np.array([[0.08, 0.08], [0.3, 0.22], [0.45, 0.5], [0.62, 0.55], [0.78, 0.8], [0.92, 0.92]])
    return np.concatenate([o[:2] + f * e[:2], np.full((len(f), 1), o[2] + z)], axis=1)
