"""Vertex form of corridor polytopes: geo_utils::enumerateVs (gcopter/geo_utils.hpp:155-202, with filterVs :128-150) batched on
the device (anet_polytope_vertices; the semantics are stated once, in include/allocnet_amd.h), and what is built from the vertices
and their active-row masks on the host: faces, volume, and upstream GCOPTER's V-polytope list of a corridor.  Polytopes are in
GCOPTER's raw form, rows h with h.[x;1] <= 0; all-zero rows are padding."""
import ctypes

import numpy as np

from .context import default_context

POLYTOPE_OK, POLYTOPE_SKIPPED, POLYTOPE_TRUNCATED = 0, 1, 2
MAX_ROWS = 128


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pad(hpolys):
    if isinstance(hpolys, np.ndarray) and hpolys.ndim == 3:
        return np.ascontiguousarray(hpolys, dtype=np.float64)
    H = max(1, max((len(h) for h in hpolys), default=1))
    hp = np.zeros((len(hpolys), H, 4))
    for i, h in enumerate(hpolys):
        hp[i, :len(h)] = h
    return hp


def polytope_vertices(hpolys, epsilon=1e-6, with_active=False, ctx=None, max_vertices=None):
    """anet_polytope_vertices on a list of (n_i, 4) raw-form polytopes (or a zero-padded (B, H, 4) array), H <= 128.
    Returns (verts, status) or (verts, active, status): verts a list of (k_i, 3) arrays in the order of the first row triple that
    produced each vertex, active a list of (k_i, 2) uint64 masks (bit r % 64 of word r // 64: row r is tight at that vertex),
    status (B,) int32: 0 ok, 1 skipped (empty, flat, padding only or unbounded: no vertices), 2 more than max_vertices vertices
    (default 2 H - 4, enough for every non-degenerate polytope; the first max_vertices are returned)."""
    ctx = ctx or default_context()
    hp = _pad(hpolys)
    B, H, _ = hp.shape
    mv = int(max_vertices) if max_vertices is not None else max(4, 2 * H - 4)
    for _ in range(2):
        verts = np.zeros((B, mv, 3)); count = np.zeros(B, dtype=np.int32); status = np.zeros(B, dtype=np.int32)
        active = np.zeros((B, mv, 2), dtype=np.uint64) if with_active else None
        ctx.check(ctx.lib.anet_polytope_vertices(ctx.handle, B, H, _p(hp), float(epsilon), mv, _p(verts), _p(count),
                                                 _p(active) if with_active else None, _p(status)))
        if max_vertices is not None or B == 0 or int(count.max()) <= mv:
            break
        mv = int(count.max())       # a degenerate polytope with more than 2 H - 4 vertices: once more with room for all
    k = np.minimum(count, mv)
    vs = [verts[b, :k[b]].copy() for b in range(B)]
    if with_active:
        return vs, [active[b, :k[b]].copy() for b in range(B)], status
    return vs, status


def polytope_vertices_dev(hpoly, epsilon=1e-6, max_vertices=None, with_active=False, stream=None, ctx=None):
    """anet_polytope_vertices_dev: hpoly a torch CUDA float64 tensor (B, H, 4), zero-padded.  Nothing leaves the device;
    asynchronous on `stream` (default: torch's current stream).  Returns dict(verts (B, max_vertices, 3), count (B,) int32,
    status (B,) int32, active (B, max_vertices, 2) int64 holding the uint64 masks' bits, or None); slots behind count[b] are zero."""
    import torch
    ctx = ctx or default_context(hpoly.device.index or 0)
    if hpoly.dtype != torch.float64 or hpoly.dim() != 3 or hpoly.shape[2] != 4 or not hpoly.is_contiguous():
        raise ValueError("hpoly: contiguous float64 (B, H, 4)")
    B, H, _ = hpoly.shape
    mv = int(max_vertices) if max_vertices is not None else max(4, 2 * H - 4)
    dev = hpoly.device
    verts = torch.zeros(B, mv, 3, device=dev, dtype=torch.float64)
    count = torch.zeros(B, device=dev, dtype=torch.int32)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    active = torch.zeros(B, mv, 2, device=dev, dtype=torch.int64) if with_active else None
    q = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    ctx.check(ctx.lib.anet_polytope_vertices_dev(ctx.handle, B, H, q(hpoly), float(epsilon), mv, q(verts), q(count), q(active),
                                                 q(status), st))
    return dict(verts=verts, count=count, status=status, active=active)


def enumerate_vs(hpoly, epsilon=1e-6, ctx=None):
    """geo_utils::enumerateVs, the two-argument overload (geo_utils.hpp:184-202): (ok, (k, 3) vertices) of one raw-form polytope;
    ok is False where the reference finds no interior point."""
    vs, status = polytope_vertices([np.asarray(hpoly, dtype=np.float64).reshape(-1, 4)], epsilon, ctx=ctx)
    return bool(status[0] != POLYTOPE_SKIPPED), vs[0]


def _is_active(active, r):
    return (active[:, r // 64] >> np.uint64(r % 64)) & np.uint64(1) == np.uint64(1)


def polytope_faces(hpoly, verts, active):
    """The faces of one polytope from the active masks of its vertices: {row: vertex indices}, for every row of hpoly with at
    least three active vertices, ordered counter-clockwise seen from outside (about the row's outward normal).  Rows that
    describe the same plane give the same face once each."""
    hpoly = np.asarray(hpoly, dtype=np.float64).reshape(-1, 4)
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    active = np.asarray(active, dtype=np.uint64).reshape(-1, 2)
    faces = {}
    for r in range(len(hpoly)):
        n = hpoly[r, :3]
        if not n.any():
            continue
        idx = np.nonzero(_is_active(active, r))[0]
        if len(idx) < 3:
            continue
        n = n / np.linalg.norm(n)
        u = np.cross(n, np.eye(3)[np.argmin(np.abs(n))]); u /= np.linalg.norm(u)
        w = np.cross(n, u)                                  # (u, w, n) is right-handed
        d = verts[idx] - verts[idx].mean(0)
        faces[r] = idx[np.argsort(np.arctan2(d @ w, d @ u), kind="stable")]
    return faces


def polytope_volume(hpoly, verts=None, active=None, epsilon=1e-6, ctx=None):
    """Volume of one polytope: the pyramids (face area x height / 3) from the mean of its vertices to its faces.  verts and active
    as polytope_vertices(with_active=True) returns them; computed here when not given.  0.0 for a polytope without vertices."""
    hpoly = np.asarray(hpoly, dtype=np.float64).reshape(-1, 4)
    if verts is None or active is None:
        vs, act, _ = polytope_vertices([hpoly], epsilon, with_active=True, ctx=ctx)
        verts, active = vs[0], act[0]
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    if len(verts) < 4:
        return 0.0
    c = verts.mean(0)
    vol, seen = 0.0, set()
    for r, idx in polytope_faces(hpoly, verts, active).items():
        key = frozenset(idx.tolist())
        if key in seen:                                     # a second row for the same plane
            continue
        seen.add(key)
        n = hpoly[r, :3] / np.linalg.norm(hpoly[r, :3])
        p = verts[idx] - verts[idx[0]]
        area = 0.5 * float(np.cross(p[1:-1], p[2:]).sum(0) @ n)
        vol += area * float((verts[idx[0]] - c) @ n) / 3.0
    return vol


def corridor_vertices(hpolys, epsilon=1e-6, ctx=None):
    """Upstream GCOPTER's V-polytope list of a corridor of n polytopes: polytope 0, overlap(0, 1), polytope 1, ..., polytope n-1
    (2 n - 1 entries; an overlap is the two polytopes' rows stacked), all in ONE batched call.  Returns (list of (k, 3) arrays,
    status (2 n - 1,))."""
    def rows(h):
        h = np.asarray(h, dtype=np.float64).reshape(-1, 4)
        return h[np.any(h[:, :3] != 0.0, axis=1)]
    h = [rows(x) for x in hpolys]
    batch = []
    for i, x in enumerate(h):
        if i:
            batch.append(np.vstack([h[i - 1], x]))
        batch.append(x)
    return polytope_vertices(batch, epsilon, ctx=ctx)
