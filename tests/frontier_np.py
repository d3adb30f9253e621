"""numpy restatement of the exploration-goal kernels (csrc/frontier_kernels.h), written from the rules in include/allocnet_amd.h:
the frontier mask, connected components labelled by their least voxel index, the component table and the view gain.  The walk,
the rays and the scan are tests/occupancy_np.py's (`walk`, `rays_of`, `integrate`): nothing of them is restated here.  Integers
throughout, so the device's results are compared for equality."""
import numpy as np

from tests import occupancy_np as onp

UNKNOWN = onp.UNKNOWN

# (dx, dy, dz) of one half of the neighbourhood: each unordered pair once
FACES = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
HALF26 = [(dx, dy, dz) for dz in (0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]


def frontier(L, size, occ, box=None):
    """(mask uint8 (n,), count): known, below occ, inside the cell box (lo, ext), with an UNKNOWN face neighbour inside the map."""
    sx, sy, sz = (int(v) for v in size)
    G = np.asarray(L).reshape(sz, sy, sx)
    unk = G == UNKNOWN
    near = np.zeros_like(unk)
    near[:, :, 1:] |= unk[:, :, :-1]; near[:, :, :-1] |= unk[:, :, 1:]
    near[:, 1:, :] |= unk[:, :-1, :]; near[:, :-1, :] |= unk[:, 1:, :]
    near[1:, :, :] |= unk[:-1, :, :]; near[:-1, :, :] |= unk[1:, :, :]
    m = ~unk & (G.astype(np.int32) < int(occ)) & near
    if box is not None:
        lo, ext = np.asarray(box[0]).reshape(3), np.asarray(box[1]).reshape(3)
        inb = np.zeros_like(m)
        inb[lo[2]:lo[2] + ext[2], lo[1]:lo[1] + ext[1], lo[0]:lo[0] + ext[0]] = True
        m &= inb
    return m.reshape(-1).astype(np.uint8), int(m.sum())


def label_components(mask, size, connectivity):
    """labels int32 (n,): -1 where mask == 0, else the least linear index of the voxel's component (6 or 26 neighbours).  A
    union-find over the neighbour pairs, the larger root always linked to the smaller, so a root is its set's least index."""
    sx, sy, sz = (int(v) for v in size)
    M = np.asarray(mask).reshape(sz, sy, sx) != 0
    idx = np.arange(sx * sy * sz, dtype=np.int64).reshape(sz, sy, sx)
    parent = np.arange(sx * sy * sz, dtype=np.int64)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def sl(d, n):
        return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))

    for dx, dy, dz in (FACES if connectivity == 6 else HALF26):
        (az, bz), (ay, by), (ax, bx) = sl(dz, sz), sl(dy, sy), sl(dx, sx)
        both = M[az, ay, ax] & M[bz, by, bx]
        for a, b in zip(idx[az, ay, ax][both].tolist(), idx[bz, by, bx][both].tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    flat = M.reshape(-1)
    out = np.full(flat.size, -1, dtype=np.int32)
    for v in np.flatnonzero(flat).tolist():
        out[v] = find(v)
    return out


def component_stats(labels, size):
    """(root (k,), count (k,), sum_xyz (k, 3) int64, bbox (k, 6)) in ascending root order."""
    sx, sy, _ = (int(v) for v in size)
    labels = np.asarray(labels)
    v = np.flatnonzero(labels >= 0)
    root, inv = np.unique(labels[v], return_inverse=True)
    xyz = np.stack([v % sx, (v // sx) % sy, v // (sx * sy)], axis=1).astype(np.int64)
    k = len(root)
    count = np.bincount(inv, minlength=k).astype(np.int32)
    sums = np.zeros((k, 3), dtype=np.int64)
    lo = np.full((k, 3), np.iinfo(np.int32).max, dtype=np.int64)
    hi = np.full((k, 3), -1, dtype=np.int64)
    np.add.at(sums, inv, xyz)
    np.minimum.at(lo, inv, xyz)
    np.maximum.at(hi, inv, xyz)
    return root.astype(np.int32), count, sums, np.concatenate([lo, hi], axis=1).astype(np.int32)


def world_points(R, t, pts):
    """(R0 x + R1 y) + R2 z + t, each operation rounded on its own (k_depth_to_points' expression)."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(R[c, 0] * p[:, 0] + R[c, 1] * p[:, 1]) + R[c, 2] * p[:, 2] + t[c] for c in range(3)], axis=1)


def view_cells(L, size, origin, scale, prm, occ, R, t, pts):
    """The set U_v of one view as a bool array over the voxels, or None for a view with a non-finite entry."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return None
    L = np.asarray(L)
    seen = np.zeros(L.size, dtype=bool)
    q, _ = onp.rays_of(world_points(R, t, pts), t, prm)
    if len(q) == 0:
        return seen
    o = np.broadcast_to(t, q.shape)

    def visit(rows, cells, tt, is_end):
        ids, inside = onp.linear_index(cells, size)
        l = L[ids]
        unknown = inside & (l == UNKNOWN)
        seen[ids[unknown]] = True
        return inside & ~unknown & (l.astype(np.int32) >= int(occ))

    onp.walk(o, q, origin, scale, visit)
    return seen


def view_gain(L, size, origin, scale, prm, occ, view_R, view_t, pts):
    """gain int32 (V,): the number of distinct UNKNOWN voxels the rays of each view cross before an occupied one; -1 for a view
    with a non-finite entry in R or t."""
    view_R = np.asarray(view_R, dtype=np.float64).reshape(-1, 3, 3)
    view_t = np.asarray(view_t, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(view_t), dtype=np.int32)
    for v in range(len(view_t)):
        seen = view_cells(L, size, origin, scale, prm, occ, view_R[v], view_t[v], pts)
        out[v] = -1 if seen is None else int(seen.sum())
    return out


def clusters(L, size, origin, scale, occ, min_size, connectivity, box=None):
    """The table of frontier clusters with at least min_size voxels: (root, count, centroid (k, 3) world, cells lo / hi)."""
    mask, _ = frontier(L, size, occ, box)
    root, count, sums, bbox = component_stats(label_components(mask, size, connectivity), size)
    keep = count >= min_size
    cen = np.asarray(origin, dtype=np.float64) + (sums[keep].astype(np.float64) / count[keep][:, None] + 0.5) * scale
    return root[keep], count[keep], cen, bbox[keep][:, :3], bbox[keep][:, 3:]
