"""numpy restatement of the log-odds occupancy grid (csrc/occupancy_kernels.h), written from the rules in include/allocnet_amd.h:
the walk of a segment over the grid, one scan (range test, truncation, marks, one update per marked voxel), the hand-over to
bytes, the unprojection of a depth image and the first hit of a segment on a byte grid.  Every floating-point operation is one
numpy operation, in the order of the header (numpy does not fuse), so the results are compared with the device's bit for bit.
All rays of a call walk in lockstep: one statement of the walk, `walk`, serves a single segment and a scan alike."""
import numpy as np

UNKNOWN = -32768
HIT_FREE = -1
HIT_INVALID = -3
MAX_SPAN = 65536
TIE = 1e-9
CELL_LIMIT = float(2 ** 30)


def cells_of(p, origin, scale):
    """(cells (n, 3) int64, ok (n,)): floor((p - origin) / scale) per axis; ok when every index is below 2^30 in magnitude."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((np.asarray(p, dtype=np.float64).reshape(-1, 3) - origin) / scale)
        ok = (np.abs(f) < CELL_LIMIT).all(axis=1)
    return np.where(ok[:, None], f, 0.0).astype(np.int64), ok


def walk(o, q, origin, scale, visit, max_span=MAX_SPAN + 1):
    """The walk of the segments o[i] -> q[i] ((n, 3) each).  visit(rows, cells, t, is_end) is called with the start cells (t = 0)
    and after every step with the cells just entered (t = the step's tm) of the rays `rows` still walking; it may return a bool
    array: True stops that ray.  Returns the (n,) mask of the rays that were walked (the others: a cell index out of range or a
    span above max_span on an axis)."""
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    origin = np.asarray(origin, dtype=np.float64).reshape(3)
    scale = float(scale)
    cur, ok1 = cells_of(o, origin, scale)
    end, ok2 = cells_of(q, origin, scale)
    ok = ok1 & ok2 & (np.abs(end - cur) <= max_span).all(axis=1)
    rows = np.flatnonzero(ok)
    o, q, cur, end = o[rows], q[rows], cur[rows], end[rows]
    d = q - o
    step = np.where(d > 0.0, 1, np.where(d < 0.0, -1, 0)).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        bnd = (cur + (step > 0)).astype(np.float64) * scale + origin
        tmax = np.where(step != 0, (bnd - o) / d, np.inf)
        tdel = np.where(step != 0, scale / np.abs(d), np.inf)
    at_end = (cur == end).all(axis=1)
    stop = visit(rows, cur.copy(), np.zeros(len(rows)), at_end)
    active = ~at_end if stop is None else ~at_end & ~stop
    while active.any():
        a = np.flatnonzero(active)
        c, e, tx = cur[a], end[a], tmax[a]
        rem = c != e
        tm = np.fmin.reduce(np.where(rem, tx, np.inf), axis=1)
        mask = rem & (tx <= (tm + TIE)[:, None])
        none = ~mask.any(axis=1)            # (unreachable: a remaining axis moves)
        if none.any():
            first = np.argmax(rem[none], axis=1)
            mask[np.flatnonzero(none), first] = True
        c = c + np.where(mask, step[a], 0)
        tx = np.where(mask, tx + tdel[a], tx)
        cur[a], tmax[a] = c, tx
        ae = (c == e).all(axis=1)
        stop = visit(rows[a], c, tm, ae)
        active[a] = ~ae if stop is None else ~ae & ~stop
    return ok


def walk_cells(o, q, origin, scale):
    """The visited cells of ONE segment, in order, as tuples."""
    out = []
    walk(np.asarray(o).reshape(1, 3), np.asarray(q).reshape(1, 3), origin, scale,
         lambda rows, cells, t, is_end: out.append(tuple(int(v) for v in cells[0])))
    return out


def linear_index(cells, size):
    """(ids, inside) of integer cells (n, 3) in a grid of `size`, x fastest."""
    size = np.asarray(size, dtype=np.int64)
    inside = ((cells >= 0) & (cells < size)).all(axis=1)
    ids = cells[:, 0] + size[0] * (cells[:, 1] + size[1] * cells[:, 2])
    return np.where(inside, ids, 0), inside


class Params:
    def __init__(self, hit=847, miss=-405, lo=-1992, hi=3476, min_range=0.0, max_range=10.0):
        self.hit, self.miss, self.lo, self.hi = int(hit), int(miss), int(lo), int(hi)
        self.min_range, self.max_range = float(min_range), float(max_range)


def rays_of(records, sensor, prm):
    """(q (m, 3), truncated (m,)) of the records that make a ray: finite, len >= min_range; longer than max_range: truncated."""
    p = np.asarray(records)[:, :3].astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    o = np.asarray(sensor, dtype=np.float64).reshape(3)
    d = p - o
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        keep = ~(ln < prm.min_range)
        p, d, ln = p[keep], d[keep], ln[keep]
        trunc = ln > prm.max_range
        r = prm.max_range / ln
        q = np.where(trunc[:, None], o + d * r[:, None], p)
    return q, trunc


def scan_marks(size, origin, scale, prm, sensor, records):
    """(hit, miss) bool per voxel: the marks of one scan before the update."""
    n = int(np.prod(size))
    hit = np.zeros(n, dtype=bool)
    miss = np.zeros(n, dtype=bool)
    q, trunc = rays_of(records, sensor, prm)
    o = np.broadcast_to(np.asarray(sensor, dtype=np.float64).reshape(3), q.shape)

    def visit(rows, cells, t, is_end):
        ids, inside = linear_index(cells, size)
        h = is_end & ~trunc[rows]
        hit[ids[inside & h]] = True
        miss[ids[inside & ~h]] = True

    walk(o, q, origin, scale, visit)
    return hit, miss


def integrate(logodds, size, origin, scale, prm, sensor, records):
    """One scan into logodds (int16, in place): one update per marked voxel, a hit mark winning; int32 arithmetic."""
    hit, miss = scan_marks(size, origin, scale, prm, sensor, records)
    L = np.where(logodds == UNKNOWN, 0, logodds).astype(np.int32)
    up = np.minimum(L + np.int32(prm.hit), np.int32(prm.hi))
    down = np.maximum(L + np.int32(prm.miss), np.int32(prm.lo))
    out = np.where(hit, up, np.where(miss, down, logodds.astype(np.int32)))
    logodds[:] = out.astype(np.int16)
    return logodds


def to_voxels(logodds, occ, unknown_blocked):
    known = logodds != UNKNOWN
    return np.where(known, logodds.astype(np.int32) >= int(occ), bool(unknown_blocked)).astype(np.uint8)


def depth_to_points(depth, K, R, t, step=1, depth_scale=1.0, min_depth=0.0, max_depth=np.inf):
    """(n, 3) float64 world points of the pixels (u, v), u, v in {0, step, ...}, row-major; NaN rows for rejected pixels."""
    depth = np.asarray(depth)
    fx, fy, cx, cy = (float(v) for v in K)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    sub = depth[::step, ::step]
    v, u = np.meshgrid(np.arange(0, depth.shape[0], step), np.arange(0, depth.shape[1], step), indexing="ij")
    u = u.reshape(-1).astype(np.float64)
    v = v.reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        z = sub.reshape(-1).astype(np.float64) * float(depth_scale)
        bad = ~np.isfinite(z) | (z <= min_depth) | (z > max_depth)
        x = (u - cx) / fx * z
        y = (v - cy) / fy * z
        out = np.stack([(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z + t[r] for r in range(3)], axis=1)
    out[bad] = np.nan
    return out


def raycast(vox, size, origin, scale, origins, ends):
    """(voxel (n,) int32, t (n,) float64) of the first visited in-bounds cell with a byte != 0."""
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    ends = np.asarray(ends, dtype=np.float64).reshape(-1, 3)
    n = len(origins)
    fin = np.flatnonzero(np.isfinite(origins).all(axis=1) & np.isfinite(ends).all(axis=1))
    first = np.full(len(fin), HIT_FREE, dtype=np.int32)     # of the finite rows; a blocked cell overwrites FREE and t = 1
    t_first = np.ones(len(fin))

    def visit(rows, cells, t, is_end):
        ids, inside = linear_index(cells, size)
        blocked = inside & (vox[ids] != 0)
        first[rows[blocked]] = ids[blocked]
        t_first[rows[blocked]] = t[blocked]
        return blocked

    ok = walk(origins[fin], ends[fin], origin, scale, visit, max_span=MAX_SPAN)
    voxel = np.full(n, HIT_INVALID, dtype=np.int32)
    t_out = np.full(n, np.nan)
    voxel[fin[ok]] = first[ok]
    t_out[fin[ok]] = t_first[ok]
    return voxel, t_out
