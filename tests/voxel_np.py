"""numpy restatement of voxel_map::VoxelMap (gcopter/voxel_map.hpp, voxel_dilater.hpp), written from its semantics:
the fill truncates (pos - o) / scale toward zero and bounds-checks after the cast; dilate(r) runs r synchronous frontier
rounds over the 26-neighbourhood (round 1 from the voxels == 1, later rounds from the previous front, only into voxels
== 0, grown voxels = 2); the surface is the last front, here in ascending linear order; surface coordinates are
id * stepScale + oc in the offset form (x, y sx, z sx sy), a product and a sum (numpy does not fuse)."""
import numpy as np

UNOCCUPIED, OCCUPIED, DILATED = 0, 1, 2


def shifted(a, dz, dy, dx):
    """out[z, y, x] = a[z + dz, y + dy, x + dx], False outside the grid."""
    out = np.zeros_like(a)
    Z, Y, X = a.shape

    def sl(d, n):
        return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
    (oz, iz), (oy, iy), (ox, ix) = sl(dz, Z), sl(dy, Y), sl(dx, X)
    out[oz, oy, ox] = a[iz, iy, ix]
    return out


OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


class VoxelMapNP:
    def __init__(self, size, origin, scale):
        self.size = np.asarray(size, dtype=np.int64).reshape(3)
        self.o = np.asarray(origin, dtype=np.float64).reshape(3)
        self.scale = float(scale)
        self.step = np.array([1, self.size[0], self.size[0] * self.size[1]], dtype=np.int64)
        self.oc = self.o + 0.5 * self.scale
        self.step_scale = (1.0 / self.step.astype(np.float64)) * self.scale
        self.vox = np.zeros(int(np.prod(self.size)), dtype=np.uint8)
        self.surf = np.zeros(0, dtype=np.int64)

    def index(self, pos):
        """(ids (n,3) int64, inside (n,)): trunc((pos - o) / scale), inside when finite and in [0, size)."""
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.trunc((pos - self.o) / self.scale)
            inside = np.isfinite(t).all(axis=1) & (t >= 0).all(axis=1) & (t < self.size).all(axis=1)
        ids = np.where(inside[:, None], t, 0).astype(np.int64)
        return ids, inside

    def set_occupied(self, pos):
        ids, inside = self.index(pos)
        self.vox[ids[inside] @ self.step] = OCCUPIED

    def set_occupied_id(self, ids):
        """setOccupied(Eigen::Vector3i): in-bounds index triples are set, the rest dropped."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1, 3)
        inside = ((ids >= 0) & (ids < self.size)).all(axis=1)
        self.vox[ids[inside] @ self.step] = OCCUPIED

    def set_occupied_cloud(self, records):
        """float32 records (n, k >= 3); mapCallBack skips a record with a non-finite coordinate."""
        p = np.asarray(records)[:, :3].astype(np.float64)
        self.set_occupied(p[np.isfinite(p).all(axis=1)])

    def dilate(self, r):
        if r <= 0:
            return
        v = self.vox.reshape(self.size[2], self.size[1], self.size[0])
        front = v == OCCUPIED
        for _ in range(r):
            nb = np.zeros_like(front)
            for d in OFFSETS:
                nb |= shifted(front, *d)
            front = nb & (v == UNOCCUPIED)
            v[front] = DILATED
        self.surf = np.flatnonzero(front.reshape(-1))

    def xyz(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        sx, sxy = int(self.size[0]), int(self.size[0] * self.size[1])
        return np.stack([ids % sx, (ids % sxy) // sx, ids // sxy], axis=1)

    def surf_points(self, ids=None):
        off = (self.xyz(self.surf if ids is None else ids) * self.step).astype(np.float64)
        return off * self.step_scale + self.oc

    def surf_in_box(self, center, half_width):
        keep = (np.abs(self.xyz(self.surf) - np.asarray(center, dtype=np.int64)) <= half_width).all(axis=1)
        return self.surf_points(self.surf[keep])

    def query(self, pos):
        ids, inside = self.index(pos)
        out = np.ones(len(ids), dtype=bool)
        out[inside] = self.vox[ids[inside] @ self.step] != 0
        return out


def chebyshev_layers(grid01, r):
    """Brute force on a 0/1 grid (z, y, x): the result of dilate(r) -- 1 stays, 0 within Chebyshev distance r of a 1
    becomes 2 -- and the ids at distance exactly r (the surface)."""
    ones = np.argwhere(grid01 == 1)
    allv = np.argwhere(np.ones_like(grid01, dtype=bool))
    if len(ones):
        d = np.abs(allv[:, None, :] - ones[None, :, :]).max(axis=2).min(axis=1)
    else:
        d = np.full(len(allv), np.iinfo(np.int64).max)
    d = d.reshape(grid01.shape)
    out = grid01.copy()
    out[(grid01 == 0) & (d <= r)] = DILATED
    surf = np.flatnonzero(((grid01 == 0) & (d == r)).reshape(-1)) if r > 0 else None
    return out, surf


def box_filter(points, bd):
    """firi.py's per-segment selection: points with max_r(bd[r,:3] . p + bd[r,3]) < 0, in order."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if not len(points):
        return points
    return points[(points @ bd[:, :3].T + bd[:, 3]).max(axis=1) < 0.0]
