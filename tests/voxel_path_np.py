"""numpy / scipy restatement of the device path search (allocnet_amd/csrc/path_kernels.h, include/allocnet_amd.h):
the cost-to-come field is scipy's Dijkstra on the no-corner-cutting 26-neighbour graph (integer weights 10 / 14 / 17, so
the float64 sums are exact), then the target, the walk, the DDA, the greedy shortcut and the cost in the kernels'
operation order, in Python floats (IEEE double, never fused)."""
import math

import numpy as np

from tests.voxel_np import VoxelMapNP, shifted  # noqa: F401  (VoxelMapNP: the map this works on)

INF32 = 0xFFFFFFFF
EXACT, APPROXIMATE, INVALID_START = 0, 1, 2
TIE_EPS = 1e-9   # the DDA's tie window in the segment parameter (path_kernels.h kPathTieEps)
# the walk's candidate order: dz, then dy, then dx, each ascending over {-1, 0, 1}
MOVES = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def weight(d):
    return {1: 10, 2: 14, 3: 17}[sum(c != 0 for c in d)]


def block(d):
    """the voxels a move by d spans: cur + e, e_i in {0, d_i}"""
    dx, dy, dz = d
    return {(ex, ey, ez) for ex in {0, dx} for ey in {0, dy} for ez in {0, dz}}


class PathNP:
    def __init__(self, m, lb=None, hb=None):
        self.m = m
        self.sx, self.sy, self.sz = (int(v) for v in m.size)
        self.n = self.sx * self.sy * self.sz
        self.scale = float(m.scale)
        self.o = [float(v) for v in m.o]
        self.oc = [float(v) for v in m.oc]
        corner = m.size.astype(np.float64) * m.scale + m.o
        self.lb = np.asarray(m.o if lb is None else lb, dtype=np.float64).reshape(3)
        self.hb = np.asarray(corner if hb is None else hb, dtype=np.float64).reshape(3)
        ins = []
        for c, s in enumerate((self.sx, self.sy, self.sz)):
            cen = np.arange(s).astype(np.float64) * m.scale + m.oc[c]
            ins.append((cen >= self.lb[c]) & (cen <= self.hb[c]))
        v = m.vox.reshape(self.sz, self.sy, self.sx)
        self.free = (v == 0) & ins[2][:, None, None] & ins[1][None, :, None] & ins[0][None, None, :]   # (z, y, x)

    # ---- voxels ---------------------------------------------------------------------------------------
    def xyz(self, i):
        i = int(i)
        sxy = self.sx * self.sy
        z = i // sxy
        y = (i - z * sxy) // self.sx
        return i - z * sxy - y * self.sx, y, z

    def is_free(self, x, y, z):
        return 0 <= x < self.sx and 0 <= y < self.sy and 0 <= z < self.sz and bool(self.free[z, y, x])

    def free_voxel(self, p):
        """the voxel of position p when it is free, else -1"""
        ids, inside = self.m.index(np.asarray(p, dtype=np.float64).reshape(1, 3))
        if not inside[0]:
            return -1
        x, y, z = (int(v) for v in ids[0])
        return x + self.sx * (y + self.sy * z) if self.free[z, y, x] else -1

    def centre(self, i):
        x, y, z = self.xyz(i)
        return [float(x) * self.scale + self.oc[0], float(y) * self.scale + self.oc[1], float(z) * self.scale + self.oc[2]]

    def edge(self, x, y, z, d):
        return all(self.is_free(x + ex, y + ey, z + ez) for ex, ey, ez in block(d))

    # ---- field ----------------------------------------------------------------------------------------
    def graph(self):
        """the undirected graph as a CSR matrix over the 13 moves whose first non-zero of (dz, dy, dx) is positive"""
        from scipy.sparse import csr_matrix
        src, dst, wt = [], [], []
        ids = np.arange(self.n, dtype=np.int64).reshape(self.sz, self.sy, self.sx)
        for d in MOVES[13:]:
            ok = np.ones_like(self.free)
            for ex, ey, ez in block(d):
                ok &= shifted(self.free, ez, ey, ex)
            s = ids[ok]
            src.append(s); dst.append(s + d[0] + self.sx * (d[1] + self.sy * d[2]))
            wt.append(np.full(len(s), float(weight(d))))
        src, dst, wt = np.concatenate(src), np.concatenate(dst), np.concatenate(wt)
        return csr_matrix((wt, (src, dst)), shape=(self.n, self.n))

    def fields(self, starts, graph=None):
        """(B, n) uint32 cost-to-come fields, INF32 unreached; all INF32 for a start that is not free"""
        from scipy.sparse.csgraph import dijkstra
        starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
        out = np.full((len(starts), self.n), INF32, dtype=np.uint32)
        sv = [self.free_voxel(s) for s in starts]
        ok = [b for b, v in enumerate(sv) if v >= 0]
        if ok:
            g = self.graph() if graph is None else graph
            d = dijkstra(g, directed=False, indices=[sv[b] for b in ok])
            for r, b in enumerate(ok):
                out[b] = np.where(np.isinf(d[r]), INF32, d[r]).astype(np.uint32)
        return out

    # ---- target, walk, waypoints ------------------------------------------------------------------------
    def target(self, field, s, g):
        sv, gv = self.free_voxel(s), self.free_voxel(g)
        if sv < 0 or field[sv] != 0:
            return INVALID_START, -1, sv
        if gv >= 0 and field[gv] != INF32:
            return EXACT, gv, sv
        reached = np.flatnonzero(field != INF32)
        sxy = self.sx * self.sy
        z = reached // sxy; y = (reached - z * sxy) // self.sx; x = reached - z * sxy - y * self.sx
        g = np.asarray(g, dtype=np.float64).reshape(3)
        dx = (x.astype(np.float64) * self.scale + self.oc[0]) - g[0]
        dy = (y.astype(np.float64) * self.scale + self.oc[1]) - g[1]
        dz = (z.astype(np.float64) * self.scale + self.oc[2]) - g[2]
        d2 = dx * dx + dy * dy + dz * dz
        d2 = np.where(np.isnan(d2), np.inf, d2)
        return APPROXIMATE, int(reached[d2 == d2.min()].min()), sv

    def walk(self, field, target, start):
        """voxels from the target to the start"""
        cur, out = target, [target]
        while cur != start:
            x, y, z = self.xyz(cur)
            dcur = int(field[cur])
            for d in MOVES:
                nx, ny, nz = x + d[0], y + d[1], z + d[2]
                if not self.is_free(nx, ny, nz) or not self.edge(x, y, z, d):
                    continue
                dn = int(field[nx + self.sx * (ny + self.sy * nz)])
                if dn != INF32 and dn + weight(d) == dcur:
                    cur = nx + self.sx * (ny + self.sy * nz)
                    break
            else:
                raise AssertionError("no predecessor")
            out.append(cur)
        return out

    def waypoints(self, walk, s, g, status):
        s = [float(v) for v in s]; g = [float(v) for v in g]
        W = [s] + [self.centre(v) for v in walk[::-1][1:]]
        if len(walk) == 1:
            W.append(g if status == EXACT else self.centre(walk[0]))
        elif status == EXACT:
            W[-1] = g
        return W

    # ---- shortcut -----------------------------------------------------------------------------------------
    def visible(self, P, Q):
        """3-D DDA (Amanatides-Woo) from P to Q: only axes with moves left take part; crossings within TIE_EPS of the
        nearest one tie, and a tie checks the whole block"""
        size = (self.sx, self.sy, self.sz)
        cur, end, step, tmax, tdel = [0] * 3, [0] * 3, [0] * 3, [0.0] * 3, [0.0] * 3
        for c in range(3):
            cur[c] = min(max(int((P[c] - self.o[c]) / self.scale), 0), size[c] - 1)
            end[c] = min(max(int((Q[c] - self.o[c]) / self.scale), 0), size[c] - 1)
            d = Q[c] - P[c]
            step[c] = 1 if d > 0.0 else -1 if d < 0.0 else 0
            if step[c] == 0:
                tmax[c] = tdel[c] = math.inf
            else:
                bnd = float(cur[c] + (1 if step[c] > 0 else 0)) * self.scale + self.o[c]
                tmax[c] = (bnd - P[c]) / d
                tdel[c] = self.scale / abs(d)
        if not self.is_free(*cur):
            return False
        while cur != end:
            tm = math.inf
            for c in range(3):
                if cur[c] != end[c] and tmax[c] < tm:
                    tm = tmax[c]
            axes = [c for c in range(3) if cur[c] != end[c] and tmax[c] <= tm + TIE_EPS]
            for e in range(1, 8):
                if any((e >> c) & 1 and c not in axes for c in range(3)):
                    continue
                v = [cur[c] + (step[c] if (e >> c) & 1 else 0) for c in range(3)]
                if not self.is_free(*v):
                    return False
            for c in axes:
                cur[c] += step[c]
                tmax[c] = tmax[c] + tdel[c]
        return True

    def shortcut(self, W):
        i, out = 0, [W[0]]
        M = len(W) - 1
        while i < M:
            best = next(k for k in range(M, i, -1) if self.visible(W[i], W[k]))   # the largest visible k
            i = best
            out.append(W[i])
        return out

    @staticmethod
    def cost(path):
        c = 0.0
        for p, q in zip(path[:-1], path[1:]):
            dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
            c = c + math.sqrt(dx * dx + dy * dy + dz * dz)
        return c

    # ---- all of it -----------------------------------------------------------------------------------------
    def plan(self, s, g, field=None):
        """(cost, path (m, 3) float64, status) of planPath(s, g) on this map and box"""
        if field is None:
            field = self.fields([s])[0]
        status, tgt, sv = self.target(field, s, g)
        if status == INVALID_START:
            return math.inf, np.zeros((0, 3)), status
        path = self.shortcut(self.waypoints(self.walk(field, tgt, sv), s, g, status))
        return self.cost(path), np.asarray(path, dtype=np.float64).reshape(-1, 3), status


def make_map(size, origin, scale, occupied_xyz=()):
    m = VoxelMapNP(size, origin, scale)
    for x, y, z in occupied_xyz:
        m.vox[x + size[0] * (y + size[1] * z)] = 1
    return m
