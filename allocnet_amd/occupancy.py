"""Occupancy from sensor scans on the device: a log-odds grid next to VoxelMap's bytes, updated scan by scan by ray carving
(allocnet_amd/csrc/occupancy_kernels.h) and handed over to a VoxelMap on demand.  A scan says three things a finished cloud
does not: the voxels between the sensor and a return are free, the voxels no ray has crossed are unknown, and a voxel seen
occupied once and seen through often enough becomes free again.  The grid is int16 per voxel in VoxelMap's order, UNKNOWN for
a voxel never observed; every rule is in include/allocnet_amd.h (anet_occupancy_*), and the grid is a function of the set of
rays of each scan, bit for bit."""
import ctypes
import math

import numpy as np

from ._lib import VoxelGrid, OccupancyParams, ANET_OCC_UNKNOWN
from .context import default_context
from .voxel_map import VoxelMap

UNKNOWN = ANET_OCC_UNKNOWN


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def occupancy_params(p_hit=0.7, p_miss=0.4, p_min=0.12, p_max=0.97, min_range=0.0, max_range=10.0, units=1000):
    """struct anet_occupancy_params from probabilities: units * logit(p), rounded to integers (hit > 0 > miss, lo < 0 < hi)."""
    def logit(p):
        return int(round(units * math.log(p / (1.0 - p))))
    prm = OccupancyParams()
    prm.hit, prm.miss, prm.lo, prm.hi = logit(p_hit), logit(p_miss), logit(p_min), logit(p_max)
    prm.min_range, prm.max_range = float(min_range), float(max_range)
    return prm


def depth_to_points_dev(depth, K, pose, step=1, depth_scale=1.0, min_depth=0.0, max_depth=math.inf, ctx=None):
    """anet_depth_to_points_dev on a CUDA tensor: depth (H, W) float32 metres or uint16 (int16 storage is read as uint16), K =
    (fx, fy, cx, cy) or a 3 x 3 intrinsic matrix, pose = (R (3, 3), t (3,)) or a 4 x 4 camera-to-world matrix.  -> (n, 3) float64
    CUDA tensor of the pixels (u, v) in {0, step, ...}^2, row-major, NaN rows for rejected pixels."""
    import torch
    ctx = ctx or default_context(depth.device.index or 0)
    u16 = tuple(d for d in (getattr(torch, "uint16", None), torch.int16) if d is not None)
    if depth.dim() != 2 or not depth.is_cuda or depth.dtype not in (torch.float32,) + u16:
        raise ValueError("depth_to_points_dev: depth must be an (H, W) float32 or uint16 CUDA tensor")
    depth = depth.contiguous()
    K = np.asarray(K, dtype=np.float64)
    k4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) if K.shape == (3, 3) else K.reshape(4)
    if isinstance(pose, (tuple, list)) and len(pose) == 2:
        R, t = np.asarray(pose[0], dtype=np.float64).reshape(3, 3), np.asarray(pose[1], dtype=np.float64).reshape(3)
    else:
        M = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        R, t = M[:3, :3], M[:3, 3]
    k4 = np.ascontiguousarray(k4); R = np.ascontiguousarray(R); t = np.ascontiguousarray(t)
    H, W = int(depth.shape[0]), int(depth.shape[1])
    step = int(step)
    if step < 1:
        raise ValueError("depth_to_points_dev: step >= 1")
    n = ((W + step - 1) // step) * ((H + step - 1) // step)
    out = torch.empty((n, 3), dtype=torch.float64, device=depth.device)
    st = ctypes.c_void_p(torch.cuda.current_stream(depth.device).cuda_stream)
    ctx.check(ctx.lib.anet_depth_to_points_dev(ctx.handle, _vp(depth), 0 if depth.dtype == torch.float32 else 1, W, H, step,
                                               float(depth_scale), k4.ctypes.data_as(ctypes.c_void_p),
                                               R.ctypes.data_as(ctypes.c_void_p), t.ctypes.data_as(ctypes.c_void_p),
                                               float(min_depth), float(max_depth), _vp(out), st))
    return out


class OccupancyMap:
    """OccupancyMap(size, origin, scale, params=None): the grid of a VoxelMap(size, origin, scale), as int16 log-odds."""

    def __init__(self, size, origin, scale, params=None, ctx=None):
        import torch
        self.ctx = ctx or default_context()
        self._size = np.asarray(size, dtype=np.int64).reshape(3)
        self._o = np.asarray(origin, dtype=np.float64).reshape(3).copy()
        self._scale = float(scale)
        self.params = params if params is not None else occupancy_params()
        self._grid = VoxelGrid()
        for c in range(3):
            self._grid.size[c] = int(self._size[c]); self._grid.origin[c] = float(self._o[c])
        self._grid.scale = self._scale
        ws = int(self.ctx.lib.anet_occupancy_workspace(ctypes.byref(self._grid)))
        if (self._size < 1).any() or int(np.prod(self._size)) >= 2 ** 31 or ws < 0:
            raise ValueError("OccupancyMap: sizes >= 1, fewer than 2^31 voxels, finite origin, scale > 0")
        self.device = torch.device("cuda", self.ctx.device)
        self._n = int(np.prod(self._size))
        self._logodds = torch.empty(self._n, dtype=torch.int16, device=self.device)
        self._work = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self.reset()

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def getSize(self):
        return self._size.astype(np.int32)

    def getScale(self):
        return self._scale

    def getOrigin(self):
        return self._o.copy()

    def reset(self):
        """Every voxel UNKNOWN again."""
        self.ctx.check(self.ctx.lib.anet_occupancy_reset_dev(self.ctx.handle, ctypes.byref(self._grid), _vp(self._logodds),
                                                             _vp(self._work), self._stream()))

    # ---- scans -------------------------------------------------------------------------------------
    def _integrate(self, t, n, stride, f64, sensor_origin):
        o = np.ascontiguousarray(np.asarray(sensor_origin, dtype=np.float64).reshape(3))
        self.ctx.check(self.ctx.lib.anet_occupancy_integrate_dev(
            self.ctx.handle, ctypes.byref(self._grid), ctypes.byref(self.params), _vp(self._logodds),
            o.ctypes.data_as(ctypes.c_void_p), _vp(t) if n else None, int(n), int(stride), int(f64), _vp(self._work), self._stream()))

    def integrate(self, points, sensor_origin):
        """One scan: points (n, k >= 3) float32 / float64 array or CUDA tensor in the world frame (first three columns x, y, z),
        seen from sensor_origin (3,).  Rows with a non-finite coordinate are skipped."""
        import torch
        t = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points))
        if t.dim() == 1:
            t = t.reshape(1, -1)
        if t.dim() != 2 or t.shape[1] < 3:
            raise ValueError("integrate: (n, 3) points expected")
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
        t = t.to(self.device).contiguous()
        self._integrate(t, t.shape[0], t.shape[1] * t.element_size(), 1 if t.dtype == torch.float64 else 0, sensor_origin)

    def integrateCloud(self, buf, point_step, sensor_origin):
        """One scan from raw PointCloud2 bytes in the world frame: records of `point_step` bytes, x, y, z float32 at offset 0."""
        import torch
        if isinstance(buf, torch.Tensor):
            t = buf.reshape(-1).view(torch.uint8)
        else:
            t = torch.from_numpy(np.frombuffer(memoryview(buf).cast("B"), dtype=np.uint8).copy())
        n = t.numel() // int(point_step)
        self._integrate(t.to(self.device).contiguous(), n, int(point_step), 0, sensor_origin)

    def integrateDepth(self, depth, K, pose, step=1, depth_scale=1.0, min_depth=0.0, max_depth=math.inf):
        """One scan from a depth image (depth_to_points_dev's arguments; a numpy image is uploaded): the unprojected points, seen
        from the camera centre pose's translation.  Returns the (n, 3) device points."""
        import torch
        if not isinstance(depth, torch.Tensor):
            a = np.ascontiguousarray(depth)
            depth = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
        depth = depth.to(self.device)
        pts = depth_to_points_dev(depth, K, pose, step, depth_scale, min_depth, max_depth, ctx=self.ctx)
        if isinstance(pose, (tuple, list)) and len(pose) == 2:
            cam = np.asarray(pose[1], dtype=np.float64).reshape(3)
        else:
            cam = np.asarray(pose, dtype=np.float64).reshape(4, 4)[:3, 3]
        self._integrate(pts, pts.shape[0], 24, 1, cam)
        return pts

    # ---- reading -----------------------------------------------------------------------------------
    def logodds_dev(self):
        """The device grid: int16 CUDA tensor, one value per voxel, x fastest; UNKNOWN where nothing was observed."""
        return self._logodds

    def getLogOdds(self):
        return self._logodds.cpu().numpy()

    def known_fraction(self):
        return float((self._logodds != UNKNOWN).sum().item()) / self._n

    def to_voxel_map(self, occ=0, unknown="blocked", dilate=0, out=None):
        """The grid as a VoxelMap of the same geometry (`out`: an existing one to overwrite): byte 1 where the log-odds are known
        and >= occ, and where they are unknown when unknown == "blocked"; 0 elsewhere.  dilate > 0: VoxelMap.dilate on top."""
        if unknown not in ("blocked", "free"):
            raise ValueError('to_voxel_map: unknown is "blocked" or "free"')
        vm = out if out is not None else VoxelMap(self._size, self._o, self._scale, ctx=self.ctx)
        if not (np.array_equal(vm._size, self._size) and np.array_equal(vm._o, self._o) and vm._scale == self._scale):
            raise ValueError("to_voxel_map: `out` must have this map's size, origin and scale")
        self.ctx.check(self.ctx.lib.anet_occupancy_to_voxels_dev(self.ctx.handle, ctypes.byref(self._grid), _vp(self._logodds), int(occ),
                                                                 1 if unknown == "blocked" else 0, _vp(vm.voxels_dev), self._stream()))
        vm._dist.clear()
        if dilate > 0:
            vm.dilate(dilate)
        return vm

    # ---- exploration goals (frontier.py) -----------------------------------------------------------
    def frontier(self, occ=0, box=None, out=None):
        """(mask uint8 CUDA (n_voxels,), count): the known voxels below `occ` with an unknown face neighbour inside the map, in
        the cell box (lo, ext) when one is given."""
        from .frontier import occupancy_frontier_dev
        return occupancy_frontier_dev(self, self._logodds, occ, box, out)

    def frontierClusters(self, occ=0, min_size=8, connectivity=26, box=None):
        """The frontier grouped into connected clusters of at least min_size voxels (frontier.frontier_clusters)."""
        from .frontier import frontier_clusters
        return frontier_clusters(self, occ, min_size, connectivity, box)

    def viewGain(self, view_R, view_t, pts, occ=0, work=None):
        """Per pose (R (V, 3, 3), t (V, 3); arrays or CUDA tensors) the number of distinct unknown voxels a scan with the
        sensor-frame template pts (R, 3) would cross, by this map's params: (V,) int32 numpy.  -1: a non-finite pose."""
        import torch
        from .frontier import view_gain_dev
        def dev(a, shape):
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
            return t.to(device=self.device, dtype=torch.float64).reshape(shape).contiguous()
        return view_gain_dev(self, self.params, self._logodds, dev(view_R, (-1, 9)), dev(view_t, (-1, 3)), dev(pts, (-1, 3)), occ,
                             work=work).cpu().numpy()
