"""voxel_map::VoxelMap (gcopter/voxel_map.hpp, voxel_dilater.hpp) on the device: the occupancy grid the online planner
fills from a point cloud, dilates and hands to convexCover (learning_planning.cpp mapCallBack, learning_planner.hpp plan).
The voxel bytes live in a torch CUDA tensor; fill, dilation, surface, query and the corridor's per-segment point
selection are HIP kernels (allocnet_amd/csrc/voxel_kernels.h).  Voxels are byte-identical to the reference's and surface
coordinates bit-identical; the surface is in ascending voxel index order (x fastest), where the reference's is in
breadth-first discovery order -- the same set."""
import ctypes

import numpy as np

from ._lib import VoxelGrid, ANET_DIST_NONE
from .context import default_context

Unoccupied = 0
Occupied = 1
Dilated = 2
DIST_NONE = ANET_DIST_NONE    # the distance field's value for a minimum over nothing (+: no blocked voxel, -: no free one)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


class VoxelMap:
    """VoxelMap(size, origin, scale): size (3,) voxel counts, origin (3,) the low corner, scale the voxel edge length."""
    Unoccupied = Unoccupied
    Occupied = Occupied
    Dilated = Dilated

    def __init__(self, size, origin, scale, ctx=None):
        import torch
        self.ctx = ctx or default_context()
        self._size = np.asarray(size, dtype=np.int64).reshape(3)
        self._o = np.asarray(origin, dtype=np.float64).reshape(3).copy()
        self._scale = float(scale)
        self._grid = VoxelGrid()
        for c in range(3):
            self._grid.size[c] = int(self._size[c]); self._grid.origin[c] = float(self._o[c])
        self._grid.scale = self._scale
        self._ws_bytes = int(self.ctx.lib.anet_voxel_workspace(ctypes.byref(self._grid)))
        if (self._size < 1).any() or int(np.prod(self._size)) >= 2 ** 31 or self._ws_bytes < 0:
            raise ValueError("VoxelMap: sizes >= 1, fewer than 2^31 voxels, finite origin, scale > 0")
        self.device = torch.device("cuda", self.ctx.device)
        n = int(np.prod(self._size))
        self._vox = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._work = None
        self._ids = torch.zeros(0, dtype=torch.int32, device=self.device)
        self._count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._surf_pts = None
        self._dist = {}                     # the distance fields, per `walls`; dropped by whatever changes the voxel bytes
        # voxel_map.hpp's derived members: oc = o + 0.5 scale, stepScale = (1 / step) scale (numpy does not fuse)
        self._step = np.array([1, self._size[0], self._size[0] * self._size[1]], dtype=np.int64)
        self._oc = self._o + 0.5 * self._scale
        self._step_scale = (1.0 / self._step.astype(np.float64)) * self._scale

    # ---- the reference's accessors ---------------------------------------------------------------
    def getSize(self):
        return self._size.astype(np.int32)

    def getScale(self):
        return self._scale

    def getOrigin(self):
        return self._o.copy()

    def getCorner(self):
        return self._size.astype(np.float64) * self._scale + self._o

    def getVoxels(self):
        """Host copy of the voxel bytes, x fastest."""
        return self._vox.cpu().numpy()

    @property
    def voxels_dev(self):
        """The device voxel bytes (uint8, one per voxel, x fastest); writes through it bypass the map's bookkeeping (a cached
        distance field does not see them: distance_field(refresh=True))."""
        return self._vox

    @property
    def surf_ids_dev(self):
        """Device int32 linear ids of the surface, ascending."""
        return self._ids

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- fill --------------------------------------------------------------------------------------
    def setOccupied(self, points):
        """setOccupied(pos) for every row of points: an (n, k >= 3) float32 / float64 array or CUDA tensor (first three
        columns x, y, z).  Rows with a non-finite coordinate are skipped; points outside the map are dropped.
        Integer rows are voxel indices (the reference's setOccupied(Eigen::Vector3i)): in-bounds ones are set directly."""
        import torch
        t = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points))
        if t.dim() == 1:
            t = t.reshape(1, -1)
        if t.dim() != 2 or t.shape[1] < 3:
            raise ValueError("setOccupied: (n, 3) points expected")
        if not (t.is_floating_point() or t.dtype == torch.bool):
            # out-of-int32 values clamp to values that are out of bounds as well, before the narrowing conversion
            ids = t[:, :3].to(device=self.device, dtype=torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
            self.ctx.check(self.ctx.lib.anet_voxel_set_occupied_ids_dev(self.ctx.handle, ctypes.byref(self._grid), _vp(self._vox),
                                                                        _vp(ids), ids.shape[0], self._stream()))
            self._dist.clear()
            return
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
        t = t.to(self.device).contiguous()
        self._scatter(t, t.shape[0], t.shape[1] * t.element_size(), 1 if t.dtype == torch.float64 else 0)

    def setOccupiedCloud(self, buf, point_step):
        """mapCallBack's fill from raw PointCloud2 bytes: records of `point_step` bytes, x, y, z float32 at offset 0."""
        import torch
        if isinstance(buf, torch.Tensor):
            t = buf.reshape(-1).view(torch.uint8)
        else:
            t = torch.from_numpy(np.frombuffer(memoryview(buf).cast("B"), dtype=np.uint8).copy())
        n = t.numel() // int(point_step)
        self._scatter(t.to(self.device).contiguous(), n, int(point_step), 0)

    def _scatter(self, t, n, stride, f64):
        self.ctx.check(self.ctx.lib.anet_voxel_set_occupied_dev(self.ctx.handle, ctypes.byref(self._grid), _vp(self._vox), _vp(t),
                                                                int(n), int(stride), int(f64), self._stream()))
        self._dist.clear()

    # ---- dilation and surface ---------------------------------------------------------------------
    def dilate(self, r):
        """dilate(r): r <= 0 does nothing (the surface keeps what it held); otherwise r frontier rounds, and the surface
        becomes the voxels the last round added."""
        import torch
        r = int(r)
        if r <= 0:
            return
        if self._work is None:
            self._work = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
        lib, h, g, st = self.ctx.lib, self.ctx.handle, ctypes.byref(self._grid), self._stream()
        self.ctx.check(lib.anet_voxel_dilate_dev(h, g, _vp(self._vox), r, _vp(self._work), st))
        self._dist.clear()
        cap = max(self._ids.numel(), 1024)
        ids = torch.empty(cap, dtype=torch.int32, device=self.device)
        self.ctx.check(lib.anet_voxel_surface_dev(h, g, _vp(self._work), cap, _vp(ids), _vp(self._count), st))
        n = int(self._count.item())
        if n > cap:  # the last front is still in the workspace: compact again into a buffer that fits
            ids = torch.empty(n, dtype=torch.int32, device=self.device)
            self.ctx.check(lib.anet_voxel_surface_dev(h, g, _vp(self._work), n, _vp(ids), _vp(self._count), self._stream()))
        self._ids = ids[:n]
        self._surf_pts = None

    def surf_points_dev(self):
        """getSurf on the device: (n, 3) float64 CUDA tensor, ascending voxel order."""
        import torch
        if self._surf_pts is None:
            n = self._ids.numel()
            out = torch.empty((n, 3), dtype=torch.float64, device=self.device)
            self.ctx.check(self.ctx.lib.anet_voxel_surf_points_dev(self.ctx.handle, ctypes.byref(self._grid), _vp(self._ids), n,
                                                                   _vp(out), self._stream()))
            self._surf_pts = out
        return self._surf_pts

    def getSurf(self):
        """(n, 3) float64: id * stepScale + oc per surface voxel, the reference's two roundings."""
        return self.surf_points_dev().cpu().numpy()

    def getSurfIds(self):
        """Host copy of the surface's linear voxel ids (ascending)."""
        return self._ids.cpu().numpy()

    def getSurfInBox(self, center, halfWidth):
        """Surface points whose integer voxel index is within halfWidth of center on every axis (Chebyshev box)."""
        c = np.asarray(center, dtype=np.int64).reshape(3)
        ids = self.getSurfIds().astype(np.int64)
        sx, sxy = int(self._size[0]), int(self._size[0] * self._size[1])
        xyz = np.stack([ids % sx, (ids % sxy) // sx, ids // sxy], axis=1)
        keep = (np.abs(xyz - c) <= int(halfWidth)).all(axis=1)
        return self.getSurf()[keep]

    # ---- queries -----------------------------------------------------------------------------------
    def query(self, pos):
        """query(pos) per row: True outside the map or in a voxel != 0.  (n, 3) -> bool (n,); one 3-vector -> bool."""
        import torch
        single = np.ndim(pos) == 1 if not isinstance(pos, torch.Tensor) else pos.dim() == 1
        t = pos if isinstance(pos, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64))
        t = t.to(device=self.device, dtype=torch.float64).reshape(-1, 3).contiguous()
        out = torch.empty(t.shape[0], dtype=torch.uint8, device=self.device)
        self.ctx.check(self.ctx.lib.anet_voxel_query_dev(self.ctx.handle, ctypes.byref(self._grid), _vp(self._vox), _vp(t),
                                                         t.shape[0], _vp(out), self._stream()))
        res = out.cpu().numpy().astype(bool)
        return bool(res[0]) if single else res

    # ---- the distance field ---------------------------------------------------------------------------
    def distance_field(self, walls=True, refresh=False):
        """The exact signed squared distance field of the map (anet_voxel_distance_dev): int32 CUDA tensor, one value per voxel
        in the layout of the bytes, + to the nearest blocked voxel for a free one, - to the nearest free voxel for a blocked one,
        in voxel units; walls: the outside of the map counts as blocked.  Cached per `walls` and dropped by setOccupied,
        setOccupiedCloud and dilate; writes through voxels_dev bypass the cache: refresh=True computes it again."""
        key = bool(walls)
        if refresh or key not in self._dist:
            self._dist[key] = distance_transform_dev(self, self._vox, key, out=self._dist.get(key))
        return self._dist[key]

    def getDistance(self, pos, grad=False, walls=True):
        """The distance in metres from pos to the nearest obstacle (negative inside one): the trilinear interpolant of the field's
        centre values (anet_voxel_distance_query_dev), constant beyond the outermost voxel centres.  One 3-vector -> float, (n, 3)
        -> (n,) numpy; grad=True returns (dist, gradient) with the gradient (3,) / (n, 3)."""
        import torch
        single = np.ndim(pos) == 1 if not isinstance(pos, torch.Tensor) else pos.dim() == 1
        t = pos if isinstance(pos, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64))
        t = t.to(device=self.device, dtype=torch.float64).reshape(-1, 3).contiguous()
        d, g = distance_query_dev(self, self.distance_field(walls), t, grad=grad)
        d = d.cpu().numpy()
        if not grad:
            return float(d[0]) if single else d
        g = g.cpu().numpy()
        return (float(d[0]), g[0]) if single else (d, g)

    def raycast(self, origins, ends):
        """First hit of the segments origins[i] -> ends[i] ((n, 3) each, or one 3-vector each) on the voxel bytes, by the walk of
        anet_voxel_raycast_dev: (voxel int32 (n,), t float64 (n,)) numpy -- the linear index of the first visited voxel != 0 and the
        parameter in [0, 1] it was entered at, HIT_FREE / t = 1 without one, HIT_INVALID / NaN for a row that cannot be walked.
        Unlike query, the outside of the map is NOT blocked: it is passed through."""
        import torch
        single = np.ndim(origins) == 1 if not isinstance(origins, torch.Tensor) else origins.dim() == 1
        def dev(a):
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
            return t.to(device=self.device, dtype=torch.float64).reshape(-1, 3).contiguous()
        voxel, t = voxel_raycast_dev(self, self._vox, dev(origins), dev(ends))
        voxel, t = voxel.cpu().numpy(), t.cpu().numpy()
        return (int(voxel[0]), float(t[0])) if single else (voxel, t)

    def posI2D(self, id):
        """id * scale + oc (a different rounding from the surface's id * stepScale + oc, as in the reference)."""
        return np.asarray(id).astype(np.float64) * self._scale + self._oc

    def posD2I(self, pos):
        """((pos - o) / scale) truncated toward zero."""
        return ((np.asarray(pos, dtype=np.float64) - self._o) / self._scale).astype(np.int32)

    # ---- planPath's field --------------------------------------------------------------------------
    def path_field_dev(self, starts, lb=None, hb=None):
        """Cost-to-come fields of the starts (B, 3) over the free voxels of [lb, hb] (default the map's box): ((B, n_voxels)
        uint32 CUDA tensor view, valid until the map's next search; rounds).  See path_search.plan_path."""
        from .path_search import path_field_dev
        return path_field_dev(self, starts, lb, hb)

    # ---- connectivity of the free space -------------------------------------------------------------
    def components(self, connectivity=26, free=True):
        """Connected components of the free voxels (free=False: of the blocked ones): int32 CUDA labels (n_voxels,), -1 off the
        set, else the least voxel index of the component -- two voxels are mutually reachable exactly when their labels agree."""
        from .frontier import label_components_dev
        mask = (self._vox == 0) if free else (self._vox != 0)
        return label_components_dev(self, mask.to(self._vox.dtype), connectivity)

    # ---- convexCover's per-segment selection --------------------------------------------------------
    def gather_boxes(self, bd, points=None):
        """For each box k of bd (K, 6, 4) (rows h . [p; 1] < 0 inside), the surface points inside it, in surface order,
        on the device.  Returns (pc (K, Np, 3) float64 CUDA tensor zero-padded, Np = max(1, largest count), counts (K,)
        int32 numpy).  points: another (n, 3) float64 CUDA tensor to select from instead of the surface."""
        import torch
        pts = self.surf_points_dev() if points is None else points
        bdt = torch.from_numpy(np.ascontiguousarray(bd, dtype=np.float64)).to(self.device)
        return gather_boxes_dev(bdt, pts, ctx=self.ctx)


def gather_boxes_dev(bd, points, ctx=None):
    """anet_voxel_gather_boxes_dev on CUDA tensors: bd (K, 6, 4) float64, points (n, 3) float64.  A counting pass sizes
    the output, then the write pass fills it: (pc (K, Np, 3) zero-padded with Np = max(1, largest count), counts (K,))."""
    import torch
    ctx = ctx or default_context()
    K, n = int(bd.shape[0]), int(points.shape[0])
    if tuple(bd.shape[1:]) != (6, 4) or tuple(points.shape[1:]) != (3,):
        raise ValueError("gather_boxes: bd (K, 6, 4), points (n, 3)")
    dev = bd.device
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws = int(ctx.lib.anet_voxel_gather_workspace(K, n))
    if ws < 0:
        raise ValueError("gather_boxes: at most 65535 boxes and 2^31 - 1 points")
    work = torch.empty(max(ws, 4), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(max(K, 1), dtype=torch.int32, device=dev)
    bd = bd.contiguous(); points = points.contiguous()
    pp = _vp(points) if n else None
    ctx.check(ctx.lib.anet_voxel_gather_boxes_dev(ctx.handle, K, _vp(bd), pp, n, 0, _vp(work), None, _vp(cnt), st))
    counts = cnt[:K].cpu().numpy()
    Np = max(1, int(counts.max()) if K else 1)
    pc = torch.zeros((K, Np, 3), dtype=torch.float64, device=dev)
    if K and counts.max() > 0:
        ctx.check(ctx.lib.anet_voxel_gather_boxes_dev(ctx.handle, K, _vp(bd), pp, n, Np, _vp(work), _vp(pc), _vp(cnt), st))
    return pc, counts


def _grid_of(vm_or_grid):
    """(VoxelGrid, context or None) of a VoxelMap or a VoxelGrid."""
    if isinstance(vm_or_grid, VoxelMap):
        return vm_or_grid._grid, vm_or_grid.ctx
    if not isinstance(vm_or_grid, VoxelGrid):
        raise TypeError("a VoxelMap or a VoxelGrid expected")
    return vm_or_grid, None


def distance_transform_dev(vm_or_grid, voxels, walls=True, out=None, stream=None, ctx=None):
    """anet_voxel_distance_dev on tensors: voxels uint8 CUDA (n_voxels,), -> the int32 field (n_voxels,) (`out` when given).
    Asynchronous on the current stream."""
    import torch
    grid, own = _grid_of(vm_or_grid)
    ctx = ctx or own or default_context(voxels.device.index or 0)
    n = int(grid.size[0]) * int(grid.size[1]) * int(grid.size[2])
    if voxels.dtype != torch.uint8 or voxels.numel() != n or not voxels.is_contiguous() or not voxels.is_cuda:
        raise ValueError("distance_transform_dev: voxels must be a contiguous uint8 CUDA tensor with one byte per voxel")
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=voxels.device)
    elif out.dtype != torch.int32 or out.numel() != n or not out.is_contiguous() or out.device != voxels.device:
        raise ValueError("distance_transform_dev: out must be a contiguous int32 tensor with one value per voxel, on the device of voxels")
    st = ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(voxels.device).cuda_stream)
    ctx.check(ctx.lib.anet_voxel_distance_dev(ctx.handle, ctypes.byref(grid), _vp(voxels), 1 if walls else 0, _vp(out), st))
    return out


def distance_query_dev(vm_or_grid, sd2, pos, grad=True, stream=None, ctx=None):
    """anet_voxel_distance_query_dev on tensors: sd2 the int32 field, pos (n, 3) float64 CUDA -> (dist (n,), grad (n, 3) or None)."""
    import torch
    grid, own = _grid_of(vm_or_grid)
    ctx = ctx or own or default_context(sd2.device.index or 0)
    if sd2.dtype != torch.int32 or sd2.numel() != int(grid.size[0]) * int(grid.size[1]) * int(grid.size[2]) or \
            not sd2.is_contiguous():
        raise ValueError("distance_query_dev: sd2 must be the contiguous int32 field of this grid")
    if pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError("distance_query_dev: pos must be (n, 3) float64")
    if not (sd2.is_cuda and pos.is_cuda) or sd2.device != pos.device:
        raise ValueError("distance_query_dev: sd2 and pos must be CUDA tensors on one device")
    pos = pos.contiguous()
    n = pos.shape[0]
    dist = torch.empty(n, dtype=torch.float64, device=pos.device)
    g = torch.empty((n, 3), dtype=torch.float64, device=pos.device) if grad else None
    st = ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(pos.device).cuda_stream)
    ctx.check(ctx.lib.anet_voxel_distance_query_dev(ctx.handle, ctypes.byref(grid), _vp(sd2), _vp(pos) if n else None, n,
                                                    _vp(dist) if n else None, _vp(g) if (grad and n) else None, st))
    return dist, g


def voxel_raycast_dev(vm_or_grid, voxels, origins, ends, stream=None, ctx=None):
    """anet_voxel_raycast_dev on tensors: voxels uint8 CUDA (n_voxels,), origins / ends (n, 3) float64 CUDA -> (voxel int32 (n,),
    t float64 (n,)).  Asynchronous on the current stream."""
    import torch
    grid, own = _grid_of(vm_or_grid)
    ctx = ctx or own or default_context(voxels.device.index or 0)
    nv = int(grid.size[0]) * int(grid.size[1]) * int(grid.size[2])
    if voxels.dtype != torch.uint8 or voxels.numel() != nv or not voxels.is_contiguous() or not voxels.is_cuda:
        raise ValueError("voxel_raycast_dev: voxels must be a contiguous uint8 CUDA tensor with one byte per voxel")
    for a in (origins, ends):
        if a.dtype != torch.float64 or a.dim() != 2 or a.shape[1] != 3 or a.device != voxels.device:
            raise ValueError("voxel_raycast_dev: origins and ends must be (n, 3) float64 tensors on the device of voxels")
    if origins.shape[0] != ends.shape[0]:
        raise ValueError("voxel_raycast_dev: as many origins as ends")
    origins = origins.contiguous(); ends = ends.contiguous()
    n = origins.shape[0]
    voxel = torch.empty(n, dtype=torch.int32, device=voxels.device)
    t = torch.empty(n, dtype=torch.float64, device=voxels.device)
    st = ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(voxels.device).cuda_stream)
    ctx.check(ctx.lib.anet_voxel_raycast_dev(ctx.handle, ctypes.byref(grid), _vp(voxels), _vp(origins) if n else None,
                                             _vp(ends) if n else None, n, _vp(voxel) if n else None, _vp(t) if n else None, st))
    return voxel, t
