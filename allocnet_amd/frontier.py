"""Where to go next on a map with unknown space (allocnet_amd/csrc/frontier_kernels.h; the rules are in include/allocnet_amd.h):

    occupancy_frontier_dev   the known-free voxels with an unknown face neighbour inside the map
    label_components_dev     connected components of any byte grid: label = the least voxel index of the component
    component_stats_dev      count, integer coordinate sums and cell box per component, in ascending label order
    view_gain_dev            per candidate pose, the number of distinct unknown voxels a scan from there would cross
    frustum_points           the template of a pinhole camera for view_gain_dev
    frontier_clusters / candidate_views / next_view   the three put together: clusters, poses around them, a ranking

All results are integers decided by integer or individually rounded arithmetic: functions of the inputs, bit for bit."""
import ctypes
import math

import numpy as np

from ._lib import VoxelGrid
from .context import default_context
from .occupancy import depth_to_points_dev
from .voxel_map import VoxelMap, _grid_of


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _n_voxels(grid):
    return int(grid.size[0]) * int(grid.size[1]) * int(grid.size[2])


def _grid_ctx(m, ctx, dev):
    """(VoxelGrid, context) of a VoxelMap, an OccupancyMap or a VoxelGrid."""
    if isinstance(m, VoxelGrid):
        return m, ctx or default_context((dev.index or 0) if dev is not None else 0)
    if isinstance(m, VoxelMap):
        grid, own = _grid_of(m)
        return grid, ctx or own
    return m._grid, ctx or m.ctx


def occupancy_frontier_dev(grid, logodds, occ=0, box=None, out=None, with_count=True, ctx=None):
    """anet_occupancy_frontier_dev on tensors: logodds int16 CUDA (n_voxels,), box None or (lo (3,), ext (3,)) in cells ->
    (mask uint8 CUDA (n_voxels,), count int or None).  `out`: a mask tensor to write into."""
    import torch
    grid, ctx = _grid_ctx(grid, ctx, logodds.device)
    n = _n_voxels(grid)
    if logodds.dtype != torch.int16 or logodds.numel() != n or not logodds.is_contiguous() or not logodds.is_cuda:
        raise ValueError("occupancy_frontier_dev: logodds must be a contiguous int16 CUDA tensor with one value per voxel")
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=logodds.device)
    elif out.dtype != torch.uint8 or out.numel() != n or not out.is_contiguous() or out.device != logodds.device:
        raise ValueError("occupancy_frontier_dev: out must be a contiguous uint8 tensor with one byte per voxel, on the device of logodds")
    lo = ext = None
    if box is not None:
        lo = np.ascontiguousarray(np.asarray(box[0]).reshape(3), dtype=np.int32)
        ext = np.ascontiguousarray(np.asarray(box[1]).reshape(3), dtype=np.int32)
    cnt = torch.zeros(1, dtype=torch.int64, device=logodds.device) if with_count else None
    ctx.check(ctx.lib.anet_occupancy_frontier_dev(ctx.handle, ctypes.byref(grid), _vp(logodds), int(occ),
                                                  lo.ctypes.data_as(ctypes.c_void_p) if lo is not None else None,
                                                  ext.ctypes.data_as(ctypes.c_void_p) if ext is not None else None,
                                                  _vp(out), _vp(cnt) if with_count else None, _stream(logodds.device)))
    return out, (int(cnt.item()) if with_count else None)


def _components_work(grid, ctx, dev):
    import torch
    ws = int(ctx.lib.anet_voxel_components_workspace(ctypes.byref(grid)))
    if ws < 0:
        raise ValueError("components: sizes >= 1, fewer than 2^31 voxels, finite origin, scale > 0")
    return torch.empty(ws // 8, dtype=torch.int64, device=dev)


def label_components_dev(grid, mask, connectivity=26, out=None, work=None, with_rounds=False, ctx=None):
    """anet_voxel_label_components_dev on tensors: mask uint8 CUDA (n_voxels,) -> labels int32 CUDA (n_voxels,): -1 off the mask,
    else the least voxel index of the component.  with_rounds: (labels, rounds)."""
    import torch
    grid, ctx = _grid_ctx(grid, ctx, mask.device)
    n = _n_voxels(grid)
    if mask.dtype not in (torch.uint8, torch.bool) or mask.numel() != n or not mask.is_contiguous() or not mask.is_cuda:
        raise ValueError("label_components_dev: mask must be a contiguous uint8 CUDA tensor with one byte per voxel")
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=mask.device)
    elif out.dtype != torch.int32 or out.numel() != n or not out.is_contiguous() or out.device != mask.device:
        raise ValueError("label_components_dev: out must be a contiguous int32 tensor with one value per voxel, on the device of mask")
    work = work if work is not None else _components_work(grid, ctx, mask.device)
    rounds = ctypes.c_int32(0)
    ctx.check(ctx.lib.anet_voxel_label_components_dev(ctx.handle, ctypes.byref(grid), _vp(mask), int(connectivity), _vp(out), _vp(work),
                                                      ctypes.byref(rounds), _stream(mask.device)))
    return (out, int(rounds.value)) if with_rounds else out


def component_stats_dev(grid, labels, max_components=4096, work=None, ctx=None):
    """anet_voxel_component_stats_dev on tensors -> (n_components int, root (m,) int32, count (m,) int32, sum_xyz (m, 3) int64,
    bbox (m, 6) int32) as CUDA tensors, m = min(n_components, max_components), in ascending root order."""
    import torch
    grid, ctx = _grid_ctx(grid, ctx, labels.device)
    n = _n_voxels(grid)
    if labels.dtype != torch.int32 or labels.numel() != n or not labels.is_contiguous() or not labels.is_cuda:
        raise ValueError("component_stats_dev: labels must be a contiguous int32 CUDA tensor with one value per voxel")
    dev, m = labels.device, int(max_components)
    work = work if work is not None else _components_work(grid, ctx, dev)
    nc = torch.zeros(1, dtype=torch.int32, device=dev)
    root = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    count = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    sums = torch.empty((max(m, 1), 3), dtype=torch.int64, device=dev)
    bbox = torch.empty((max(m, 1), 6), dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.anet_voxel_component_stats_dev(ctx.handle, ctypes.byref(grid), _vp(labels), m, _vp(nc), _vp(root), _vp(count),
                                                     _vp(sums), _vp(bbox), _vp(work), _stream(dev)))
    k = int(nc.item())
    m = min(k, m)
    return k, root[:m], count[:m], sums[:m], bbox[:m]


DEFAULT_VIEW_CHUNK = 32   # views per chunk of view_gain_dev's own workspace: a slot is megabytes on a large map at a long range


def view_gain_workspace(grid, params, n_views=None, ctx=None):
    """Bytes of workspace for n_views in one chunk (None: the least, one view)."""
    grid, ctx = _grid_ctx(grid, ctx, None)
    if n_views is None:
        ws = int(ctx.lib.anet_occupancy_view_gain_workspace_min(ctypes.byref(grid), ctypes.byref(params)))
    else:
        ws = int(ctx.lib.anet_occupancy_view_gain_workspace(ctypes.byref(grid), ctypes.byref(params), int(n_views)))
    if ws < 0:
        raise ValueError("view_gain_workspace: bad grid or params")
    return ws


def view_gain_dev(grid, params, logodds, view_R, view_t, pts, occ=0, work=None, ctx=None):
    """anet_occupancy_view_gain_dev on tensors: view_R (V, 3, 3), view_t (V, 3), pts (R, 3) float64 CUDA -> gain (V,) int32 CUDA.
    work: a ZEROED uint8 CUDA tensor of at least view_gain_workspace(grid, params) bytes (it is all zero again afterwards); None:
    one for chunks of up to DEFAULT_VIEW_CHUNK views, kept on the context and reused by later calls (the marks are zero again after
    every call, so it is zeroed once)."""
    import torch
    grid, ctx = _grid_ctx(grid, ctx, logodds.device)
    dev = logodds.device
    if logodds.dtype != torch.int16 or logodds.numel() != _n_voxels(grid) or not logodds.is_contiguous() or not logodds.is_cuda:
        raise ValueError("view_gain_dev: logodds must be a contiguous int16 CUDA tensor with one value per voxel")
    view_R = view_R.reshape(-1, 9); view_t = view_t.reshape(-1, 3); pts = pts.reshape(-1, 3)
    for a in (view_R, view_t, pts):
        if a.dtype != torch.float64 or a.device != dev:
            raise ValueError("view_gain_dev: view_R, view_t and pts must be float64 tensors on the device of logodds")
    V, n_pts = int(view_t.shape[0]), int(pts.shape[0])
    if view_R.shape[0] != V:
        raise ValueError("view_gain_dev: as many rotations as translations")
    view_R = view_R.contiguous(); view_t = view_t.contiguous(); pts = pts.contiguous()
    gain = torch.empty(V, dtype=torch.int32, device=dev)
    if V == 0:
        return gain
    if work is None:
        want = view_gain_workspace(grid, params, min(V, DEFAULT_VIEW_CHUNK), ctx=ctx)
        work = getattr(ctx, "_view_gain_work", None)
        if work is None or work.device != dev or work.numel() < want:
            work = ctx._view_gain_work = torch.zeros(want, dtype=torch.uint8, device=dev)
    ctx.check(ctx.lib.anet_occupancy_view_gain_dev(ctx.handle, ctypes.byref(grid), ctypes.byref(params), _vp(logodds), int(occ),
                                                   _vp(view_R), _vp(view_t), V, _vp(pts) if n_pts else None, n_pts, _vp(gain),
                                                   _vp(work), int(work.numel() * work.element_size()), _stream(dev)))
    return gain


def frustum_points(K, width, height, step, depth, device=None, ctx=None):
    """The template of a pinhole camera: the unprojection (depth_to_points_dev) of a constant-depth image with the identity pose,
    (n, 3) float64 CUDA in the camera frame (z forward), n = ceil(width / step) * ceil(height / step)."""
    import torch
    ctx = ctx or default_context()
    dev = device or torch.device("cuda", ctx.device)
    img = torch.full((int(height), int(width)), float(depth), dtype=torch.float32, device=dev)
    return depth_to_points_dev(img, K, (np.eye(3), np.zeros(3)), step=step, ctx=ctx)


# ---- clusters, candidate poses, ranking -----------------------------------------------------------------------------------------
def clusters_table(n, root, count, sums, bbox, origin, scale, min_size):
    """The host table of components_stats_dev's rows with count >= min_size: a dict of arrays -- root, count, centroid (m, 3)
    world = origin + (sum / count + 0.5) * scale, bbox_lo / bbox_hi (m, 3) world corners of the cell box, cells_lo / cells_hi."""
    root, count, sums, bbox = (np.asarray(a) for a in (root, count, sums, bbox))
    keep = count >= int(min_size)
    root, count, sums, bbox = root[keep], count[keep], sums[keep].reshape(-1, 3), bbox[keep].reshape(-1, 6)
    origin = np.asarray(origin, dtype=np.float64)
    cen = origin + (sums.astype(np.float64) / np.maximum(count, 1)[:, None] + 0.5) * scale
    return dict(n_components=int(n), root=root, count=count, centroid=cen, cells_lo=bbox[:, :3], cells_hi=bbox[:, 3:],
                bbox_lo=origin + bbox[:, :3] * scale, bbox_hi=origin + (bbox[:, 3:] + 1) * scale)


def frontier_clusters(occ_map, occ=0, min_size=8, connectivity=26, box=None, max_components=65536):
    """The frontier of an OccupancyMap grouped into clusters: clusters_table of its components with at least min_size voxels
    (filtered on the host), plus "mask" and "labels", the device tensors they were made from."""
    L = occ_map.logodds_dev()
    mask, _ = occupancy_frontier_dev(occ_map, L, occ, box, with_count=False)
    work = _components_work(occ_map._grid, occ_map.ctx, L.device)
    labels = label_components_dev(occ_map, mask, connectivity, work=work)
    n, root, count, sums, bbox = component_stats_dev(occ_map, labels, max_components, work=work)
    tab = clusters_table(n, root.cpu().numpy(), count.cpu().numpy(), sums.cpu().numpy(), bbox.cpu().numpy(), occ_map.getOrigin(),
                         occ_map.getScale(), min_size)
    tab["mask"], tab["labels"] = mask, labels
    return tab


def _cells(vm, pos):
    """(cells (n, 3) int64, inside (n,), linear ids) by floor((p - origin) / scale), the occupancy grid's rule."""
    size = np.asarray(vm.getSize(), dtype=np.int64)
    c = np.floor((np.asarray(pos, dtype=np.float64).reshape(-1, 3) - vm.getOrigin()) / vm.getScale()).astype(np.int64)
    inside = ((c >= 0) & (c < size)).all(axis=1)
    ids = c[:, 0] + size[0] * (c[:, 1] + size[1] * c[:, 2])
    return c, inside, np.where(inside, ids, 0)


def look_at(eye, target):
    """Camera-to-world rotations (n, 3, 3) of pinhole cameras at `eye` looking at `target` (z forward, x right, y down; world z up)."""
    f = np.asarray(target, dtype=np.float64).reshape(-1, 3) - np.asarray(eye, dtype=np.float64).reshape(-1, 3)
    f[np.linalg.norm(f, axis=1) < 1e-9] = [1.0, 0.0, 0.0]          # (the eye on the target: any direction)
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    up = np.array([0.0, 0.0, 1.0])
    r = np.cross(f, up)
    flat = np.linalg.norm(r, axis=1) < 1e-9
    r[flat] = [1.0, 0.0, 0.0]
    r = r / np.linalg.norm(r, axis=1, keepdims=True)
    d = np.cross(f, r)
    return np.stack([r, d, f], axis=2)


def candidate_views(clusters, vm, robot, radii=(1.0, 2.0), n_yaw=8, height=None, free_labels=None, on_frontier=True):
    """Poses on rings of `radii` around each cluster centroid, n_yaw per ring, at the centroid's height (or `height`), facing
    the centroid; on_frontier: also, per cluster, the centre of its frontier voxel nearest the centroid among those the robot can
    reach (needs clusters["labels"]), so that a cluster whose rings are all blocked still has a pose.  A pose is kept only when
    its cell is free in vm and carries the label of the robot's cell among the 6-connected components of vm's free bytes: the
    pose is reachable.  -> dict(t (m, 3), R (m, 3, 3), cluster (m,) row of the table, free_labels, robot_label); m == 0 when the
    robot's own cell is not free."""
    import torch
    if free_labels is None:
        free_labels = vm.components(6)
    cen = np.asarray(clusters["centroid"], dtype=np.float64).reshape(-1, 3)
    _, r_in, r_id = _cells(vm, robot)
    robot_label = int(free_labels[int(r_id[0])].item()) if r_in[0] else -1
    empty = dict(t=np.zeros((0, 3)), R=np.zeros((0, 3, 3)), cluster=np.zeros(0, dtype=np.int64), free_labels=free_labels,
                 robot_label=robot_label)
    if robot_label < 0 or len(cen) == 0:
        return empty
    yaw = (np.arange(int(n_yaw)) + 0.5) * (2.0 * math.pi / int(n_yaw))
    ring = np.concatenate([r * np.stack([np.cos(yaw), np.sin(yaw), np.zeros_like(yaw)], axis=1) for r in radii]).reshape(-1, 3)
    t = (cen[:, None, :] + ring[None, :, :]).reshape(-1, 3)
    which = np.repeat(np.arange(len(cen)), len(ring))
    if height is not None:
        t[:, 2] = float(height)
    if on_frontier and "labels" in clusters:
        size = np.asarray(vm.getSize(), dtype=np.int64)
        extra_t, extra_c = [], []
        for k, root in enumerate(np.asarray(clusters["root"]).tolist()):
            ids = torch.nonzero(clusters["labels"] == int(root)).reshape(-1)
            ids = ids[free_labels[ids] == robot_label].cpu().numpy()
            if len(ids) == 0:
                continue
            c = np.stack([ids % size[0], (ids // size[0]) % size[1], ids // (size[0] * size[1])], axis=1)
            p = vm.getOrigin() + (c + 0.5) * vm.getScale()
            extra_t.append(p[np.argmin(((p - cen[k]) ** 2).sum(axis=1))])
            extra_c.append(k)
        if extra_t:
            t = np.concatenate([t, np.asarray(extra_t)])
            which = np.concatenate([which, np.asarray(extra_c)])
    _, inside, ids = _cells(vm, t)
    lab = free_labels[torch.from_numpy(ids).to(free_labels.device)].cpu().numpy()
    keep = inside & (lab == robot_label)
    t, which = t[keep], which[keep]
    return dict(empty, t=t, R=look_at(t, cen[which]), cluster=which)


def next_view(occ_map, vm, robot, pts, occ=0, min_size=8, connectivity=26, radii=(1.0, 2.0), n_yaw=8, height=None, lam=0.2,
              clusters=None, work=None):
    """Rank candidate poses: gain per candidate (view_gain_dev with the template pts), route length from the robot on vm's
    path field (unit steps of scale / 10), utility gain * exp(-lam * length).  -> dict(t, R, cluster, gain, length, utility,
    order (best first), clusters); candidates the field does not reach have utility 0."""
    import torch
    clusters = clusters if clusters is not None else frontier_clusters(occ_map, occ, min_size, connectivity)
    cand = candidate_views(clusters, vm, robot, radii, n_yaw, height)
    m = len(cand["t"])
    out = dict(cand, clusters=clusters, gain=np.zeros(m, dtype=np.int32), length=np.zeros(m), utility=np.zeros(m),
               order=np.zeros(0, dtype=np.int64))
    if m == 0:
        return out
    dev = occ_map.device
    gain = view_gain_dev(occ_map, occ_map.params, occ_map.logodds_dev(), torch.from_numpy(np.ascontiguousarray(cand["R"])).to(dev),
                         torch.from_numpy(np.ascontiguousarray(cand["t"])).to(dev), pts, occ, work=work).cpu().numpy()
    field, _ = vm.path_field_dev(np.asarray(robot, dtype=np.float64).reshape(1, 3))
    _, _, ids = _cells(vm, cand["t"])
    d = field[0].view(torch.int32)[torch.from_numpy(ids).to(field.device)].cpu().numpy().view(np.uint32).astype(np.int64)
    reached = d != 0xFFFFFFFF
    length = np.where(reached, d * (vm.getScale() / 10.0), np.inf)
    util = np.where(reached & (gain > 0), gain * np.exp(-lam * np.where(reached, length, 0.0)), 0.0)
    out.update(gain=gain, length=length, utility=util, order=np.argsort(-util, kind="stable"))
    return out
