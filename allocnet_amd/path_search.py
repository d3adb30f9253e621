"""sfc_gen::planPath on the device voxel map: the front-end route of LearningPlanner::plan (learning_planner.hpp) from a
start and a goal, as a collision-free polyline and its length.  The search is a resolution-complete shortest-path field on
the grid (26 neighbours, weights 10 / 14 / 17, no corner cutting), a walk back along it and a greedy line-of-sight
shortcut, all HIP kernels (allocnet_amd/csrc/path_kernels.h); the semantics are in include/allocnet_amd.h.  Unlike OMPL's
InformedRRT*, it is exact and deterministic: `timeout` is accepted for the signature and bounds nothing."""
import ctypes

import numpy as np

from ._lib import ANET_ERR_INVALID, AnetError

PATH_EXACT = 0
PATH_APPROXIMATE = 1
PATH_INVALID_START = 2

_CAP = 1024   # path points per problem on the first extraction; a longer path is extracted again with its true count


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _box(vm, lb, hb):
    lo = vm.getOrigin() if lb is None else np.asarray(lb, dtype=np.float64).reshape(3)
    hi = vm.getCorner() if hb is None else np.asarray(hb, dtype=np.float64).reshape(3)
    return (ctypes.c_double * 6)(*[float(v) for v in np.concatenate([lo, hi])])


def _points(x, name):
    p = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    if not len(p):
        raise ValueError(f"{name}: at least one (3,) point")
    return p


def _workspace(vm, B):
    """the map's path workspace for B problems (kept on the map, grown on demand)"""
    import torch
    need = int(vm.ctx.lib.anet_voxel_path_workspace(ctypes.byref(vm._grid), int(B)))
    if need < 0:
        raise AnetError(ANET_ERR_INVALID, "path search: 1 <= B <= 65535 and 17 * voxels below 2^32 - 1")
    ws = getattr(vm, "_path_work", None)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=vm.device)
        vm._path_work = ws
    return ws


def path_field_dev(vm, starts, lb=None, hb=None):
    """The cost-to-come fields of B starts on the map: ((B, n_voxels) uint32 CUDA tensor, a view of the map's workspace
    valid until its next search; rounds).  UINT32_MAX marks unreached and non-free voxels."""
    import torch
    s = _points(starts, "path_field_dev")
    B = len(s)
    ws = _workspace(vm, B)
    st = vm._stream()
    sd = torch.from_numpy(s).to(vm.device)
    rounds = ctypes.c_int32(0)
    vm.ctx.check(vm.ctx.lib.anet_voxel_path_field_dev(vm.ctx.handle, ctypes.byref(vm._grid), _vp(vm.voxels_dev), _box(vm, lb, hb),
                                                      _vp(sd), B, _vp(ws), ctypes.byref(rounds), st))
    n = int(np.prod(vm._size))
    return ws[:4 * B * n].view(torch.uint32).reshape(B, n), int(rounds.value)


def extract_paths(vm, starts, goals, lb=None, hb=None):
    """Target, walk, shortcut and cost on the fields of the map's last path_field_dev (same starts and box):
    (costs (B,), paths [(m_b, 3)], status (B,))."""
    import torch
    s, g = _points(starts, "extract_paths"), _points(goals, "extract_paths")
    if s.shape != g.shape:
        raise ValueError("extract_paths: as many goals as starts")
    B = len(s)
    ws = _workspace(vm, B)
    dev, st, lib, h = vm.device, vm._stream(), vm.ctx.lib, vm.ctx.handle
    sd, gd = torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev)
    npts = torch.zeros(B, dtype=torch.int32, device=dev)
    cost = torch.zeros(B, dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    box = _box(vm, lb, hb)
    cap = _CAP
    while True:
        out = torch.empty((B, cap, 3), dtype=torch.float64, device=dev)
        vm.ctx.check(lib.anet_voxel_path_extract_dev(h, ctypes.byref(vm._grid), _vp(vm.voxels_dev), box, _vp(sd), _vp(gd), B,
                                                     _vp(ws), cap, _vp(out), _vp(npts), _vp(cost), _vp(status), st))
        n = npts.cpu().numpy()
        if n.max() <= cap:
            break
        cap = int(n.max())
    stt = status.cpu().numpy()
    if (stt < 0).any():
        raise AnetError(ANET_ERR_INVALID, "extract_paths: the walk found no predecessor (fields and starts disagree)")
    o = out.cpu().numpy()
    return cost.cpu().numpy(), [o[b, :n[b]].copy() for b in range(B)], stt


def plan_paths(starts, goals, vm, lb=None, hb=None, with_rounds=False):
    """B searches in one call: (costs (B,) float64, paths [(m_b, 3) float64], status (B,) int32 PATH_*).
    INVALID_START gives cost inf and a (0, 3) path.  with_rounds: also return the field's round count."""
    s, g = _points(starts, "plan_paths"), _points(goals, "plan_paths")
    if s.shape != g.shape:
        raise ValueError("plan_paths: as many goals as starts")
    _, rounds = path_field_dev(vm, s, lb, hb)
    res = extract_paths(vm, s, g, lb, hb)
    return res + (rounds,) if with_rounds else res


def plan_path(s, g, lb, hb, vm, timeout=0.01):
    """sfc_gen::planPath(s, g, lb, hb, mapPtr, timeout, p): (cost, path (m, 3) float64).  A start that is not free gives
    (inf, (0, 3)).  lb / hb None: the map's [getOrigin(), getCorner()].  timeout bounds nothing (the search is exact)."""
    del timeout
    costs, paths, _ = plan_paths(np.reshape(s, (1, 3)), np.reshape(g, (1, 3)), vm, lb, hb)
    return float(costs[0]), paths[0]
