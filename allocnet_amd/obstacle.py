"""The static map as a penalty of the MINCO objective: what traj_first_collision and getClearance find, this term removes.  A batch
of trajectories is kept `clearance` away from the blocked voxels of a VoxelMap through its exact distance field
(VoxelMap.distance_field), with gradients for the coefficients and the durations -- no corridor, no homotopy class fixed in advance.

All arithmetic runs in the HIP kernel of csrc/distance_kernels.h behind anet_minco_obstacle_partial_grads_dev; the semantics are
stated in include/allocnet_amd.h.  `field` is a pair (VoxelMap or VoxelGrid, sd2 int32 CUDA tensor), or a VoxelMap alone, whose
cached field with walls is taken.
"""
import ctypes

import numpy as np

from ._lib import ObstaclePenalty
from .avoid import _f64, _ref, _stream_of, _tptr
from .context import default_context
from .voxel_map import VoxelMap, _grid_of


def _field(field):
    """-> (VoxelGrid, sd2)"""
    import torch
    if isinstance(field, VoxelMap):
        return field._grid, field.distance_field(walls=True)
    vm, sd2 = field
    grid, _ = _grid_of(vm)
    if sd2.dtype != torch.int32 or sd2.numel() != int(grid.size[0]) * int(grid.size[1]) * int(grid.size[2]) or \
            not (sd2.is_contiguous() and sd2.is_cuda):
        raise ValueError("the field must be the contiguous int32 CUDA distance field of its grid")
    return grid, sd2


def make_obstacle_penalty(w=100.0, smooth_mu=0.05, clearance=0.5, res=20):
    """struct anet_obstacle_penalty: weight, smoothedL1 mu (m), the distance to keep from blocked voxel centres (m) and the samples
    per piece."""
    return ObstaclePenalty(float(w), float(smooth_mu), float(clearance), int(res))


def minco_obstacle_partial_grads_dev(obstacle_penalty, s, N, B, coeffs, T, field, gdC, gdT, piece_cost=None, accumulate=False,
                                     stream=None, ctx=None):
    """anet_minco_obstacle_partial_grads_dev on batch-minor torch CUDA float64 tensors with the row stride of T."""
    ctx = ctx or default_context(T.device.index or 0)
    grid, sd2 = _field(field)
    ctx.check(ctx.lib.anet_minco_obstacle_partial_grads_dev(
        ctx.handle, _ref(obstacle_penalty), int(s), int(N), int(B), T.stride(0), _tptr(coeffs), _tptr(T), ctypes.byref(grid),
        _tptr(sd2), 1 if accumulate else 0, _tptr(gdC), _tptr(gdT), _tptr(piece_cost), _stream_of(T, stream)))
    return gdC, gdT, piece_cost


def minco_obstacle_cost_grad_dev(head, tail, wps, T, s, c, N, B, field, obstacle_penalty, hpolys=None, penalty=None, stream=None,
                                 ctx=None):
    """J = int (p^(s))^2 + rho sum T + J_pen + J_obs and its gradient, composed at the C ABI as minco_avoid_cost_grad_dev is:
    anet_minco_solve_dev -> anet_minco_partial_grads_dev -> anet_minco_obstacle_partial_grads_dev(accumulate = 1) ->
    anet_minco_propagate_grad_dev.  Batch-minor torch CUDA float64 tensors with a common row stride.
    Returns cost (ld,), gradP (max(3 (N-1), 1), ld), gradT (N, ld), coeffs (N*3*2s, ld)."""
    import torch
    from .minco import minco_solve_dev
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    st = _stream_of(T, stream)
    field = _field(field)
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
    zeros = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float64)
    coeffs, energy = new(N * 3 * 2 * s, ld), new(ld)
    minco_solve_dev(head, tail, wps, T, s, c, N, B, coeffs=coeffs, energy=energy, stream=st.value, ctx=ctx)
    gdC, gdT, pc = new(N * 3 * 2 * s, ld), new(N, ld), zeros(N, ld)
    ctx.check(ctx.lib.anet_minco_partial_grads_dev(ctx.handle, s, N, B, ld, _tptr(coeffs), _tptr(T), _tptr(hpolys),
                                                   _ref(penalty) if penalty is not None else None, 1, _tptr(gdC), _tptr(gdT),
                                                   _tptr(pc), st))
    minco_obstacle_partial_grads_dev(obstacle_penalty, s, N, B, coeffs, T, field, gdC, gdT, pc, accumulate=True, stream=st.value,
                                     ctx=ctx)
    gradP, gradT = zeros(max(3 * (N - 1), 1), ld), new(N, ld)
    ctx.check(ctx.lib.anet_minco_propagate_grad_dev(ctx.handle, s, c, N, B, ld, _tptr(T), _tptr(coeffs), _tptr(gdC), _tptr(gdT),
                                                    _tptr(gradP), _tptr(gradT), st))
    # the adjoint kernel is given no cost to assemble here: the sum of the terms and rho's share of the time gradient
    rho = penalty.rho if penalty is not None else 0.0
    cost = energy + rho * T.sum(0) + pc.sum(0)
    if rho != 0.0:
        gradT = gradT + rho
    return cost, gradP, gradT, coeffs


def minco_obstacle_cost_grad(head, tail, wps, T, s, field, obstacle_penalty, hpolys=None, penalty=None, ctx=None):
    """Host (numpy, trajectory-major) form of minco_obstacle_cost_grad_dev, with minco_avoid_cost_grad's shapes: head, tail
    (B, 3, c); wps (B, N-1, 3); T (B, N); hpolys (B, N, M, 4).  Returns cost (B,), gradP (B, N-1, 3), gradT (B, N)."""
    import torch
    head = _f64(head)
    B, _, c = head.shape
    tail = _f64(tail, (B, 3, c))
    T = _f64(T)
    N = T.shape[1]
    wps = _f64(wps if wps is not None else np.zeros((B, 0, 3)), (B, N - 1, 3))
    ctx = ctx or default_context()
    dev = torch.device("cuda", ctx.device)
    ld = int(ctx.lib.anet_recommended_ld(B)) if B > 1 else 1

    def up(a):     # (B, fields) -> batch-minor (fields, ld)
        t = torch.zeros(max(a.shape[1], 1), ld, device=dev, dtype=torch.float64)
        if a.shape[1]:
            t[:a.shape[1], :B] = torch.from_numpy(a).to(dev).T
        return t
    d_T = up(T)
    d_T[:, B:] = 1.0
    d_hp = None
    if hpolys is not None:
        hpolys = _f64(hpolys)
        if penalty is None or hpolys.shape != (B, N, penalty.poly_rows, 4):
            raise ValueError("hpolys must be (B, N, penalty.poly_rows, 4)")
        d_hp = up(hpolys.reshape(B, -1))
    cost, gP, gT, _ = minco_obstacle_cost_grad_dev(up(head.reshape(B, -1)), up(tail.reshape(B, -1)), up(wps.reshape(B, -1)), d_T, s,
                                                   c, N, B, field, obstacle_penalty, hpolys=d_hp, penalty=penalty, ctx=ctx)
    gradP = gP[:3 * (N - 1), :B].T.contiguous().cpu().numpy().reshape(B, N - 1, 3)
    return cost[:B].cpu().numpy(), gradP, gT[:, :B].T.contiguous().cpu().numpy()


def obstacle_objective_dev(head, tail, s, c, N, B, field, obstacle_penalty, hpolys=None, penalty=None, ctx=None):
    """The composed objective as an `evaluate(x, f, g)` of lbfgs_optimize_dev, as avoid_objective_dev: x (3 (N-1) + N, ld) holds the
    waypoints (the rows of minco_cost_grad_dev's wps) and below them the LOG durations, so that every duration stays positive;
    g is the gradient w.r.t. x (dJ/dlog T = T dJ/dT).  The field is taken once, here: the map is a constant of the run."""
    import torch
    nw = 3 * (N - 1)
    field = _field(field)

    def evaluate(x, f, g):
        T = torch.exp(x[nw:nw + N])
        wps = x[:nw] if nw else torch.zeros(1, x.shape[1], device=x.device, dtype=torch.float64)
        cost, gP, gT, _ = minco_obstacle_cost_grad_dev(head, tail, wps, T, s, c, N, B, field, obstacle_penalty, hpolys=hpolys,
                                                       penalty=penalty, ctx=ctx)
        f.copy_(cost)
        if nw:
            g[:nw].copy_(gP[:nw])
        g[nw:nw + N].copy_(gT * T)
    return evaluate
