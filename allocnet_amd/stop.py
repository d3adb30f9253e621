"""Stop within known space: at every instant the vehicle must be able to come to rest inside space that is known to be free.  On a
map whose blocked set is occupied OR unknown (OccupancyMap.to_voxel_map(unknown="blocked")) the distance field measures how far
the vehicle is from everything nobody has seen, and this term holds the reaction distance plus the braking distance,
t_react |v| + v.v / (2 a_brake), grown by `clearance`, inside it -- as a penalty of the MINCO objective with gradients for the
coefficients and the durations, and as a sampled check.  The obstacle term (obstacle.py) keeps a trajectory away from the unknown;
this one also slows it down where the known region is thin.  It dominates the obstacle term of the same clearance, weight and mu
and equals it at a_brake = inf, t_react = 0: a caller uses one or the other.

All arithmetic runs in the HIP kernels of csrc/stop_kernels.h behind anet_minco_stop_partial_grads_dev and
anet_traj_stop_margin[_dev]; the semantics are stated in include/allocnet_amd.h.  `field` is a pair (VoxelMap or VoxelGrid, sd2 int32
CUDA tensor), or a VoxelMap alone, whose cached field with walls is taken.
"""
import ctypes
import math

import numpy as np

from ._lib import StopPenalty
from .avoid import _f64, _ref, _stream_of, _tptr
from .context import default_context
from .obstacle import _field
from .trajectory import _ptr, traj_eval


def make_stop_penalty(w=100.0, smooth_mu=0.05, clearance=0.0, a_brake=5.0, t_react=0.0, speed_eps=1e-2, res=20):
    """struct anet_stop_penalty: weight, smoothedL1 mu (m), the distance to keep on top of the stop distance (m), the braking
    deceleration (m/s^2; inf: none), the reaction time (s), the smoothing of |v| in the reaction term (m/s; only read when
    t_react > 0) and the samples per piece."""
    return StopPenalty(float(w), float(smooth_mu), float(clearance), float(a_brake), float(t_react), float(speed_eps), int(res))


def minco_stop_partial_grads_dev(stop_penalty, s, N, B, coeffs, T, field, gdC, gdT, piece_cost=None, accumulate=False, stream=None,
                                 ctx=None):
    """anet_minco_stop_partial_grads_dev on batch-minor torch CUDA float64 tensors with the row stride of T."""
    ctx = ctx or default_context(T.device.index or 0)
    grid, sd2 = _field(field)
    ctx.check(ctx.lib.anet_minco_stop_partial_grads_dev(
        ctx.handle, _ref(stop_penalty), int(s), int(N), int(B), T.stride(0), _tptr(coeffs), _tptr(T), ctypes.byref(grid),
        _tptr(sd2), 1 if accumulate else 0, _tptr(gdC), _tptr(gdT), _tptr(piece_cost), _stream_of(T, stream)))
    return gdC, gdT, piece_cost


def minco_stop_cost_grad_dev(head, tail, wps, T, s, c, N, B, field, stop_penalty, hpolys=None, penalty=None, stream=None, ctx=None):
    """J = int (p^(s))^2 + rho sum T + J_pen + J_stop and its gradient, composed at the C ABI as minco_obstacle_cost_grad_dev is:
    anet_minco_solve_dev -> anet_minco_partial_grads_dev -> anet_minco_stop_partial_grads_dev(accumulate = 1) ->
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
    minco_stop_partial_grads_dev(stop_penalty, s, N, B, coeffs, T, field, gdC, gdT, pc, accumulate=True, stream=st.value, ctx=ctx)
    gradP, gradT = zeros(max(3 * (N - 1), 1), ld), new(N, ld)
    ctx.check(ctx.lib.anet_minco_propagate_grad_dev(ctx.handle, s, c, N, B, ld, _tptr(T), _tptr(coeffs), _tptr(gdC), _tptr(gdT),
                                                    _tptr(gradP), _tptr(gradT), st))
    # the adjoint kernel is given no cost to assemble here: the sum of the terms and rho's share of the time gradient
    rho = penalty.rho if penalty is not None else 0.0
    cost = energy + rho * T.sum(0) + pc.sum(0)
    if rho != 0.0:
        gradT = gradT + rho
    return cost, gradP, gradT, coeffs


def minco_stop_cost_grad(head, tail, wps, T, s, field, stop_penalty, hpolys=None, penalty=None, ctx=None):
    """Host (numpy, trajectory-major) form of minco_stop_cost_grad_dev, with minco_obstacle_cost_grad's shapes: head, tail
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
    cost, gP, gT, _ = minco_stop_cost_grad_dev(up(head.reshape(B, -1)), up(tail.reshape(B, -1)), up(wps.reshape(B, -1)), d_T, s, c, N,
                                               B, field, stop_penalty, hpolys=d_hp, penalty=penalty, ctx=ctx)
    gradP = gP[:3 * (N - 1), :B].T.contiguous().cpu().numpy().reshape(B, N - 1, 3)
    return cost[:B].cpu().numpy(), gradP, gT[:, :B].T.contiguous().cpu().numpy()


def stop_objective_dev(head, tail, s, c, N, B, field, stop_penalty, hpolys=None, penalty=None, ctx=None):
    """The composed objective as an `evaluate(x, f, g)` of lbfgs_optimize_dev, as obstacle_objective_dev: x (3 (N-1) + N, ld) holds
    the waypoints (the rows of minco_cost_grad_dev's wps) and below them the LOG durations, so that every duration stays positive;
    g is the gradient w.r.t. x (dJ/dlog T = T dJ/dT).  The field is taken once, here: the map is a constant of the run."""
    import torch
    nw = 3 * (N - 1)
    field = _field(field)

    def evaluate(x, f, g):
        T = torch.exp(x[nw:nw + N])
        wps = x[:nw] if nw else torch.zeros(1, x.shape[1], device=x.device, dtype=torch.float64)
        cost, gP, gT, _ = minco_stop_cost_grad_dev(head, tail, wps, T, s, c, N, B, field, stop_penalty, hpolys=hpolys,
                                                   penalty=penalty, ctx=ctx)
        f.copy_(cost)
        if nw:
            g[:nw].copy_(gP[:nw])
        g[nw:nw + N].copy_(gT * T)
    return evaluate


# ---------------------------------------------------------------------------------------------
# the sampled check
# ---------------------------------------------------------------------------------------------
def traj_stop_margin_dev(stop_penalty, s, N, B, coeffs, T, field, margin=None, t=None, speed=None, dist=None, stream=None, ctx=None):
    """anet_traj_stop_margin_dev on batch-minor torch CUDA float64 tensors with the row stride of T: coeffs (N*3*2s, ld), T (N, ld)
    -> margin, t, speed, dist (N, ld): per piece the least d - clearance - t_react |v| - v.v / (2 a_brake) over res + 1 samples, and
    the local time, |v| and d where it is attained."""
    import torch
    ctx = ctx or default_context(T.device.index or 0)
    grid, sd2 = _field(field)
    ld, dev = T.stride(0), T.device
    new = lambda given: given if given is not None else torch.empty(N, ld, device=dev, dtype=torch.float64)
    margin, t, speed, dist = new(margin), new(t), new(speed), new(dist)
    ctx.check(ctx.lib.anet_traj_stop_margin_dev(ctx.handle, _ref(stop_penalty), int(s), int(N), int(B), ld, _tptr(coeffs), _tptr(T),
                                                ctypes.byref(grid), _tptr(sd2), _tptr(margin), _tptr(t), _tptr(speed), _tptr(dist),
                                                _stream_of(T, stream)))
    return margin, t, speed, dist


def traj_stop_margin(coeffs, T, field, a_brake, t_react=0.0, clearance=0.0, res=20, ctx=None):
    """The sampled stop margin per piece (anet_traj_stop_margin): coeffs (B, N, 3, D), T (B, N) numpy -> margin, t, speed, dist
    (B, N).  margin >= 0: at each of the res + 1 samples of the piece a ball of radius t_react |v| + v.v / (2 a_brake) + clearance
    around the vehicle lies in free space, by the field's interpolant.  A SAMPLED check: nothing bounds the value between samples.
    NaN: a non-finite coefficient or duration of that piece, or a duration <= 0."""
    ctx = ctx or default_context()
    coeffs = _f64(coeffs); T = _f64(T)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N):
        raise ValueError("shape mismatch")
    grid, sd2 = _field(field)
    pen = make_stop_penalty(0.0, 1.0, clearance, a_brake, t_react, 0.0, res)
    out = [np.empty((B, N)) for _ in range(4)]
    ctx.check(ctx.lib.anet_traj_stop_margin(ctx.handle, _ref(pen), D // 2, N, B, _ptr(coeffs), _ptr(T), ctypes.byref(grid),
                                            _tptr(sd2), *[_ptr(o) for o in out]))
    return tuple(out)


def traj_stop_check(coeffs, T, vm, a_brake, t_react=0.0, res=20, ctx=None):
    """The directional form of the check, composed of existing kernels (anet_traj_eval, anet_voxel_raycast_dev,
    anet_voxel_query_dev): at the samples of traj_stop_margin (sigma = j / res of every piece, j = 0..res) the straight stop segment
    from p along v / |v| of length t_react |v| + v.v / (2 a_brake) is walked through the voxels of the VoxelMap vm.  A sample is
    unsafe when the walk meets a voxel != 0 or when vm.query of the segment's end is blocked -- the walk passes through the outside
    of the map, query does not.  A sample at rest (|v| = 0) tests its own voxel.  coeffs (B, N, 3, D), T (B, N) numpy ->
    (count (B,) int64 of unsafe samples, first (B,) int64: the flat index i * (res + 1) + j of the first one, -1 without one).

    This is TIGHTER than the ball form that the penalty controls and traj_stop_margin reports: it looks along the direction of
    motion only.  The expectation, not a theorem, is that a sample with ball margin >= 0 at a clearance >= 0 is also safe here, up
    to the interpolation error of the field (the ball is measured between voxel centres, the walk tests whole voxels)."""
    import torch
    coeffs = _f64(coeffs); T = _f64(T)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N):
        raise ValueError("shape mismatch")
    if not (a_brake > 0.0) or not (t_react >= 0.0 and math.isfinite(t_react)) or res < 1:
        raise ValueError("a_brake > 0, t_react >= 0 and finite, res >= 1")
    ctx = ctx or vm.ctx
    # every piece as a trajectory of its own: the local times then address the piece itself, also at its two ends
    one = coeffs.reshape(B * N, 1, 3, D)
    Tq = T.reshape(B * N, 1)
    tq = (np.arange(res + 1, dtype=np.float64) / np.float64(res))[None, :] * Tq
    p = traj_eval(one, Tq, tq, 0, ctx=ctx).reshape(-1, 3)
    v = traj_eval(one, Tq, tq, 1, ctx=ctx).reshape(-1, 3)
    vv = (v * v).sum(1)
    speed = np.sqrt(vv)
    length = t_react * speed + vv / (2.0 * a_brake)
    with np.errstate(invalid="ignore", divide="ignore"):
        ends = np.where(speed[:, None] > 0.0, p + v / speed[:, None] * length[:, None], p)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(vm.device)
    voxel, _ = vm.raycast(dev(p), dev(ends))
    from .trajectory import HIT_FREE
    unsafe = ((voxel != HIT_FREE) | vm.query(ends)).reshape(B, N * (res + 1))
    count = unsafe.sum(1).astype(np.int64)
    first = np.where(count > 0, unsafe.argmax(1), -1).astype(np.int64)
    return count, first
