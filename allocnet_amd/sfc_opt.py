"""Corridor-constrained MINCO optimisation: every waypoint a convex combination of the vertices of the overlap of the two
polytopes it joins, P_w = (sum_j xi_j^2 v_j) / sum_j xi_j^2 (upstream GCOPTER's forwardP / backwardGradP / backwardP), and the
L-BFGS over (xi, tau) on top of it -- so every iterate has its junctions inside the corridor, as every iterate has positive
durations.  The transform, its gradient, the norm restriction and the inverse are stated once, in
allocnet_amd/csrc/sfc_param_kernels.h; the entry points in include/allocnet_amd.h (anet_sfc_*, anet_lbfgs_minco_sfc*).  Its
starting point -- the shortest route through the corridor in the same variables (upstream's getShortestPath,
allocnet_amd/csrc/sfc_path_kernels.h), pieces per polytope, first waypoints and durations -- is `sfc_setup` at the end.

Host functions take trajectory-major numpy arrays: hpolys (B, N, M, 4) rows a.x <= b with zero rows as padding (what
`to_planner_form` returns), xi (B, N-1, K), verts (B, N-1, K, 3), count / status (B, N-1), wps (B, N-1, 3).  The `_dev`
functions take torch CUDA tensors, batch-minor with a common row stride ld: xi (N-1)K x ld, verts (N-1)K3 x ld, count / status
(N-1) x ld int32, wps 3(N-1) x ld."""
import ctypes

import numpy as np

from .context import default_context
from .lbfgs import OPT_TIMES, OPT_WAYPOINTS, lbfgs_parameter_t
from .polytope import POLYTOPE_OK, POLYTOPE_SKIPPED, POLYTOPE_TRUNCATED  # noqa: F401

SFC_NO_OVERLAP = -2048


def _q(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _vp(o):
    return ctypes.cast(ctypes.pointer(o), ctypes.c_void_p) if o is not None else None


def _stream(stream, dev):
    import torch
    return ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)


def _ld(B):
    from .minco import recommended_ld
    return 1 if B == 1 else recommended_ld(B)


def _bm(a, B, dtype=None, ctx=None):
    """(B, ...) numpy -> batch-minor torch CUDA tensor (fields, ld) on the context's device."""
    import torch
    f = np.ascontiguousarray(np.asarray(a).reshape(B, -1).T)
    dev = torch.device("cuda", (ctx or default_context()).device)
    t = torch.zeros(f.shape[0], _ld(B), device=dev, dtype=dtype or torch.float64)
    t[:, :B] = torch.from_numpy(f).to(t.device, t.dtype)
    return t


def _tm(t, B, shape=()):
    """batch-minor torch tensor (fields, ld) -> (B, *shape) numpy."""
    return np.ascontiguousarray(t[:, :B].cpu().numpy().T).reshape((B,) + tuple(shape))


def sfc_overlap_vertices_dev(hpolys, N, B, M, max_verts, epsilon=1e-6, verts=None, count=None, status=None, stream=None, ctx=None):
    """anet_sfc_overlap_vertices_dev: hpolys (N M 4, ld) as `minco_cost_grad_dev` takes it.  Returns dict(verts ((N-1) K 3, ld),
    count ((N-1), ld) int32 clamped to K, status ((N-1), ld) int32: 0 ok, 1 no interior, 2 truncated to max_verts); the three may
    be passed in (same row stride)."""
    import torch
    ctx = ctx or default_context(hpolys.device.index or 0)
    ld, dev, K = hpolys.stride(0), hpolys.device, int(max_verts)
    verts = verts if verts is not None else torch.zeros((N - 1) * K * 3, ld, device=dev, dtype=torch.float64)
    count = count if count is not None else torch.zeros(N - 1, ld, device=dev, dtype=torch.int32)
    status = status if status is not None else torch.zeros(N - 1, ld, device=dev, dtype=torch.int32)
    work = torch.empty(max(1, ctx.lib.anet_sfc_overlap_workspace(N, B, M, K)), device=dev, dtype=torch.float64)
    ctx.check(ctx.lib.anet_sfc_overlap_vertices_dev(ctx.handle, N, B, ld, M, _q(hpolys), float(epsilon), K, _q(verts), _q(count),
                                                    _q(status), _q(work), _stream(stream, dev)))
    return dict(verts=verts, count=count, status=status)


def sfc_default_max_verts(hpolys, epsilon=1e-6, ctx=None):
    """The next multiple of 8 above the largest vertex count among the overlaps of the corridors hpolys (B, N, M, 4): one
    enumeration call that only counts (anet_polytope_vertices with room for one vertex reports the true counts)."""
    ctx = ctx or default_context()
    hp = np.ascontiguousarray(hpolys, dtype=np.float64)
    B, N, M, _ = hp.shape
    stacked = np.concatenate([hp[:, :-1], hp[:, 1:]], axis=2).reshape(B * (N - 1), 2 * M, 4).copy()
    stacked[:, :, 3] *= -1.0
    cnt = np.zeros(B * (N - 1), dtype=np.int32)
    one = np.zeros((B * (N - 1), 1, 3))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ctx.check(ctx.lib.anet_polytope_vertices(ctx.handle, B * (N - 1), 2 * M, p(stacked), float(epsilon), 1, p(one), p(cnt), None, None))
    return (int(cnt.max(initial=0)) // 8 + 1) * 8


def sfc_overlap_vertices(hpolys, max_verts=None, epsilon=1e-6, ctx=None):
    """The vertices of overlap(polytope w, polytope w + 1) for every junction of every corridor (anet_sfc_overlap_vertices_dev).
    max_verts None: the next multiple of 8 above the largest overlap's count (one extra enumeration call that only counts).
    Returns dict(verts (B, N-1, K, 3), count (B, N-1), status (B, N-1), max_verts)."""
    ctx = ctx or default_context()
    hp = np.ascontiguousarray(hpolys, dtype=np.float64)
    B, N, M, _ = hp.shape
    K = int(max_verts) if max_verts is not None else sfc_default_max_verts(hp, epsilon, ctx)
    out = sfc_overlap_vertices_dev(_bm(hp, B, ctx=ctx), N, B, M, K, epsilon, ctx=ctx)
    return dict(verts=_tm(out["verts"], B, (N - 1, K, 3)), count=_tm(out["count"], B, (N - 1,)),
                status=_tm(out["status"], B, (N - 1,)), max_verts=K)


def sfc_forward_p_dev(xi, verts, N, B, max_verts, w_norm=1.0, wps=None, norm=None, stream=None, ctx=None):
    """anet_sfc_forward_p_dev.  Returns dict(wps (3(N-1), ld), norm (3(N-1), ld): rows w 1 / S, rows (N-1) + w the norm cost,
    rows 2(N-1) + w the norm gradient factor)."""
    import torch
    ctx = ctx or default_context(xi.device.index or 0)
    ld, dev = xi.stride(0), xi.device
    wps = wps if wps is not None else torch.zeros(3 * (N - 1), ld, device=dev, dtype=torch.float64)
    norm = norm if norm is not None else torch.zeros(3 * (N - 1), ld, device=dev, dtype=torch.float64)
    ctx.check(ctx.lib.anet_sfc_forward_p_dev(ctx.handle, N, B, ld, int(max_verts), _q(xi), _q(verts), float(w_norm), _q(wps),
                                             _q(norm), _stream(stream, dev)))
    return dict(wps=wps, norm=norm)


def sfc_forward_p(xi, verts, w_norm=1.0, ctx=None):
    """P(xi) for xi (B, N-1, K), verts (B, N-1, K, 3) (anet_sfc_forward_p_dev).  Returns dict(wps (B, N-1, 3), inv_s (B, N-1),
    norm_cost (B, N-1))."""
    xi = np.asarray(xi, dtype=np.float64)
    B, Nm1, K = xi.shape
    ctx = ctx or default_context()
    out = sfc_forward_p_dev(_bm(xi, B, ctx=ctx), _bm(verts, B, ctx=ctx), Nm1 + 1, B, K, w_norm, ctx=ctx)
    nrm = _tm(out["norm"], B, (3, Nm1))
    return dict(wps=_tm(out["wps"], B, (Nm1, 3)), inv_s=nrm[:, 0], norm_cost=nrm[:, 1])


def sfc_backward_grad_p_dev(xi, verts, wps, norm, grad_p, N, B, max_verts, grad_xi=None, cost=None, stream=None, ctx=None):
    """anet_sfc_backward_grad_p_dev: dJ/dxi ((N-1) K, ld) from dJ/dP (3(N-1), ld) and the wps / norm rows `sfc_forward_p_dev`
    left, the norm term included; cost ((ld,) or None) receives the problem's norm costs on top of what it holds."""
    import torch
    ctx = ctx or default_context(xi.device.index or 0)
    ld, dev = xi.stride(0), xi.device
    grad_xi = grad_xi if grad_xi is not None else torch.zeros_like(xi)
    ctx.check(ctx.lib.anet_sfc_backward_grad_p_dev(ctx.handle, N, B, ld, int(max_verts), _q(xi), _q(verts), _q(wps), _q(norm),
                                                   _q(grad_p), _q(grad_xi), _q(cost), _stream(stream, dev)))
    return grad_xi


def sfc_backward_p_dev(verts, count, wps, N, B, max_verts, stream=None, ctx=None):
    """anet_sfc_backward_p_dev: xi of unit norm per waypoint with P(xi) nearest to wps.  Returns dict(xi ((N-1) K, ld), residual
    ((N-1), ld) = |P(xi) - wps|).  Synchronises the stream (completion polls of the lockstep L-BFGS)."""
    import torch
    ctx = ctx or default_context(verts.device.index or 0)
    ld, dev, K = verts.stride(0), verts.device, int(max_verts)
    xi = torch.zeros((N - 1) * K, ld, device=dev, dtype=torch.float64)
    residual = torch.zeros(N - 1, ld, device=dev, dtype=torch.float64)
    work = torch.empty(ctx.lib.anet_sfc_backward_p_workspace(N, K, ld), device=dev, dtype=torch.float64)
    ctx.check(ctx.lib.anet_sfc_backward_p_dev(ctx.handle, N, B, ld, K, _q(verts), _q(count), _q(wps), _q(xi), _q(residual), _q(work),
                                              _stream(stream, dev)))
    return dict(xi=xi, residual=residual)


def sfc_backward_p(wps, verts, count, ctx=None):
    """backward_p for wps (B, N-1, 3), verts (B, N-1, K, 3), count (B, N-1) (anet_sfc_backward_p_dev).  Returns dict(xi (B, N-1, K),
    residual (B, N-1)): the minimiser is not unique for more than four vertices -- P(xi) and the residual are the results; a
    waypoint outside its overlap keeps a positive residual."""
    import torch
    verts = np.asarray(verts, dtype=np.float64)
    B, Nm1, K, _ = verts.shape
    ctx = ctx or default_context()
    out = sfc_backward_p_dev(_bm(verts, B, ctx=ctx), _bm(np.asarray(count, dtype=np.int32), B, torch.int32, ctx=ctx), _bm(wps, B, ctx=ctx),
                             Nm1 + 1, B, K, ctx=ctx)
    return dict(xi=_tm(out["xi"], B, (Nm1, K)), residual=_tm(out["residual"], B, (Nm1,)))


def lbfgs_minco_sfc_dev(head, tail, xi, T, verts, count, s, c, N, B, max_verts, hpolys=None, penalty=None, param=None,
                        opt=OPT_WAYPOINTS | OPT_TIMES, max_evals=2000, min_duration=0.0, w_norm=1.0, overlap_status=None,
                        coeffs=None, stream=None, ctx=None):
    """anet_lbfgs_minco_sfc_dev: L-BFGS over (xi, tau), lockstep shape.  xi ((N-1) K, ld) and T (N, ld) are updated in place.
    Returns dict(cost, status, iters, evals (B,), wps (3(N-1), ld) = P(xi) of the final iterate).  A problem with a waypoint
    of count < 2 or overlap status 1 reports SFC_NO_OVERLAP, zero counters, cost NaN and keeps its xi and T."""
    import torch
    ctx = ctx or default_context(T.device.index or 0)
    param = param or lbfgs_parameter_t()
    ld, dev, K = T.stride(0), T.device, int(max_verts)
    work = torch.empty(ctx.lib.anet_sfc_workspace(s, N, K, ld, _vp(param)), device=dev, dtype=torch.float64)
    cost = torch.empty(ld, device=dev, dtype=torch.float64)
    wps = torch.zeros(3 * (N - 1), ld, device=dev, dtype=torch.float64)
    status, iters, evals = (torch.empty(ld, device=dev, dtype=torch.int32) for _ in range(3))
    ctx.check(ctx.lib.anet_lbfgs_minco_sfc_dev(
        ctx.handle, s, c, N, B, ld, _q(head), _q(tail), _q(xi), _q(T), _q(verts), _q(count), _q(overlap_status), K, _q(hpolys),
        _vp(penalty), _vp(param), int(opt), int(max_evals), float(min_duration), float(w_norm), _q(work), _q(cost), _q(wps),
        _q(coeffs), _q(status), _q(iters), _q(evals), _stream(stream, dev)))
    return dict(cost=cost[:B], status=status[:B], iters=iters[:B], evals=evals[:B], wps=wps)


def lbfgs_minco_sfc(head, tail, hpolys, T, s, wps=None, penalty=None, param=None, opt=OPT_WAYPOINTS | OPT_TIMES, max_evals=2000,
                    min_duration=0.0, w_norm=1.0, max_verts=None, epsilon=1e-6, want_coeffs=True, ctx=None):
    """Corridor-constrained `lbfgs_minco` (anet_lbfgs_minco_sfc): hpolys (B, N, M, 4) with M = penalty.poly_rows, wps (B, N-1, 3)
    start waypoints or None (None: the mean of each overlap's vertices).  Overlap enumeration, backward_p, then the L-BFGS over
    (xi, tau).  max_verts None: the next multiple of 8 above the largest overlap count.  Returns dict(wps, T, cost, coeffs,
    status, iters, evals, residual (B, N-1): how far backward_p's start is from the given wps, overlap_status (B, N-1), xi
    (B, N-1, K), max_verts); every returned waypoint satisfies the rows of both polytopes it joins within epsilon."""
    ctx = ctx or default_context()
    param = param or lbfgs_parameter_t()
    if penalty is None:
        raise ValueError("lbfgs_minco_sfc: penalty (with poly_rows) is required")
    head = np.ascontiguousarray(head, dtype=np.float64)
    tail = np.ascontiguousarray(tail, dtype=np.float64)
    B, _, c = head.shape
    T = np.array(T, dtype=np.float64).copy()
    N = T.shape[1]
    hp = np.ascontiguousarray(hpolys, dtype=np.float64)
    if hp.shape != (B, N, penalty.poly_rows, 4):
        raise ValueError("hpolys must be (B, N, penalty.poly_rows, 4)")
    K = int(max_verts) if max_verts is not None else sfc_default_max_verts(hp, epsilon, ctx)
    w0 = None if wps is None else np.ascontiguousarray(wps, dtype=np.float64).reshape(B, N - 1, 3)
    out_w = np.empty((B, N - 1, 3)); cost = np.empty(B)
    coeffs = np.empty((B, N, 3, 2 * s)) if want_coeffs else None
    status, iters, evals = (np.empty(B, dtype=np.int32) for _ in range(3))
    residual = np.empty((B, N - 1)); ostat = np.empty((B, N - 1), dtype=np.int32); xi = np.empty((B, N - 1, K))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    ctx.check(ctx.lib.anet_lbfgs_minco_sfc(
        ctx.handle, s, c, N, B, p(head), p(tail), p(w0), p(T), p(hp), _vp(penalty), _vp(param), int(opt), int(max_evals),
        float(min_duration), float(w_norm), float(epsilon), K, p(out_w), p(cost), p(coeffs), p(status), p(iters), p(evals),
        p(residual), p(ostat), p(xi)))
    return dict(wps=out_w, T=T, cost=cost, coeffs=coeffs, status=status, iters=iters, evals=evals, residual=residual,
                overlap_status=ostat, xi=xi, max_verts=K)


# ---- the shortest route through a corridor, and the setup of an optimisation on top of it -------------------------------------------
SFC_PATH_MAX_EVALS = 400


def sfc_path_cost_grad_dev(start, goal, xi, verts, N, B, max_verts, eps=1e-2, w_norm=1.0, cost=None, grad_xi=None, stream=None, ctx=None):
    """anet_sfc_path_cost_grad_dev: one evaluation of the route objective, one launch.  start, goal (3, ld), xi ((N-1) K, ld), verts
    ((N-1) K 3, ld).  Returns (cost (ld,): sum of the smoothed legs plus the norm terms, grad_xi ((N-1) K, ld))."""
    import torch
    ctx = ctx or default_context(xi.device.index or 0)
    ld, dev = xi.stride(0), xi.device
    cost = cost if cost is not None else torch.zeros(ld, device=dev, dtype=torch.float64)
    grad_xi = grad_xi if grad_xi is not None else torch.zeros_like(xi)
    ctx.check(ctx.lib.anet_sfc_path_cost_grad_dev(ctx.handle, N, B, ld, int(max_verts), _q(start), _q(goal), _q(xi), _q(verts), float(eps),
                                                  float(w_norm), _q(cost), _q(grad_xi), _stream(stream, dev)))
    return cost, grad_xi


def sfc_shortest_path_dev(start, goal, verts, count, N, B, max_verts, xi=None, overlap_status=None, eps=1e-2, w_norm=1.0, param=None,
                          max_evals=SFC_PATH_MAX_EVALS, work=None, stream=None, ctx=None):
    """anet_sfc_shortest_path_dev: the shortest smoothed polyline start -> one point in every overlap -> goal, L-BFGS over the xi
    rows ((N-1) K, ld).  start, goal (3, ld); verts, count, overlap_status as `sfc_overlap_vertices_dev` returns them.  xi None: the
    run starts from the vertex mean; else xi is the start and is updated in place.  param None: the defaults (mem_size 8, past 3,
    delta 1e-6, g_epsilon 1e-5).  Returns dict(xi, wps (3(N-1), ld) = P(xi), length (B,): the unsmoothed polyline length, cost (B,):
    the smoothed objective, status, iters, evals (B,), work).  A problem with a waypoint of count < 2 or overlap status 1 reports
    SFC_NO_OVERLAP, zero counters, length NaN and keeps its xi.  Synchronises the stream (completion polls of the lockstep L-BFGS)."""
    import torch
    ctx = ctx or default_context(verts.device.index or 0)
    ld, dev, K = verts.stride(0), verts.device, int(max_verts)
    from_mean = xi is None
    if from_mean:
        xi = torch.zeros((N - 1) * K, ld, device=dev, dtype=torch.float64)
    if work is None:
        work = torch.empty(ctx.lib.anet_sfc_shortest_path_workspace(N, K, ld, _vp(param)), device=dev, dtype=torch.float64)
    wps = torch.zeros(3 * (N - 1), ld, device=dev, dtype=torch.float64)
    length, cost = (torch.empty(ld, device=dev, dtype=torch.float64) for _ in range(2))
    status, iters, evals = (torch.empty(ld, device=dev, dtype=torch.int32) for _ in range(3))
    ctx.check(ctx.lib.anet_sfc_shortest_path_dev(
        ctx.handle, N, B, ld, K, _q(start), _q(goal), _q(verts), _q(count), _q(overlap_status), _q(xi), int(from_mean), float(eps),
        float(w_norm), _vp(param), int(max_evals), _q(work), _q(wps), _q(length), _q(cost), _q(status), _q(iters), _q(evals),
        _stream(stream, dev)))
    return dict(xi=xi, wps=wps, length=length[:B], cost=cost[:B], status=status[:B], iters=iters[:B], evals=evals[:B], work=work)


def sfc_shortest_path(start, goal, hpolys, max_verts=None, epsilon=1e-6, eps=1e-2, w_norm=1.0, param=None,
                      max_evals=SFC_PATH_MAX_EVALS, ctx=None):
    """The shortest route through corridors (anet_sfc_shortest_path; upstream GCOPTER's getShortestPath): start, goal (B, 3), hpolys
    (B, N, M, 4) rows a.x <= b with zero rows as padding.  Overlap enumeration, then the L-BFGS from the vertex means.  max_verts
    None: the next multiple of 8 above the largest overlap count.  Returns dict(wps (B, N-1, 3): one point in every overlap, length
    (B,): the polyline length start -> wps -> goal, status, iters, evals, overlap_status (B, N-1), xi (B, N-1, K), max_verts)."""
    ctx = ctx or default_context()
    hp = np.ascontiguousarray(hpolys, dtype=np.float64)
    B, N, M, _ = hp.shape
    start = np.ascontiguousarray(start, dtype=np.float64).reshape(B, 3)
    goal = np.ascontiguousarray(goal, dtype=np.float64).reshape(B, 3)
    K = int(max_verts) if max_verts is not None else sfc_default_max_verts(hp, epsilon, ctx)
    wps = np.empty((B, N - 1, 3)); length = np.empty(B)
    status, iters, evals = (np.empty(B, dtype=np.int32) for _ in range(3))
    ostat = np.empty((B, N - 1), dtype=np.int32); xi = np.empty((B, N - 1, K))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ctx.check(ctx.lib.anet_sfc_shortest_path(ctx.handle, N, B, M, p(hp), p(start), p(goal), float(epsilon), K, float(eps), float(w_norm),
                                             _vp(param), int(max_evals), p(wps), p(length), p(status), p(iters), p(evals), p(ostat),
                                             p(xi)))
    return dict(wps=wps, length=length, status=status, iters=iters, evals=evals, overlap_status=ostat, xi=xi, max_verts=K)


def sfc_allot_pieces(route_points, length_per_piece):
    """Pieces per polytope from a route (upstream's lengthPerPiece): route_points (..., N+1, 3) = start, one point per overlap,
    goal; polytope i carries leg i and gets ceil(|leg i| / length_per_piece) pieces, at least 1.  Returns int64 (..., N)."""
    if not length_per_piece > 0.0:
        raise ValueError("sfc_allot_pieces: length_per_piece must be > 0")
    legs = np.linalg.norm(np.diff(np.asarray(route_points, dtype=np.float64), axis=-2), axis=-1)
    return np.maximum(np.ceil(legs / float(length_per_piece)), 1.0).astype(np.int64)


def sfc_expand_corridor(hpolys, pieces):
    """hpolys (N, M, 4) with polytope i repeated pieces[i] times: (sum(pieces), M, 4).  A waypoint between two copies of a polytope
    then has that polytope's own vertices for its overlap: the stacked pair's duplicated rows only add singular triples and
    repeated points, which the enumeration drops."""
    hp = np.asarray(hpolys, dtype=np.float64)
    pieces = np.asarray(pieces, dtype=np.int64)
    if hp.ndim != 3 or pieces.shape != (hp.shape[0],) or (pieces < 1).any():
        raise ValueError("sfc_expand_corridor: hpolys (N, M, 4) and pieces (N,) >= 1")
    return np.repeat(hp, pieces, axis=0)


def sfc_route_waypoints(route_points, pieces):
    """The waypoints of the expanded corridor: the route's inner points, and pieces[i] - 1 points evenly spaced on leg i.
    route_points (N+1, 3) -> (sum(pieces) - 1, 3), and the piece lengths (sum(pieces),): |leg i| / pieces[i] each."""
    r = np.asarray(route_points, dtype=np.float64)
    wps, lens = [], []
    for i, k in enumerate(np.asarray(pieces, dtype=np.int64)):
        leg = r[i + 1] - r[i]
        for j in range(1, int(k) + 1):
            wps.append(r[i] + leg * (j / float(k)) if j < k else r[i + 1])
        lens += [np.linalg.norm(leg) / float(k)] * int(k)
    return np.array(wps[:-1]).reshape(-1, 3), np.array(lens)


def sfc_first_durations(piece_lengths, speed, min_duration=0.0):
    """T_i = max(len_i / speed, min_duration)."""
    if not speed > 0.0:
        raise ValueError("sfc_first_durations: speed must be > 0")
    return np.maximum(np.asarray(piece_lengths, dtype=np.float64) / float(speed), float(min_duration))


def sfc_setup(start, goal, hpolys, length_per_piece, speed, min_duration=1e-2, max_verts=None, epsilon=1e-6, eps=1e-2, w_norm=1.0,
              param=None, max_evals=SFC_PATH_MAX_EVALS, ctx=None):
    """What upstream GCOPTER's setup() does before its optimisation: the shortest route through every corridor
    (`sfc_shortest_path`), pieces per polytope from its legs (`sfc_allot_pieces`), the corridor with every polytope repeated per
    piece (`sfc_expand_corridor`), inner waypoints evenly spaced on their leg and first durations max(len / speed, min_duration).
    start, goal (B, 3), hpolys (B, N, M, 4).  Problems end with different piece counts, so the result is a list of groups by
    ascending piece count (as `learning_planner.group_by_seg` groups by polytope count), each a dict(hpolys (Bg, Ng, M, 4), wps
    (Bg, Ng-1, 3), T (Bg, Ng), pieces (Bg, N), index (Bg,): the problems' positions in the batch, route (Bg, N+1, 3), length (Bg,))
    that `lbfgs_minco_sfc(head[index], tail[index], hpolys, T, s, wps=wps, ...)` takes as it is.  A problem whose route did not run
    (SFC_NO_OVERLAP) is in no group."""
    from .learning_planner import group_by_seg
    hp = np.ascontiguousarray(hpolys, dtype=np.float64)
    B, N, M, _ = hp.shape
    start = np.asarray(start, dtype=np.float64).reshape(B, 3)
    goal = np.asarray(goal, dtype=np.float64).reshape(B, 3)
    route = sfc_shortest_path(start, goal, hp, max_verts, epsilon, eps, w_norm, param, max_evals, ctx)
    pts = np.concatenate([start[:, None], route["wps"], goal[:, None]], axis=1)          # (B, N+1, 3)
    keep = route["status"] != SFC_NO_OVERLAP
    pieces = np.ones((B, N), dtype=np.int64)
    pieces[keep] = sfc_allot_pieces(pts[keep], length_per_piece)
    groups = []
    for seg, idx in group_by_seg(pieces.sum(1), keep).items():
        g = dict(hpolys=np.empty((len(idx), seg, M, 4)), wps=np.empty((len(idx), seg - 1, 3)), T=np.empty((len(idx), seg)),
                 pieces=pieces[idx], index=np.array(idx, dtype=np.int64), route=pts[idx], length=route["length"][idx])
        for r, b in enumerate(idx):
            g["hpolys"][r] = sfc_expand_corridor(hp[b], pieces[b])
            g["wps"][r], lens = sfc_route_waypoints(pts[b], pieces[b])
            g["T"][r] = sfc_first_durations(lens, speed, min_duration)
        groups.append(g)
    return groups
