"""Corridor-constrained MINCO optimisation: every waypoint a convex combination of the vertices of the overlap of the two
polytopes it joins, P_w = (sum_j xi_j^2 v_j) / sum_j xi_j^2 (upstream GCOPTER's forwardP / backwardGradP / backwardP), and the
L-BFGS over (xi, tau) on top of it -- so every iterate has its junctions inside the corridor, as every iterate has positive
durations.  The transform, its gradient, the norm restriction and the inverse are stated once, in
allocnet_amd/csrc/sfc_param_kernels.h; the entry points in include/allocnet_amd.h (anet_sfc_*, anet_lbfgs_minco_sfc*).

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
