"""The whole body in the corridor: the vertices of a body-fixed polytope, rotated by the attitude the trajectory itself implies
(the quaternion of the flatness map at v(t), a(t), psi = 0), held inside the corridor polytopes -- as a penalty of the MINCO
objective with its gradient, and as a sampled margin.  A flat vehicle can so roll to pass a slot narrower than its span, which
no dilation of the map expresses.

All arithmetic runs in the HIP kernels of csrc/body_kernels.h behind anet_minco_body_partial_grads_dev and
anet_traj_body_margin[_dev]; the semantics are stated in include/allocnet_amd.h.
"""
import itertools

import numpy as np

from ._lib import ANET_MAX_BODY_VERTS, BodyPenalty
from .context import default_context
from .flatness import _f64, _params_of, _ptr, _ref, _stream_of, _tptr


def box_body(half_extents):
    """The 8 vertices (+-hx, +-hy, +-hz) of a box in the body frame, (8, 3)."""
    h = _f64(half_extents, (3,))
    return np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx, sy, sz in itertools.product((-1.0, 1.0), repeat=3)])


def make_body_penalty(verts, w=100.0, smooth_mu=0.05, res=20, poly_rows=1):
    """struct anet_body_penalty: the body vertices (K, 3) in the body frame in metres, K <= 16, the weight, smoothedL1 mu (m), the
    samples per piece and the rows per polytope of the hpolys it will be used with."""
    verts = _f64(verts)
    if verts.ndim != 2 or verts.shape[1] != 3 or not 1 <= verts.shape[0] <= ANET_MAX_BODY_VERTS:
        raise ValueError(f"verts must be (K, 3) with 1 <= K <= {ANET_MAX_BODY_VERTS}")
    pen = BodyPenalty(float(w), float(smooth_mu), int(res), int(poly_rows), verts.shape[0], 0)
    for k in range(verts.shape[0]):
        for c in range(3):
            pen.verts[k][c] = verts[k, c]
    return pen


def _body_of(body, res=None, poly_rows=None):
    """a BodyPenalty (copied, with res / poly_rows replaced where given) or an array of vertices"""
    if isinstance(body, BodyPenalty):
        pen = BodyPenalty.from_buffer_copy(body)
        if res is not None:
            pen.res = int(res)
        if poly_rows is not None:
            pen.poly_rows = int(poly_rows)
        return pen
    return make_body_penalty(body, res=20 if res is None else res, poly_rows=1 if poly_rows is None else poly_rows)


def minco_body_partial_grads_dev(params, body_penalty, s, N, B, coeffs, T, hpolys, gdC, gdT, piece_cost=None, accumulate=False,
                                 stream=None, ctx=None):
    """anet_minco_body_partial_grads_dev on batch-minor torch CUDA float64 tensors with the row stride of T; hpolys
    (N * poly_rows * 4, ld) as for minco_cost_grad_dev."""
    ctx = ctx or default_context(T.device.index or 0)
    ctx.check(ctx.lib.anet_minco_body_partial_grads_dev(ctx.handle, _ref(_params_of(params)), _ref(body_penalty), int(s), int(N),
                                                        int(B), T.stride(0), _tptr(coeffs), _tptr(T), _tptr(hpolys),
                                                        1 if accumulate else 0, _tptr(gdC), _tptr(gdT), _tptr(piece_cost),
                                                        _stream_of(T, stream)))
    return gdC, gdT, piece_cost


def minco_body_cost_grad_dev(head, tail, wps, T, s, c, N, B, flatmap, body_penalty, body_hpolys, hpolys=None, penalty=None,
                             stream=None, ctx=None):
    """J = int (p^(s))^2 + rho sum T + J_pen + J_body and its gradient, composed at the C ABI as minco_obstacle_cost_grad_dev is:
    anet_minco_solve_dev -> anet_minco_partial_grads_dev -> anet_minco_body_partial_grads_dev(accumulate = 1) ->
    anet_minco_propagate_grad_dev.  body_hpolys (N * body_penalty.poly_rows * 4, ld): the corridor the body is held in; hpolys /
    penalty: the point terms of minco_cost_grad_dev (they may name the same corridor, another one or none).
    Batch-minor torch CUDA float64 tensors with a common row stride.
    Returns cost (ld,), gradP (max(3 (N-1), 1), ld), gradT (N, ld), coeffs (N*3*2s, ld)."""
    import torch
    from .minco import minco_solve_dev
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    st = _stream_of(T, stream)
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
    zeros = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float64)
    coeffs, energy = new(N * 3 * 2 * s, ld), new(ld)
    minco_solve_dev(head, tail, wps, T, s, c, N, B, coeffs=coeffs, energy=energy, stream=st.value, ctx=ctx)
    gdC, gdT, pc = new(N * 3 * 2 * s, ld), new(N, ld), zeros(N, ld)
    ctx.check(ctx.lib.anet_minco_partial_grads_dev(ctx.handle, s, N, B, ld, _tptr(coeffs), _tptr(T), _tptr(hpolys),
                                                   _ref(penalty) if penalty is not None else None, 1, _tptr(gdC), _tptr(gdT),
                                                   _tptr(pc), st))
    minco_body_partial_grads_dev(flatmap, body_penalty, s, N, B, coeffs, T, body_hpolys, gdC, gdT, pc, accumulate=True,
                                 stream=st.value, ctx=ctx)
    gradP, gradT = zeros(max(3 * (N - 1), 1), ld), new(N, ld)
    ctx.check(ctx.lib.anet_minco_propagate_grad_dev(ctx.handle, s, c, N, B, ld, _tptr(T), _tptr(coeffs), _tptr(gdC), _tptr(gdT),
                                                    _tptr(gradP), _tptr(gradT), st))
    # the adjoint kernel is given no cost to assemble here: the sum of the terms and rho's share of the time gradient
    rho = penalty.rho if penalty is not None else 0.0
    cost = energy + rho * T.sum(0) + pc.sum(0)
    if rho != 0.0:
        gradT = gradT + rho
    return cost, gradP, gradT, coeffs


def minco_body_cost_grad(head, tail, wps, T, s, flatmap, body_penalty, body_hpolys, hpolys=None, penalty=None, ctx=None):
    """Host (numpy, trajectory-major) form of minco_body_cost_grad_dev, with minco_cost_grad's shapes: head, tail (B, 3, c);
    wps (B, N-1, 3); T (B, N); body_hpolys (B, N, body_penalty.poly_rows, 4); hpolys (B, N, penalty.poly_rows, 4).
    Returns cost (B,), gradP (B, N-1, 3), gradT (B, N)."""
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
    body_hpolys = _f64(body_hpolys, (B, N, body_penalty.poly_rows, 4))
    d_hp = None
    if hpolys is not None:
        hpolys = _f64(hpolys)
        if penalty is None or hpolys.shape != (B, N, penalty.poly_rows, 4):
            raise ValueError("hpolys must be (B, N, penalty.poly_rows, 4)")
        d_hp = up(hpolys.reshape(B, -1))
    cost, gP, gT, _ = minco_body_cost_grad_dev(up(head.reshape(B, -1)), up(tail.reshape(B, -1)), up(wps.reshape(B, -1)), d_T, s, c,
                                               N, B, flatmap, body_penalty, up(body_hpolys.reshape(B, -1)), hpolys=d_hp,
                                               penalty=penalty, ctx=ctx)
    gradP = gP[:3 * (N - 1), :B].T.contiguous().cpu().numpy().reshape(B, N - 1, 3)
    return cost[:B].cpu().numpy(), gradP, gT[:, :B].T.contiguous().cpu().numpy()


def body_objective_dev(head, tail, s, c, N, B, flatmap, body_penalty, body_hpolys, hpolys=None, penalty=None, ctx=None):
    """The composed objective as an `evaluate(x, f, g)` of lbfgs_optimize_dev, as obstacle_objective_dev: x (3 (N-1) + N, ld) holds
    the waypoints (the rows of minco_cost_grad_dev's wps) and below them the LOG durations, so that every duration stays positive;
    g is the gradient w.r.t. x (dJ/dlog T = T dJ/dT)."""
    import torch
    nw = 3 * (N - 1)

    def evaluate(x, f, g):
        T = torch.exp(x[nw:nw + N])
        wps = x[:nw] if nw else torch.zeros(1, x.shape[1], device=x.device, dtype=torch.float64)
        cost, gP, gT, _ = minco_body_cost_grad_dev(head, tail, wps, T, s, c, N, B, flatmap, body_penalty, body_hpolys,
                                                   hpolys=hpolys, penalty=penalty, ctx=ctx)
        f.copy_(cost)
        if nw:
            g[:nw].copy_(gP[:nw])
        g[nw:nw + N].copy_(gT * T)
    return evaluate


def traj_body_margin(flatmap, body, coeffs, T, hpolys, res=20, ctx=None):
    """The sampled body margin per piece (anet_traj_body_margin): the maximum of a_r . (p(t) + R(q(t)) b_k) - h_r over
    t = j T_i / res, j = 0..res, the non-padding rows of the piece's polytope and the body vertices.  body: vertices (K, 3) or a
    BodyPenalty; coeffs (B, N, 3, D), T (B, N), hpolys (B, N, M, 4) -> margin (B, N), t (B, N) local time, row, vert (B, N) int32.
    -inf: the piece has no row; NaN: a non-finite coefficient, duration or row field of that piece."""
    ctx = ctx or default_context()
    coeffs = _f64(coeffs); T = _f64(T); hpolys = _f64(hpolys)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N) or hpolys.ndim != 4 or hpolys.shape[:2] != (B, N) or hpolys.shape[3] != 4:
        raise ValueError("shape mismatch")
    pen = _body_of(body, res, hpolys.shape[2])
    margin, t = np.empty((B, N)), np.empty((B, N))
    row, vert = np.empty((B, N), dtype=np.int32), np.empty((B, N), dtype=np.int32)
    ctx.check(ctx.lib.anet_traj_body_margin(ctx.handle, _ref(_params_of(flatmap)), _ref(pen), D // 2, N, B, _ptr(coeffs), _ptr(T),
                                            _ptr(hpolys), _ptr(margin), _ptr(t), _ptr(row), _ptr(vert)))
    return margin, t, row, vert


def traj_body_margin_dev(flatmap, body_penalty, s, N, B, coeffs, T, hpolys, margin=None, t=None, row=None, vert=None,
                         stream=None, ctx=None):
    """anet_traj_body_margin_dev on batch-minor torch CUDA tensors with the row stride of T: coeffs (N*3*2s, ld), T (N, ld),
    hpolys (N * body_penalty.poly_rows * 4, ld) -> margin, t (N, ld) float64, row, vert (N, ld) int32."""
    import torch
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    margin = margin if margin is not None else torch.empty(N, ld, device=dev, dtype=torch.float64)
    t = t if t is not None else torch.empty(N, ld, device=dev, dtype=torch.float64)
    row = row if row is not None else torch.empty(N, ld, device=dev, dtype=torch.int32)
    vert = vert if vert is not None else torch.empty(N, ld, device=dev, dtype=torch.int32)
    ctx.check(ctx.lib.anet_traj_body_margin_dev(ctx.handle, _ref(_params_of(flatmap)), _ref(body_penalty), int(s), int(N), int(B),
                                                ld, _tptr(coeffs), _tptr(T), _tptr(hpolys), _tptr(margin), _tptr(t), _tptr(row),
                                                _tptr(vert), _stream_of(T, stream)))
    return margin, t, row, vert
