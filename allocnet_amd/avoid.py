"""Trajectory avoidance as a penalty of the MINCO objective: what traj_separation finds, this term removes.  A batch of ego
trajectories is kept min_dist away from listed neighbours of another set of piecewise polynomials -- the other vehicles of a fleet at
a frozen iterate, moving obstacles -- with gradients for the coefficients, the durations and the start time.

All arithmetic runs in the HIP kernel of csrc/avoid_kernels.h behind anet_minco_avoid_partial_grads_dev; the semantics are stated in
include/allocnet_amd.h.  Neighbour lists are in CSR form: (nbr_start int32 [B + 1], nbr int32 [nbr_start[B]]).
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._lib import AvoidPenalty
from .context import default_context

# The other set on the device, batch-minor as the ego: coeffs (N*3*2s, ld), T (N, ld), t0 (B,) or None, N pieces, B trajectories.
AvoidOthers = namedtuple("AvoidOthers", "coeffs T t0 N B")


def _tptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ref(struct):
    return ctypes.cast(ctypes.pointer(struct), ctypes.c_void_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _stream_of(t, stream):
    import torch
    return ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(t.device).cuda_stream)


def make_avoid_penalty(w=100.0, smooth_mu=1e-2, min_dist=0.6, z_scale=1.0, res=20):
    """struct anet_avoid_penalty: weight, smoothedL1 mu (m^2), the distance to keep (m), the vertical stretch of the keep-out
    (1: a sphere, > 1: taller, for downwash) and the samples per ego piece."""
    return AvoidPenalty(float(w), float(smooth_mu), float(min_dist), float(z_scale), int(res))


# ---------------------------------------------------------------------------------------------
# neighbour lists
# ---------------------------------------------------------------------------------------------
def _csr(rows, cols, B):
    order = np.lexsort((cols, rows))
    start = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=B), out=start[1:])
    return start, np.ascontiguousarray(cols[order], dtype=np.int32)


def neighbours_all(B, Bo, exclude_self=False):
    """Every one of the Bo others as a neighbour of each of the B egos, ascending; exclude_self leaves b out of its own list (the
    sets alias).  Returns (nbr_start, nbr)."""
    rows, cols = np.divmod(np.arange(B * Bo, dtype=np.int64), Bo)
    if exclude_self:
        keep = rows != cols
        rows, cols = rows[keep], cols[keep]
    return _csr(rows, cols, B)


def neighbours_from_pairs(pairs, B, keep=None):
    """The lists of a fleet checked against itself, from the pairs traj_separation returns: both directions of every kept pair
    (keep: a boolean mask over the pairs, e.g. sep < radius; None keeps all), each list ascending and without repeats, never b in
    its own list.  Returns (nbr_start, nbr)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if keep is not None:
        pairs = pairs[np.asarray(keep, dtype=bool)]
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    if pairs.size and (pairs.min() < 0 or pairs.max() >= B):
        raise ValueError("pair index outside [0, B)")
    both = np.unique(np.concatenate([pairs, pairs[:, ::-1]]), axis=0) if pairs.size else pairs
    return _csr(both[:, 0], both[:, 1], B)


def _nbr_dev(nbr, dev):
    """(nbr_start, nbr) as int32 device tensors; an empty list array still gets an address."""
    import torch
    start, lst = nbr
    as_dev = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
    start, lst = as_dev(start).to(dev), as_dev(lst).to(dev)
    if start.dtype != torch.int32 or lst.dtype != torch.int32:
        raise ValueError("neighbour lists must be int32")
    if lst.numel() == 0:
        lst = torch.zeros(1, dtype=torch.int32, device=dev)
    return start.contiguous(), lst.contiguous()


# ---------------------------------------------------------------------------------------------
# the penalty
# ---------------------------------------------------------------------------------------------
def minco_avoid_partial_grads_dev(avoid_penalty, s, N, B, coeffs, T, others, nbr, gdC, gdT, piece_cost=None, gd_t0=None, t0=None,
                                  accumulate=False, stream=None, ctx=None):
    """anet_minco_avoid_partial_grads_dev on batch-minor torch CUDA float64 tensors: the ego with the row stride of T, `others` an
    AvoidOthers with the row stride of its T, nbr = (nbr_start, nbr) int32 device tensors."""
    ctx = ctx or default_context(T.device.index or 0)
    start, lst = _nbr_dev(nbr, T.device)
    if start.numel() != B + 1:
        raise ValueError("nbr_start must hold B + 1 entries")
    ctx.check(ctx.lib.anet_minco_avoid_partial_grads_dev(
        ctx.handle, _ref(avoid_penalty), int(s), int(N), int(B), T.stride(0), _tptr(coeffs), _tptr(T), _tptr(t0), int(others.N),
        int(others.B), others.T.stride(0), _tptr(others.coeffs), _tptr(others.T), _tptr(others.t0), _tptr(start), _tptr(lst),
        1 if accumulate else 0, _tptr(gdC), _tptr(gdT), _tptr(piece_cost), _tptr(gd_t0), _stream_of(T, stream)))
    return gdC, gdT, piece_cost, gd_t0


def minco_avoid_cost_grad_dev(head, tail, wps, T, s, c, N, B, others, avoid_penalty, nbr, t0=None, hpolys=None, penalty=None,
                              stream=None, ctx=None):
    """J = int (p^(s))^2 + rho sum T + J_pen + J_avoid and its gradient, composed at the C ABI as minco_flat_cost_grad_dev is:
    anet_minco_solve_dev -> anet_minco_partial_grads_dev -> anet_minco_avoid_partial_grads_dev(accumulate = 1) ->
    anet_minco_propagate_grad_dev.  Batch-minor torch CUDA float64 tensors with a common row stride; t0 (B,) or None.
    Returns cost (ld,), gradP (max(3 (N-1), 1), ld), gradT (N, ld), grad_t0 (ld,), coeffs (N*3*2s, ld)."""
    import torch
    from .minco import minco_solve_dev
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    st = _stream_of(T, stream)
    nbr = _nbr_dev(nbr, dev)
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
    zeros = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float64)
    coeffs, energy = new(N * 3 * 2 * s, ld), new(ld)
    minco_solve_dev(head, tail, wps, T, s, c, N, B, coeffs=coeffs, energy=energy, stream=st.value, ctx=ctx)
    gdC, gdT, pc, gt0 = new(N * 3 * 2 * s, ld), new(N, ld), zeros(N, ld), zeros(ld)
    ctx.check(ctx.lib.anet_minco_partial_grads_dev(ctx.handle, s, N, B, ld, _tptr(coeffs), _tptr(T), _tptr(hpolys),
                                                   _ref(penalty) if penalty is not None else None, 1, _tptr(gdC), _tptr(gdT),
                                                   _tptr(pc), st))
    minco_avoid_partial_grads_dev(avoid_penalty, s, N, B, coeffs, T, others, nbr, gdC, gdT, pc, gt0, t0=t0, accumulate=True,
                                  stream=st.value, ctx=ctx)
    gradP, gradT = zeros(max(3 * (N - 1), 1), ld), new(N, ld)
    ctx.check(ctx.lib.anet_minco_propagate_grad_dev(ctx.handle, s, c, N, B, ld, _tptr(T), _tptr(coeffs), _tptr(gdC), _tptr(gdT),
                                                    _tptr(gradP), _tptr(gradT), st))
    # the adjoint kernel is given no cost to assemble here: the sum of the terms and rho's share of the time gradient
    rho = penalty.rho if penalty is not None else 0.0
    cost = energy + rho * T.sum(0) + pc.sum(0)
    if rho != 0.0:
        gradT = gradT + rho
    return cost, gradP, gradT, gt0, coeffs


def upload_others(o_coeffs, o_T, o_t0=None, ctx=None):
    """Trajectory-major numpy others -- o_coeffs (Bo, No, 3, 2s), o_T (Bo, No), o_t0 (Bo,) or None -- as an AvoidOthers on the
    context's device."""
    import torch
    ctx = ctx or default_context()
    o_coeffs, o_T = _f64(o_coeffs), _f64(o_T)
    Bo, No = o_T.shape
    if o_coeffs.shape[:3] != (Bo, No, 3):
        raise ValueError("o_coeffs must be (Bo, No, 3, 2s)")
    dev = torch.device("cuda", ctx.device)
    ld = int(ctx.lib.anet_recommended_ld(Bo)) if Bo > 1 else 1
    d_co = torch.zeros(o_coeffs[0].size, ld, device=dev, dtype=torch.float64)
    d_co[:, :Bo] = torch.from_numpy(o_coeffs.reshape(Bo, -1)).to(dev).T
    d_T = torch.zeros(No, ld, device=dev, dtype=torch.float64)
    d_T[:, :Bo] = torch.from_numpy(o_T).to(dev).T
    d_t0 = torch.from_numpy(_f64(o_t0, (Bo,))).to(dev) if o_t0 is not None else None
    return AvoidOthers(d_co, d_T, d_t0, No, Bo)


def minco_avoid_cost_grad(head, tail, wps, T, s, others, avoid_penalty, nbr, t0=None, hpolys=None, penalty=None, ctx=None):
    """Host (numpy, trajectory-major) form of minco_avoid_cost_grad_dev, with minco_flat_cost_grad's shapes: head, tail (B, 3, c);
    wps (B, N-1, 3); T (B, N); t0 (B,) or None; hpolys (B, N, M, 4); others = (o_coeffs (Bo, No, 3, 2s), o_T (Bo, No), o_t0 (Bo,) or
    None) or an AvoidOthers already on the device; nbr = (nbr_start, nbr).
    Returns cost (B,), gradP (B, N-1, 3), gradT (B, N), grad_t0 (B,)."""
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
    if not isinstance(others, AvoidOthers):
        others = upload_others(*others, ctx=ctx)

    def up(a):     # (B, fields) -> batch-minor (fields, ld)
        t = torch.zeros(max(a.shape[1], 1), ld, device=dev, dtype=torch.float64)
        if a.shape[1]:
            t[:a.shape[1], :B] = torch.from_numpy(a).to(dev).T
        return t
    d_T = up(T)
    d_T[:, B:] = 1.0
    d_t0 = torch.from_numpy(_f64(t0, (B,))).to(dev) if t0 is not None else None
    d_hp = None
    if hpolys is not None:
        hpolys = _f64(hpolys)
        if penalty is None or hpolys.shape != (B, N, penalty.poly_rows, 4):
            raise ValueError("hpolys must be (B, N, penalty.poly_rows, 4)")
        d_hp = up(hpolys.reshape(B, -1))
    cost, gP, gT, g0, _ = minco_avoid_cost_grad_dev(up(head.reshape(B, -1)), up(tail.reshape(B, -1)), up(wps.reshape(B, -1)), d_T, s,
                                                    c, N, B, others, avoid_penalty, nbr, t0=d_t0, hpolys=d_hp, penalty=penalty,
                                                    ctx=ctx)
    gradP = gP[:3 * (N - 1), :B].T.contiguous().cpu().numpy().reshape(B, N - 1, 3)
    return cost[:B].cpu().numpy(), gradP, gT[:, :B].T.contiguous().cpu().numpy(), g0[:B].cpu().numpy()


def avoid_objective_dev(head, tail, s, c, N, B, others, avoid_penalty, nbr, t0=None, hpolys=None, penalty=None, ctx=None):
    """The composed objective as an `evaluate(x, f, g)` of lbfgs_optimize_dev, the others frozen: x (3 (N-1) + N, ld) holds the
    waypoints (the rows of minco_cost_grad_dev's wps) and below them the LOG durations, so that every duration stays positive;
    g is the gradient w.r.t. x (dJ/dlog T = T dJ/dT).  One round of a fleet's deconfliction is one lbfgs_optimize_dev run on this
    with `others` the fleet at the previous iterate."""
    import torch
    nw = 3 * (N - 1)
    nbr = _nbr_dev(nbr, head.device)

    def evaluate(x, f, g):
        T = torch.exp(x[nw:nw + N])
        wps = x[:nw] if nw else torch.zeros(1, x.shape[1], device=x.device, dtype=torch.float64)
        cost, gP, gT, _, _ = minco_avoid_cost_grad_dev(head, tail, wps, T, s, c, N, B, others, avoid_penalty, nbr, t0=t0,
                                                       hpolys=hpolys, penalty=penalty, ctx=ctx)
        f.copy_(cost)
        if nw:
            g[:nw].copy_(gP[:nw])
        g[nw:nw + N].copy_(gT * T)
    return evaluate
