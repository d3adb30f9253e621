"""Host mirror of the reference's Piece<D> / Trajectory<D> containers
(src/planner/include/gcopter/trajectory.hpp:37-645) and of network/utils/trajectory.py.

Structure (durations, coefficient matrices, junctions) is host bookkeeping, exactly like the
reference; everything that evaluates polynomials or the control-effort cost runs in the HIP
kernels through anet_traj_eval / anet_traj_cost.  A Trajectory here may hold one trajectory
(reference semantics) -- batches go through `traj_eval` / `traj_cost` directly.
"""
import ctypes
import numpy as np

from .context import default_context


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def traj_eval(coeffs, T, tq, deriv, ctx=None):
    """coeffs (B,N,3,D), T (B,N), tq (B,nq) absolute times -> (B,nq,3)."""
    ctx = ctx or default_context()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    tq = np.ascontiguousarray(tq, dtype=np.float64)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N) or tq.shape[0] != B:
        raise ValueError("shape mismatch")
    nq = tq.shape[1]
    out = np.empty((B, nq, 3))
    ctx.check(ctx.lib.anet_traj_eval(ctx.handle, D // 2, N, B, _ptr(coeffs), _ptr(T), nq, _ptr(tq),
                                     int(deriv), _ptr(out)))
    return out


def traj_cost(coeffs, T, order=None, m34=1400.0, ctx=None):
    """Trajectory::getTrajCost batched: coeffs (B,N,3,D), T (B,N) -> (B,)."""
    ctx = ctx or default_context()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    B, N, _, D = coeffs.shape
    s = D // 2
    if order is not None and order != s:
        raise ValueError("order must be D/2 (3 for degree 5, 4 for degree 7)")
    out = np.empty(B)
    ctx.check(ctx.lib.anet_traj_cost(ctx.handle, s, N, B, _ptr(coeffs), _ptr(T), float(m34), _ptr(out)))
    return out


def traj_cost_grad_T(coeffs, T, m34=1400.0, ctx=None):
    """d getTrajCost / dT at fixed coefficients, (B,N): the time gradient the reference's training
    propagates (layers.py:143-147 with the QP solution detached, :121)."""
    ctx = ctx or default_context()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    B, N, _, D = coeffs.shape
    out = np.empty((B, N))
    ctx.check(ctx.lib.anet_traj_cost_grad_T(ctx.handle, D // 2, N, B, _ptr(coeffs), _ptr(T), float(m34), _ptr(out)))
    return out


def traj_max_rate(coeffs, T, which, ctx=None):
    """Per-piece maximum of ||v|| (which=1) or ||a|| (which=2): Piece::getMaxVelRate/getMaxAccRate batched.
    coeffs (B,N,3,D), T (B,N) -> (B,N)."""
    ctx = ctx or default_context()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    B, N, _, D = coeffs.shape
    out = np.empty((B, N))
    ctx.check(ctx.lib.anet_traj_max_rate(ctx.handle, D // 2, N, B, _ptr(coeffs), _ptr(T), int(which), _ptr(out)))
    return out


def traj_row_margin(coeffs, T, rows, deriv=0, ctx=None):
    """Exact per-piece margin against linear rows a.x <= b (anet_traj_row_margin): the maximum over the non-padding rows of a
    piece and over t in [0, T_i] of a . p^(deriv)(t) - b.  Positive: the deepest excursion; negative: the clearance kept; -inf:
    no row; NaN: a non-finite input of that piece.  coeffs (B,N,3,D), T (B,N), rows (B,N,M,4) with all-zero rows as padding ->
    (margin (B,N), row (B,N) int32: a maximising row or -1, t (B,N): its local time)."""
    ctx = ctx or default_context()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N) or rows.ndim != 4 or rows.shape[:2] != (B, N) or rows.shape[3] != 4:
        raise ValueError("shape mismatch")
    M = rows.shape[2]
    margin = np.empty((B, N))
    row = np.empty((B, N), dtype=np.int32)
    t = np.empty((B, N))
    ctx.check(ctx.lib.anet_traj_row_margin(ctx.handle, D // 2, N, B, _ptr(coeffs), _ptr(T), int(deriv), M, _ptr(rows),
                                           _ptr(margin), _ptr(row), _ptr(t)))
    return margin, row, t


def box_rows(limit):
    """The six rows +-e_axis . x <= limit of the per-axis boxes of QPSolver::solve (qp_solver.hpp:268-296), (6, 4)."""
    r = np.zeros((6, 4))
    for ax in range(3):
        r[2 * ax, ax] = 1.0
        r[2 * ax + 1, ax] = -1.0
    r[:, 3] = float(limit)
    return r


def traj_qp_margins(coeffs, T, hpolys, max_vel, max_acc, ctx=None):
    """The exact margins of the three inequality groups QPSolver::solve samples: corridor rows on the position, +-v_axis <=
    max_vel, +-a_axis <= max_acc.  hpolys (B,N,M,4) -> (corridor, vel_box, acc_box), each (B,N)."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    B, N = coeffs.shape[:2]
    corridor = traj_row_margin(coeffs, T, hpolys, 0, ctx=ctx)[0]
    vel = traj_row_margin(coeffs, T, np.broadcast_to(box_rows(max_vel), (B, N, 6, 4)), 1, ctx=ctx)[0]
    acc = traj_row_margin(coeffs, T, np.broadcast_to(box_rows(max_acc), (B, N, 6, 4)), 2, ctx=ctx)[0]
    return corridor, vel, acc


def _stack_hpolys(hPolys):
    """A list of (M_i, 4) polytopes -> (1, N, max M_i, 4), padded with zero rows."""
    hp = [np.asarray(h, dtype=np.float64).reshape(-1, 4) for h in hPolys]
    M = max(1, max(h.shape[0] for h in hp))
    out = np.zeros((1, len(hp), M, 4))
    for i, h in enumerate(hp):
        out[0, i, :h.shape[0]] = h
    return out


HIT_FREE, HIT_OUTSIDE, HIT_INVALID = -1, -2, -3


def traj_voxel_hit(coeffs, T, vm, ctx=None):
    """Exact first collision of every piece with the VoxelMap vm (anet_traj_voxel_hit): t_hit = inf{t in [0, T_i]: vm.query(p_i(t))},
    +inf for a free piece, NaN for a piece with a non-finite input or a negative duration.  coeffs (B,N,3,D), T (B,N) ->
    (t_hit (B,N), voxel (B,N) int32: the linear index x + sx (y + sy z) of the blocked voxel entered, HIT_FREE, HIT_OUTSIDE when
    the curve left the map, HIT_INVALID; HIT_INVALID with a finite t_hit: undecided from t_hit on, treat as a hit)."""
    import torch
    ctx = ctx or vm.ctx
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N):
        raise ValueError("shape mismatch")
    t_hit = np.empty((B, N))
    voxel = np.empty((B, N), dtype=np.int32)
    torch.cuda.current_stream(vm.device).synchronize()      # the map's fills and dilations run there, the call on the context's stream
    ctx.check(ctx.lib.anet_traj_voxel_hit(ctx.handle, D // 2, N, B, _ptr(coeffs), _ptr(T), ctypes.byref(vm._grid),
                                          ctypes.c_void_p(vm.voxels_dev.data_ptr()), _ptr(t_hit), _ptr(voxel)))
    return t_hit, voxel


def traj_voxel_hit_dev(coeffs, T, vm, s, n_pieces, batch, t_hit=None, voxel=None, ctx=None):
    """anet_traj_voxel_hit_dev on batch-minor CUDA tensors, asynchronous on torch's current stream: coeffs (N*3*2s, ld), T (N, ld)
    float64 -> (t_hit (N, ld) float64, voxel (N, ld) int32); columns from `batch` on are not touched.  voxel=False: not wanted."""
    import torch
    ctx = ctx or vm.ctx
    ld = int(T.shape[1])
    if coeffs.dtype != torch.float64 or T.dtype != torch.float64 or not (coeffs.is_contiguous() and T.is_contiguous()):
        raise ValueError("traj_voxel_hit_dev: contiguous float64 tensors expected")
    if tuple(coeffs.shape) != (n_pieces * 6 * s, ld) or T.shape[0] != n_pieces:
        raise ValueError("shape mismatch")
    if t_hit is None:
        t_hit = torch.empty((n_pieces, ld), dtype=torch.float64, device=T.device)
    if voxel is None:
        voxel = torch.empty((n_pieces, ld), dtype=torch.int32, device=T.device)
    for out, dt in ((t_hit, torch.float64), (voxel, torch.int32)):
        if out is not False and (out.dtype != dt or tuple(out.shape) != (n_pieces, ld) or not out.is_contiguous()):
            raise ValueError("traj_voxel_hit_dev: outputs are contiguous (N, ld) tensors, float64 and int32")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(T.device).cuda_stream)
    ctx.check(ctx.lib.anet_traj_voxel_hit_dev(ctx.handle, int(s), int(n_pieces), int(batch), ld, p(coeffs), p(T),
                                              ctypes.byref(vm._grid), p(vm.voxels_dev), p(t_hit),
                                              None if voxel is False else p(voxel), stream))
    return t_hit, (None if voxel is False else voxel)


def first_collision_of(t_hit, voxel, T):
    """The per-piece answers of traj_voxel_hit -> per trajectory (t (B,) global time, piece (B,) int32, voxel (B,) int32): the
    first piece whose t_hit is not +inf (a NaN piece counts: nothing is known from its start on); free: (inf, -1, HIT_FREE)."""
    t_hit = np.asarray(t_hit, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    B, N = t_hit.shape
    start = np.concatenate([np.zeros((B, 1)), np.cumsum(T, axis=1)[:, :-1]], axis=1)
    found = ~(t_hit == np.inf)
    piece = np.where(found.any(axis=1), found.argmax(axis=1), -1).astype(np.int32)
    rows, col = np.arange(B), np.maximum(piece, 0)
    t = np.where(piece >= 0, start[rows, col] + t_hit[rows, col], np.inf)
    vox = np.where(piece >= 0, np.asarray(voxel)[rows, col], HIT_FREE).astype(np.int32)
    return t, piece, vox


def traj_first_collision(coeffs, T, vm, ctx=None):
    """First collision of every trajectory with the VoxelMap vm: (t (B,): global time, the earlier durations plus t_hit; piece (B,)
    int32; voxel (B,) int32 as in traj_voxel_hit).  A free trajectory has t = inf, piece = -1, voxel = HIT_FREE."""
    t_hit, voxel = traj_voxel_hit(coeffs, T, vm, ctx=ctx)
    return first_collision_of(t_hit, voxel, T)


def _is_voxel_map(x):
    return hasattr(x, "surf_points_dev") and hasattr(x, "voxels_dev")


def traj_clearance(coeffs, T, points, counts=None, ctx=None):
    """Exact per-piece clearance to obstacle points (anet_traj_clearance): the minimum over the finite points q of a piece's set
    and over t in [0, T_i] of ||p_i(t) - q||, metres; +inf: no finite point; NaN: a non-finite input of that piece or T_i < 0.
    coeffs (B,N,3,D), T (B,N); points (P,3): one cloud shared by every piece, or (N,Pmax,3): piece i against points[i] (the
    output of VoxelMap.gather_boxes), numpy or a CUDA tensor; a VoxelMap stands for its surface points.  counts: the number of
    points of each set, (N,) or a scalar for a shared cloud, clamped to the set's rows; None: all of them.
    -> (clearance (B,N), point (B,N) int32: a minimising point's index in its set or -1, t (B,N): its local time)."""
    if _is_voxel_map(points):
        ctx = ctx or points.ctx
        points = points.surf_points_dev()
    ctx = ctx or default_context()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N) or D not in (4, 6, 8):
        raise ValueError("shape mismatch")
    if not isinstance(points, np.ndarray) and hasattr(points, "is_cuda"):
        import torch
        if not points.is_cuda:
            points = points.numpy()
        else:       # the cloud stays where it is: the batch goes to the device instead
            dev = points.device
            co = torch.from_numpy(coeffs.reshape(B, N * 3 * D).T.copy()).to(dev)
            Td = torch.from_numpy(T.T.copy()).to(dev)
            if counts is not None and not isinstance(counts, torch.Tensor):
                counts = torch.from_numpy(np.atleast_1d(np.asarray(counts, dtype=np.int32))).to(dev)
            c, p, t = traj_clearance_dev(co, Td, points, D // 2, N, B, counts=counts, ctx=ctx)
            return c.cpu().numpy().T.copy(), p.cpu().numpy().T.copy(), t.cpu().numpy().T.copy()
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.ndim == 2 and points.shape[1] == 3:
        n_sets, pmax = 1, points.shape[0]
    elif points.ndim == 3 and points.shape[0] == N and points.shape[2] == 3:
        n_sets, pmax = N, points.shape[1]
    else:
        raise ValueError("points: (P, 3) or (N, Pmax, 3)")
    if counts is not None:
        counts = np.ascontiguousarray(np.atleast_1d(counts), dtype=np.int32)
        if counts.shape != (n_sets,):
            raise ValueError("counts: one per set")
    clearance = np.empty((B, N))
    point = np.empty((B, N), dtype=np.int32)
    t = np.empty((B, N))
    ctx.check(ctx.lib.anet_traj_clearance(ctx.handle, D // 2, N, B, _ptr(coeffs), _ptr(T), n_sets, pmax, _ptr(points),
                                          None if counts is None else _ptr(counts), _ptr(clearance), _ptr(point), _ptr(t)))
    return clearance, point, t


def traj_clearance_dev(coeffs, T, points, s, n_pieces, batch, counts=None, clearance=None, point=None, t=None, ctx=None):
    """anet_traj_clearance_dev on batch-minor CUDA tensors, asynchronous on torch's current stream: coeffs (N*3*2s, ld), T (N, ld)
    float64; points (P, 3) or (N, Pmax, 3) float64 CUDA (or a VoxelMap: its surface points), counts (n_sets,) int32 CUDA or None
    -> (clearance (N, ld) float64, point (N, ld) int32, t (N, ld) float64); columns from `batch` on are not touched.
    point=False / t=False: not wanted."""
    import torch
    if _is_voxel_map(points):
        ctx = ctx or points.ctx
        points = points.surf_points_dev()
    ctx = ctx or default_context()
    ld = int(T.shape[1])
    if coeffs.dtype != torch.float64 or T.dtype != torch.float64 or not (coeffs.is_contiguous() and T.is_contiguous()):
        raise ValueError("traj_clearance_dev: contiguous float64 tensors expected")
    if tuple(coeffs.shape) != (n_pieces * 6 * s, ld) or T.shape[0] != n_pieces:
        raise ValueError("shape mismatch")
    if points.dtype != torch.float64 or not points.is_cuda or not points.is_contiguous():
        raise ValueError("traj_clearance_dev: points is a contiguous float64 CUDA tensor")
    if points.dim() == 2 and points.shape[1] == 3:
        n_sets, pmax = 1, int(points.shape[0])
    elif points.dim() == 3 and points.shape[0] == n_pieces and points.shape[2] == 3:
        n_sets, pmax = int(n_pieces), int(points.shape[1])
    else:
        raise ValueError("points: (P, 3) or (N, Pmax, 3)")
    if counts is not None and (counts.dtype != torch.int32 or not counts.is_cuda or counts.numel() != n_sets or not counts.is_contiguous()):
        raise ValueError("traj_clearance_dev: counts is a contiguous int32 CUDA tensor, one per set")
    if clearance is None:
        clearance = torch.empty((n_pieces, ld), dtype=torch.float64, device=T.device)
    if point is None:
        point = torch.empty((n_pieces, ld), dtype=torch.int32, device=T.device)
    if t is None:
        t = torch.empty((n_pieces, ld), dtype=torch.float64, device=T.device)
    for out, dt in ((clearance, torch.float64), (point, torch.int32), (t, torch.float64)):
        if out is not False and (out.dtype != dt or tuple(out.shape) != (n_pieces, ld) or not out.is_contiguous()):
            raise ValueError("traj_clearance_dev: outputs are contiguous (N, ld) tensors, float64 / int32 / float64")
    if clearance is False:
        raise ValueError("traj_clearance_dev: clearance is always written")
    p = lambda x: None if (x is None or x is False) else ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(T.device).cuda_stream)
    ctx.check(ctx.lib.anet_traj_clearance_dev(ctx.handle, int(s), int(n_pieces), int(batch), ld, p(coeffs), p(T), n_sets, pmax,
                                              p(points) if pmax else None, p(counts), p(clearance), p(point), p(t), stream))
    return clearance, (None if point is False else point), (None if t is False else t)


def clearance_of(clearance, point, t, T):
    """The per-piece answers of traj_clearance -> per trajectory (clearance (B,), t (B,) global time, piece (B,) int32, point
    (B,) int32): the piece with the smallest clearance.  A NaN piece makes the trajectory's clearance NaN (nothing is known
    about that piece) and is the piece named; no finite point anywhere: (inf, 0, -1, -1)."""
    clearance = np.asarray(clearance, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    B, N = clearance.shape
    start = np.concatenate([np.zeros((B, 1)), np.cumsum(T, axis=1)[:, :-1]], axis=1)
    bad = np.isnan(clearance)
    piece = np.where(bad.any(axis=1), bad.argmax(axis=1), np.where(bad, np.inf, clearance).argmin(axis=1)).astype(np.int32)
    rows = np.arange(B)
    c = clearance[rows, piece]
    none = c == np.inf
    pt = np.where(none, -1, np.asarray(point)[rows, piece]).astype(np.int32)
    tt = np.where(none | np.isnan(c), 0.0, start[rows, piece] + np.asarray(t)[rows, piece])
    return c, tt, np.where(none, -1, piece).astype(np.int32), pt


def clearance_at_least(clearance, min_dist):
    """True when every clearance is >= min_dist; a NaN is False"""
    return bool(np.all(np.asarray(clearance, dtype=np.float64) >= float(min_dist)))


def all_pairs(B):
    """every (a, b) with a < b < B, sorted by a: (P, 2) int32 -- the order in which anet_traj_separation reads fastest"""
    a, b = np.triu_indices(int(B), 1)
    return np.stack([a, b], axis=1).astype(np.int32)


def traj_separation(coeffs, T, pairs=None, t0=None, cutoff=np.inf, ctx=None):
    """Exact minimum separation between pairs of trajectories of one batch (anet_traj_separation), metres: the minimum over the
    time both trajectories of a pair exist of ||p_a(t) - p_b(t)||, found between the samples, not on them.
    coeffs (B,N,3,D), T (B,N); t0 (B,): global start times (None: 0); pairs (P,2) int: indices into the batch (None: every a < b,
    sorted by a).  Knots are the float64 sums t0 + T_0 + ... in piece order; a piece of zero duration occupies no time (padding).
    cutoff: a separation at or above it need not be refined (it is still an actual distance of the two curves, never below the
    exact minimum); inf: off.  Holding position before the start or after the end is not a mode: prepend or append a constant
    piece of the wanted duration.
    -> (sep (P,), t (P,) global time of a minimum, pieces (P,2) int32, pairs (P,2) int32).  No common time: (inf, 0, -1, -1); a
    non-finite or negative duration, a non-finite t0, or a non-finite coefficient in a piece that is used: (nan, 0, -1, -1) for
    that pair only.  An index outside [0, B) raises AnetError."""
    ctx = ctx or default_context()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N) or D not in (4, 6, 8):
        raise ValueError("shape mismatch")
    if t0 is not None:
        t0 = np.ascontiguousarray(t0, dtype=np.float64)
        if t0.shape != (B,):
            raise ValueError("t0: one start time per trajectory")
    pairs = all_pairs(B) if pairs is None else np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError("pairs: (P, 2) integers")
    if pairs.size and (pairs.min() < -2 ** 31 or pairs.max() >= 2 ** 31):
        raise ValueError("pairs: indices must fit int32")
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    P = pairs.shape[0]
    pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    sep = np.empty(P)
    t = np.empty(P)
    qa, qb = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32)
    ctx.check(ctx.lib.anet_traj_separation(ctx.handle, D // 2, N, B, _ptr(coeffs), _ptr(T), None if t0 is None else _ptr(t0), P,
                                           _ptr(pa), _ptr(pb), float(cutoff), _ptr(sep), _ptr(t), _ptr(qa), _ptr(qb)))
    return sep, t, np.stack([qa, qb], axis=1), pairs


def traj_separation_dev(coeffs, T, pair_a, pair_b, s, n_pieces, batch, t0=None, cutoff=np.inf, sep=None, t=None, piece_a=None,
                        piece_b=None, ctx=None):
    """anet_traj_separation_dev on CUDA tensors, asynchronous on torch's current stream: coeffs (N*3*2s, ld), T (N, ld) float64
    batch-minor; t0 (>= batch,) float64 or None; pair_a, pair_b (P,) int32 -> (sep (P,) float64, t (P,) float64, piece_a (P,)
    int32, piece_b (P,) int32).  Caller-supplied outputs may be longer than P: elements from P on are not touched.  t=False /
    piece_a=False / piece_b=False: not wanted.  A pair with an index outside [0, batch) gets (nan, 0, -1, -1)."""
    import torch
    ctx = ctx or default_context()
    ld = int(T.shape[1])
    if coeffs.dtype != torch.float64 or T.dtype != torch.float64 or not (coeffs.is_contiguous() and T.is_contiguous()):
        raise ValueError("traj_separation_dev: contiguous float64 tensors expected")
    if tuple(coeffs.shape) != (n_pieces * 6 * s, ld) or T.shape[0] != n_pieces:
        raise ValueError("shape mismatch")
    if t0 is not None and (t0.dtype != torch.float64 or not t0.is_cuda or not t0.is_contiguous() or t0.dim() != 1 or t0.numel() < batch):
        raise ValueError("traj_separation_dev: t0 is a contiguous float64 CUDA tensor, one per trajectory")
    P = int(pair_a.numel())
    for x in (pair_a, pair_b):
        if x.dtype != torch.int32 or not x.is_cuda or not x.is_contiguous() or x.dim() != 1 or x.numel() != P:
            raise ValueError("traj_separation_dev: pair_a, pair_b are contiguous int32 CUDA tensors of one length")
    if sep is None:
        sep = torch.empty(P, dtype=torch.float64, device=T.device)
    if t is None:
        t = torch.empty(P, dtype=torch.float64, device=T.device)
    if piece_a is None:
        piece_a = torch.empty(P, dtype=torch.int32, device=T.device)
    if piece_b is None:
        piece_b = torch.empty(P, dtype=torch.int32, device=T.device)
    for out, dt in ((sep, torch.float64), (t, torch.float64), (piece_a, torch.int32), (piece_b, torch.int32)):
        if out is not False and (out.dtype != dt or out.dim() != 1 or out.numel() < P or not out.is_contiguous() or not out.is_cuda):
            raise ValueError("traj_separation_dev: outputs are contiguous CUDA vectors of at least P elements, float64 / int32")
    if sep is False:
        raise ValueError("traj_separation_dev: sep is always written")
    p = lambda x: None if (x is None or x is False) else ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(T.device).cuda_stream)
    ctx.check(ctx.lib.anet_traj_separation_dev(ctx.handle, int(s), int(n_pieces), int(batch), ld, p(coeffs), p(T), p(t0), P, p(pair_a),
                                               p(pair_b), float(cutoff), p(sep), p(t), p(piece_a), p(piece_b), stream))
    return sep, (None if t is False else t), (None if piece_a is False else piece_a), (None if piece_b is False else piece_b)


def separation_at_least(sep, min_dist):
    """True when every separation is >= min_dist; a NaN is False; +inf (no common time) is clear"""
    return bool(np.all(np.asarray(sep, dtype=np.float64) >= float(min_dist)))


def piece_normalized_coeffs(coeffs, T, deriv, ctx=None):
    """Piece::normalizePosCoeffMat / normalizeVelCoeffMat / normalizeAccCoeffMat (trajectory.hpp:135-171) for a batch of pieces:
    coefficients of position (deriv 0), velocity (1) or acceleration (2) in normalised time.  coeffs (P,3,D), T (P,) -> (P,3,D-deriv)."""
    ctx = ctx or default_context()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    P, _, D = coeffs.shape
    out = np.empty((P, 3, D - int(deriv)))
    ctx.check(ctx.lib.anet_piece_normalized_coeffs(ctx.handle, D // 2, P, _ptr(coeffs), _ptr(T), int(deriv), _ptr(out)))
    return out


class Piece:
    """Piece<D> (trajectory.hpp:37-316): duration + 3 x (D+1) coefficient matrix, highest power first."""

    def __init__(self, dur, cMat, ctx=None):
        self.duration = float(dur)
        self.coeffMat = np.array(cMat, dtype=np.float64)
        if self.coeffMat.ndim != 2 or self.coeffMat.shape[0] != 3:
            raise ValueError("coefficient matrix must be 3 x (D+1)")
        self._ctx = ctx

    def getDim(self):
        return 3

    def getDegree(self):
        return self.coeffMat.shape[1] - 1

    def getDuration(self):
        return self.duration

    def getCoeffMat(self):
        return self.coeffMat

    def _eval(self, t, d):
        # a one-piece trajectory with a huge duration: no piece location involved
        co = self.coeffMat[None, None]
        return traj_eval(co, np.array([[np.inf]]), np.array([[float(t)]]), d, ctx=self._ctx)[0, 0]

    def getPos(self, t):
        return self._eval(t, 0)

    def getVel(self, t):
        return self._eval(t, 1)

    def getAcc(self, t):
        return self._eval(t, 2)

    def getJer(self, t):
        return self._eval(t, 3)

    # trajectory.hpp:135-171
    def normalizePosCoeffMat(self):
        return piece_normalized_coeffs(self.coeffMat[None], np.array([self.duration]), 0, ctx=self._ctx)[0]

    def normalizeVelCoeffMat(self):
        return piece_normalized_coeffs(self.coeffMat[None], np.array([self.duration]), 1, ctx=self._ctx)[0]

    def normalizeAccCoeffMat(self):
        return piece_normalized_coeffs(self.coeffMat[None], np.array([self.duration]), 2, ctx=self._ctx)[0]

    # trajectory.hpp:177-314
    def getMaxVelRate(self):
        return float(traj_max_rate(self.coeffMat[None, None], np.array([[self.duration]]), 1, ctx=self._ctx)[0, 0])

    def getMaxAccRate(self):
        return float(traj_max_rate(self.coeffMat[None, None], np.array([[self.duration]]), 2, ctx=self._ctx)[0, 0])

    def checkMaxVelRate(self, maxVelRate):
        return self.getMaxVelRate() < maxVelRate

    def checkMaxAccRate(self, maxAccRate):
        return self.getMaxAccRate() < maxAccRate

    def getCorridorMargin(self, hPoly):
        """Exact max over the rows a.x <= b of hPoly (M, 4) and over the piece of a . p(t) - b (no counterpart in the reference)."""
        return float(traj_row_margin(self.coeffMat[None, None], np.array([[self.duration]]), _stack_hpolys([hPoly]), 0,
                                     ctx=self._ctx)[0][0, 0])

    def getFirstCollision(self, vm):
        """(t, voxel): the first local time at which the piece is in a blocked voxel of the VoxelMap vm or outside it (inf: never)
        and the voxel's linear index (HIT_FREE, HIT_OUTSIDE, HIT_INVALID); exact, not sampled (no counterpart in the reference)."""
        t, v = traj_voxel_hit(self.coeffMat[None, None], np.array([[self.duration]]), vm, ctx=self._ctx)
        return float(t[0, 0]), int(v[0, 0])

    def getClearance(self, points):
        """(clearance, t, point): the exact smallest distance of the piece to the points (P, 3) (or a VoxelMap's surface), the local
        time at which it is attained and the point's index; (inf, 0, -1) without a finite point (no counterpart in the reference)."""
        c, p, t = traj_clearance(self.coeffMat[None, None], np.array([[self.duration]]), points, ctx=self._ctx)
        return float(c[0, 0]), float(t[0, 0]), int(p[0, 0])

    def checkClearance(self, points, min_dist):
        return clearance_at_least(self.getClearance(points)[0], min_dist)


class Trajectory:
    """Trajectory<D> (trajectory.hpp:317-645)."""

    def __init__(self, durs=None, cMats=None, ctx=None):
        self.pieces = []
        self._ctx = ctx
        if durs is not None:
            for d, c in zip(durs, cMats):       # min(durs.size(), cMats.size()) like the reference
                self.pieces.append(Piece(d, c, ctx))

    # --- container interface --------------------------------------------------------------
    def getPieceNum(self):
        return len(self.pieces)

    def getDurations(self):
        return np.array([p.duration for p in self.pieces])

    def getTotalDuration(self):
        return float(sum(p.duration for p in self.pieces))

    def __getitem__(self, i):
        return self.pieces[i]

    def __iter__(self):
        return iter(self.pieces)

    def clear(self):
        self.pieces.clear()

    def reserve(self, n):
        return None

    def emplace_back(self, *args):
        if len(args) == 1:
            self.pieces.append(args[0])
        else:
            self.pieces.append(Piece(args[0], args[1], self._ctx))

    def append(self, traj):
        self.pieces.extend(traj.pieces)

    def _arrays(self):
        if not self.pieces:
            raise RuntimeError("empty trajectory")
        co = np.stack([p.coeffMat for p in self.pieces])[None]
        return co, self.getDurations()[None]

    # --- evaluation (GPU) -----------------------------------------------------------------
    def _eval(self, t, d):
        co, T = self._arrays()
        t = np.atleast_1d(np.asarray(t, dtype=np.float64))
        out = traj_eval(co, T, t[None], d, ctx=self._ctx)[0]
        return out[0] if out.shape[0] == 1 else out

    def getPos(self, t):
        return self._eval(t, 0)

    def getVel(self, t):
        return self._eval(t, 1)

    def getAcc(self, t):
        return self._eval(t, 2)

    def getJer(self, t):
        return self._eval(t, 3)

    def getTrajCost(self, order, m34=1400.0):
        co, T = self._arrays()
        return float(traj_cost(co, T, order, m34, ctx=self._ctx)[0])

    # --- dynamic feasibility (trajectory.hpp:576-630): maximum over the pieces
    def getMaxVelRate(self):
        co, T = self._arrays()
        return float(traj_max_rate(co, T, 1, ctx=self._ctx).max())

    def getMaxAccRate(self):
        co, T = self._arrays()
        return float(traj_max_rate(co, T, 2, ctx=self._ctx).max())

    def checkMaxVelRate(self, maxVelRate):
        return self.getMaxVelRate() < maxVelRate

    def checkMaxAccRate(self, maxAccRate):
        return self.getMaxAccRate() < maxAccRate

    # --- exact margins against the corridor and the per-axis boxes (no counterpart in the reference, which samples them)
    def getCorridorMargin(self, hPolys, per_piece=False):
        """Maximum over the pieces of the exact corridor margin, piece i against hPolys[i] (rows a.x <= b); per_piece=True: the
        triple (margin, row, t) of arrays over the pieces."""
        co, T = self._arrays()
        if len(hPolys) != len(self.pieces):
            raise ValueError("one polytope per piece")
        m, r, t = traj_row_margin(co, T, _stack_hpolys(hPolys), 0, ctx=self._ctx)
        return (m[0], r[0], t[0]) if per_piece else float(m.max())

    def checkCorridor(self, hPolys, tol=0.0):
        return self.getCorridorMargin(hPolys) <= tol

    def checkBoxLimits(self, max_vel, max_acc):
        """True when every axis of the velocity stays within +-max_vel and of the acceleration within +-max_acc, exactly."""
        co, T = self._arrays()
        shape = (1, len(self.pieces), 6, 4)
        vel = traj_row_margin(co, T, np.broadcast_to(box_rows(max_vel), shape), 1, ctx=self._ctx)[0]
        acc = traj_row_margin(co, T, np.broadcast_to(box_rows(max_acc), shape), 2, ctx=self._ctx)[0]
        return bool(vel.max() <= 0.0 and acc.max() <= 0.0)

    # --- exact first collision with the voxel map (no counterpart in the reference) -----------------------------------
    def getFirstCollision(self, vm, per_piece=False):
        """(t, piece, voxel): the global time of the first collision with the VoxelMap vm (inf: none), its piece (-1) and the
        voxel's linear index (HIT_FREE, HIT_OUTSIDE, HIT_INVALID); per_piece=True: the arrays (t_hit, voxel) over the pieces,
        t_hit in local time."""
        co, T = self._arrays()
        t_hit, voxel = traj_voxel_hit(co, T, vm, ctx=self._ctx)
        if per_piece:
            return t_hit[0], voxel[0]
        t, piece, vox = first_collision_of(t_hit, voxel, T)
        return float(t[0]), int(piece[0]), int(vox[0])

    def checkCollisionFree(self, vm):
        return self.getFirstCollision(vm)[1] < 0

    # --- exact clearance to obstacle points (no counterpart in the reference) ------------------------------------------
    def getClearance(self, points, per_piece=False):
        """(clearance, t, piece, point): the exact smallest distance, in metres, of the trajectory to the points -- (P, 3), one
        cloud for every piece; (N, Pmax, 3), piece i against points[i]; or a VoxelMap, its surface -- the global time at which it
        is attained, its piece and the point's index in its set; (inf, 0, -1, -1) without a finite point.  per_piece=True: the
        arrays (clearance, point, t) over the pieces, t in local time."""
        co, T = self._arrays()
        c, p, t = traj_clearance(co, T, points, ctx=self._ctx)
        if per_piece:
            return c[0], p[0], t[0]
        cc, tt, piece, pt = clearance_of(c, p, t, T)
        return float(cc[0]), float(tt[0]), int(piece[0]), int(pt[0])

    def checkClearance(self, points, min_dist):
        """True when every piece keeps at least min_dist metres from every point, exactly; a NaN clearance is False."""
        return clearance_at_least(self.getClearance(points, per_piece=True)[0], min_dist)

    # --- exact minimum separation to another trajectory (no counterpart in the reference) ---------------------------------
    def _pair_arrays(self, other):
        """both trajectories as one batch of two: the shorter is padded with pieces of zero duration, which occupy no time"""
        if not self.pieces or not other.pieces:
            raise RuntimeError("empty trajectory")
        D = self.pieces[0].coeffMat.shape[1]
        if any(p.coeffMat.shape[1] != D for p in self.pieces + other.pieces):
            raise ValueError("getSeparation: both trajectories must have one order")
        N = max(len(self.pieces), len(other.pieces))
        co = np.zeros((2, N, 3, D))
        T = np.zeros((2, N))
        for r, tr in enumerate((self, other)):
            for i, p in enumerate(tr.pieces):
                co[r, i] = p.coeffMat
                T[r, i] = p.duration
        return co, T

    def getSeparation(self, other, t0=0.0, other_t0=0.0, cutoff=np.inf):
        """(d, t, piece_self, piece_other): the exact smallest distance, in metres, between this trajectory started at global
        time t0 and `other` started at other_t0, over the time both exist; the global time at which it is attained and the two
        pieces.  (inf, 0, -1, -1): no common time.  Holding position before the start or after the end is not a mode: prepend
        or append a constant piece (a coefficient matrix with only its last column set) of the wanted duration."""
        co, T = self._pair_arrays(other)
        sep, t, pieces, _ = traj_separation(co, T, np.array([[0, 1]], dtype=np.int32), np.array([float(t0), float(other_t0)]),
                                            cutoff, ctx=self._ctx)
        return float(sep[0]), float(t[0]), int(pieces[0, 0]), int(pieces[0, 1])

    def checkSeparation(self, other, min_dist, t0=0.0, other_t0=0.0):
        """True when the two trajectories keep at least min_dist metres apart over their common time, exactly; a NaN separation
        is False, no common time is True.  Separations above min_dist are not refined (cutoff just above min_dist)."""
        min_dist = float(min_dist)
        cutoff = max(np.nextafter(min_dist, np.inf), 0.0)
        return separation_at_least(self.getSeparation(other, t0, other_t0, cutoff)[0], min_dist)

    # --- the vehicle's own terms: thrust, attitude, body rate through the flatness map (flatness.py) ---------------
    def getFlatState(self, t, flatmap):
        """What the reference's process() computes at time t (learning_planning.cpp:236-251): getVel/getAcc/getJer pushed
        through flatmap.forward with psi = dpsi = 0.  Returns a dict: thr, quat (4,), omg (3,), speed, tilt, bdr; arrays over
        the queries when t is a sequence."""
        from .flatness import traj_flat_states
        co, T = self._arrays()
        tq = np.atleast_1d(np.asarray(t, dtype=np.float64))
        o = traj_flat_states(flatmap, co, T, tq[None], ctx=self._ctx)[0]
        if np.ndim(t) == 0:
            o = o[0]
        return {"thr": o[..., 0], "quat": o[..., 1:5], "omg": o[..., 5:8], "speed": o[..., 8], "tilt": o[..., 9],
                "bdr": o[..., 10]}

    def getFlatExtrema(self, flatmap, res=20):
        """(min thrust, max thrust, max tilt, max body-rate magnitude) over res + 1 samples of every piece: a sampled check."""
        from .flatness import traj_flat_extrema
        co, T = self._arrays()
        return tuple(float(x) for x in traj_flat_extrema(flatmap, co, T, res, ctx=self._ctx)[0])

    def checkFlatLimits(self, flatmap, min_thrust, max_thrust, max_tilt, max_bdr, res=20):
        """True when the sampled thrust stays inside (min_thrust, max_thrust) and the sampled tilt and body rate below their limits
        (strict, like checkMaxVelRate)."""
        lo, hi, tilt, bdr = self.getFlatExtrema(flatmap, res)
        return lo > min_thrust and hi < max_thrust and tilt < max_tilt and bdr < max_bdr

    # --- the whole body in the corridor: body vertices through the flatness attitude (body.py) ---------------------
    def getBodyMargin(self, flatmap, verts, hPolys, res=20, per_piece=False):
        """Maximum over the pieces of the sampled body margin: a_r . (p(t) + R(q(t)) b_k) - h_r over res + 1 samples of piece i,
        the rows of hPolys[i] and the body vertices verts (K, 3), q(t) the attitude of the flatness map.  A sampled check.
        per_piece=True: the arrays (margin, t, row, vert) over the pieces."""
        from .body import traj_body_margin
        co, T = self._arrays()
        if len(hPolys) != len(self.pieces):
            raise ValueError("one polytope per piece")
        m, t, r, k = traj_body_margin(flatmap, verts, co, T, _stack_hpolys(hPolys), res, ctx=self._ctx)
        return (m[0], t[0], r[0], k[0]) if per_piece else float(m.max())

    def checkBodyCorridor(self, flatmap, verts, hPolys, res=20, tol=0.0):
        """True when every sampled body vertex stays within tol of its piece's polytope; a NaN margin is False."""
        return bool(self.getBodyMargin(flatmap, verts, hPolys, res) <= tol)

    # --- stop within known space: speed against the distance field of the map (stop.py) ------------------------------
    def getStopMargin(self, vm, a_brake, t_react=0.0, clearance=0.0, res=20, per_piece=False):
        """(margin, t, piece): the least d(p) - clearance - t_react |v| - v.v / (2 a_brake) over res + 1 samples of every piece,
        d the distance field of the VoxelMap vm (walls count; on a map made with unknown="blocked" the distance to everything not
        seen to be free), the global time at which it is attained and its piece.  A sampled check.  per_piece=True: the arrays
        (margin, t, speed, dist) over the pieces, t in local time."""
        from .stop import traj_stop_margin
        co, T = self._arrays()
        m, t, sp, d = traj_stop_margin(co, T, vm, a_brake, t_react, clearance, res, ctx=self._ctx)
        if per_piece:
            return m[0], t[0], sp[0], d[0]
        if np.isnan(m[0]).any():
            i = int(np.isnan(m[0]).argmax())
            return float("nan"), float(T[0, :i].sum()), i
        i = int(m[0].argmin())
        return float(m[0, i]), float(T[0, :i].sum() + t[0, i]), i

    def checkStoppable(self, vm, a_brake, t_react=0.0, clearance=0.0, res=20):
        """True when the sampled stop margin is >= 0 on every piece; a NaN margin is False."""
        return bool(self.getStopMargin(vm, a_brake, t_react, clearance, res)[0] >= 0.0)

    # --- yaw: the direction of travel inside the field of view, the yaw rate under its limit (yaw.py) -------------------
    def getYawMargin(self, yaw, half_fov, v_min=0.0, res=20, per_piece=False):
        """(margin, t, piece): the least half_fov - |angle between the horizontal velocity and the heading| over the res + 1
        samples of every piece with |v_xy| >= v_min, the global time at which it is attained and its piece; yaw is a YawTrajectory
        over the same durations.  +inf when no sample moves that fast.  A sampled check.  per_piece=True: the arrays (margin, t,
        rate) over the pieces, t in local time, rate the largest sampled |dpsi|."""
        from .yaw import traj_yaw_margin
        co, T = self._arrays()
        if yaw.getPieceNum() != len(self.pieces) or not np.array_equal(yaw.getDurations(), T[0]):
            raise ValueError("the yaw trajectory must share the pieces and durations")
        m, t, r = traj_yaw_margin(co, yaw.coeffs[None], T, half_fov, v_min, res, ctx=self._ctx)
        if per_piece:
            return m[0], t[0], r[0]
        if np.isnan(m[0]).any():
            i = int(np.isnan(m[0]).argmax())
            return float("nan"), float(T[0, :i].sum()), i
        i = int(m[0].argmin())
        return float(m[0, i]), float(T[0, :i].sum() + t[0, i]), i

    def checkYaw(self, yaw, half_fov, max_rate, v_min=0.0, res=20):
        """True when the sampled look margin is >= 0 on every piece and the sampled |dpsi| stays within max_rate; NaN is False."""
        m, _, r = self.getYawMargin(yaw, half_fov, v_min, res, per_piece=True)
        return bool((m >= 0.0).all() and (r <= max_rate).all())

    # --- junctions (trajectory.hpp:540-574): direct coefficient reads except at the very end
    def getPositions(self):
        N = self.getPieceNum()
        D = self.pieces[0].getDegree()
        pos = np.zeros((3, N + 1))
        for i in range(N):
            pos[:, i] = self.pieces[i].coeffMat[:, D]
        pos[:, N] = self.pieces[-1].getPos(self.pieces[-1].duration)
        return pos

    def getJuncPos(self, j):
        D = self.pieces[0].getDegree()
        if j != self.getPieceNum():
            return self.pieces[j].coeffMat[:, D].copy()
        return self.pieces[j - 1].getPos(self.pieces[j - 1].duration)

    def getJuncVel(self, j):
        D = self.pieces[0].getDegree()
        if j != self.getPieceNum():
            return self.pieces[j].coeffMat[:, D - 1].copy()
        return self.pieces[j - 1].getVel(self.pieces[j - 1].duration)

    def getJuncAcc(self, j):
        D = self.pieces[0].getDegree()
        if j != self.getPieceNum():
            return self.pieces[j].coeffMat[:, D - 2] * 2.0
        return self.pieces[j - 1].getAcc(self.pieces[j - 1].duration)

    def locatePieceIdx(self, t):
        """Returns (idx, local t) -- the reference mutates t in place (trajectory.hpp:496-514)."""
        N = self.getPieceNum()
        idx = 0
        while idx < N and t > self.pieces[idx].duration:
            t -= self.pieces[idx].duration
            idx += 1
        if idx == N:
            idx -= 1
            t += self.pieces[idx].duration
        return idx, t
