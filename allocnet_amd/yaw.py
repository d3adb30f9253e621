"""Yaw trajectories: the heading psi as a second, one-axis minimum-control polynomial over the pieces and durations of the position
trajectory, with an order sy of its own; the penalty that keeps the horizontal direction of travel inside the camera's field of
view and the yaw rate under the platform's limit; the sampled check that goes with it; flat states that use the yaw.  psi is an
unwrapped real number in radians.

All arithmetic runs in the HIP kernels of csrc/yaw_kernels.h behind anet_minco_solve_scalar[_dev],
anet_minco_propagate_grad_scalar_dev, anet_minco_yaw_partial_grads_dev, anet_traj_yaw_margin[_dev] and
anet_traj_states_yaw[_dev]; the semantics are stated in include/allocnet_amd.h.  Device forms take batch-minor torch CUDA
float64 tensors with a common row stride: yaw head / tail (cy, ld), yaw waypoints (N-1, ld), yaw coefficients (N*2sy, ld).
"""
import math

import numpy as np

from ._lib import YawPenalty
from .avoid import _f64, _ref, _stream_of, _tptr
from .context import default_context
from .flatness import FLAT_STATE_FIELDS, _params_of
from .trajectory import _ptr


def make_yaw_penalty(w_look=100.0, mu_look=0.05, half_fov=math.radians(35.0), speed_eps=1e-2, w_rate=100.0, mu_rate=0.05,
                     max_rate=1.0, w_energy=0.0, res=20):
    """struct anet_yaw_penalty: the look term's weight and smoothedL1 mu (m/s), the horizontal half field of view (rad, at most
    pi/2), the smoothing of |v_xy| (m/s), the rate term's weight and mu ((rad/s)^2), the yaw-rate limit (rad/s; inf: none), the
    weight of int (psi^(sy))^2 and the samples per piece."""
    return YawPenalty(float(w_look), float(mu_look), float(half_fov), float(speed_eps), float(w_rate), float(mu_rate),
                      float(max_rate), float(w_energy), int(res))


# ---------------------------------------------------------------------------------------------
# the one-axis MINCO
# ---------------------------------------------------------------------------------------------
def minco_solve_scalar(head, tail, wps, T, s, want_coeffs=True, ctx=None):
    """anet_minco_solve_scalar: head, tail (B, c); wps (B, N-1); T (B, N) numpy -> coeffs (B, N, 2s) [or None], energy (B,)."""
    ctx = ctx or default_context()
    head = _f64(head)
    B, c = head.shape
    tail = _f64(tail, (B, c))
    T = _f64(T)
    N = T.shape[1]
    wps = _f64(wps if wps is not None else np.zeros((B, 0)), (B, N - 1))
    coeffs = np.empty((B, N, 2 * s)) if want_coeffs else None
    energy = np.empty(B)
    ctx.check(ctx.lib.anet_minco_solve_scalar(ctx.handle, int(s), c, N, B, _ptr(head), _ptr(tail), _ptr(wps), _ptr(T), _ptr(coeffs),
                                              _ptr(energy)))
    return coeffs, energy


def minco_solve_scalar_dev(head, tail, wps, T, s, c, N, B, coeffs=None, energy=None, stream=None, ctx=None):
    """anet_minco_solve_scalar_dev: head, tail (c, ld), wps (N-1, ld), T (N, ld) -> coeffs (N*2s, ld), energy (ld,); either output
    is allocated when not given."""
    import torch
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    if coeffs is None:
        coeffs = torch.empty(N * 2 * s, ld, device=dev, dtype=torch.float64)
    if energy is None:
        energy = torch.empty(ld, device=dev, dtype=torch.float64)
    ctx.check(ctx.lib.anet_minco_solve_scalar_dev(ctx.handle, int(s), int(c), int(N), int(B), ld, _tptr(head), _tptr(tail),
                                                  _tptr(wps) if N > 1 else None, _tptr(T), _tptr(coeffs), _tptr(energy),
                                                  _stream_of(T, stream)))
    return coeffs, energy


def minco_propagate_grad_scalar_dev(T, coeffs, gdC, gdT, s, c, N, B, gradP=None, gradT=None, stream=None, ctx=None):
    """anet_minco_propagate_grad_scalar_dev: the adjoint of the one-axis solve.  gdC (N*2s, ld); gdT (N, ld) or None (= zeros: the
    direct share of the durations is added once, on the position side) -> gradP (max(N-1, 1), ld), gradT (N, ld)."""
    import torch
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    if gradP is None:
        gradP = torch.zeros(max(N - 1, 1), ld, device=dev, dtype=torch.float64)
    if gradT is None:
        gradT = torch.empty(N, ld, device=dev, dtype=torch.float64)
    ctx.check(ctx.lib.anet_minco_propagate_grad_scalar_dev(ctx.handle, int(s), int(c), int(N), int(B), ld, _tptr(T), _tptr(coeffs),
                                                           _tptr(gdC), _tptr(gdT), _tptr(gradP), _tptr(gradT), _stream_of(T, stream)))
    return gradP, gradT


# ---------------------------------------------------------------------------------------------
# the penalty and the composed objective
# ---------------------------------------------------------------------------------------------
def minco_yaw_partial_grads_dev(yaw_penalty, s, sy, N, B, coeffs, ycoeffs, T, gdC, gdCy, gdT, piece_cost=None, accumulate=False,
                                stream=None, ctx=None):
    """anet_minco_yaw_partial_grads_dev.  `accumulate` governs gdC, gdT and piece_cost; gdCy is always overwritten."""
    ctx = ctx or default_context(T.device.index or 0)
    ctx.check(ctx.lib.anet_minco_yaw_partial_grads_dev(
        ctx.handle, _ref(yaw_penalty), int(s), int(sy), int(N), int(B), T.stride(0), _tptr(coeffs), _tptr(ycoeffs), _tptr(T),
        1 if accumulate else 0, _tptr(gdC), _tptr(gdCy), _tptr(gdT), _tptr(piece_cost), _stream_of(T, stream)))
    return gdC, gdCy, gdT, piece_cost


def minco_yaw_cost_grad_dev(head, tail, wps, yhead, ytail, ywps, T, s, c, sy, cy, N, B, yaw_penalty, hpolys=None, penalty=None,
                            extra_terms=(), stream=None, ctx=None):
    """J = int (p^(s))^2 + rho sum T + J_pen + [extra terms] + J_yaw and its gradient, composed at the C ABI:
    anet_minco_solve_dev, anet_minco_solve_scalar_dev -> anet_minco_partial_grads_dev -> every term of `extra_terms` ->
    anet_minco_yaw_partial_grads_dev(accumulate = 1) -> anet_minco_propagate_grad_dev (with the summed direct gdT),
    anet_minco_propagate_grad_scalar_dev (gdT = NULL) -> gradT summed.  An extra term is a callable
    term(coeffs, T, gdC, gdT, piece_cost, stream) that adds its complete share to the three outputs (an accumulate = 1 entry point,
    e.g. minco_stop_partial_grads_dev), so that the stop or the obstacle term can ride along.
    Returns cost (ld,), gradP (max(3 (N-1), 1), ld), gradPy (max(N-1, 1), ld), gradT (N, ld), coeffs, ycoeffs."""
    import torch
    from .minco import minco_solve_dev
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    st = _stream_of(T, stream)
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
    zeros = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float64)
    coeffs, energy = new(N * 3 * 2 * s, ld), new(ld)
    minco_solve_dev(head, tail, wps, T, s, c, N, B, coeffs=coeffs, energy=energy, stream=st.value, ctx=ctx)
    ycoeffs, _ = minco_solve_scalar_dev(yhead, ytail, ywps, T, sy, cy, N, B, stream=st.value, ctx=ctx)
    gdC, gdCy, gdT, pc = new(N * 3 * 2 * s, ld), new(N * 2 * sy, ld), new(N, ld), zeros(N, ld)
    ctx.check(ctx.lib.anet_minco_partial_grads_dev(ctx.handle, s, N, B, ld, _tptr(coeffs), _tptr(T), _tptr(hpolys),
                                                   _ref(penalty) if penalty is not None else None, 1, _tptr(gdC), _tptr(gdT),
                                                   _tptr(pc), st))
    for term in extra_terms:
        term(coeffs, T, gdC, gdT, pc, st.value)
    minco_yaw_partial_grads_dev(yaw_penalty, s, sy, N, B, coeffs, ycoeffs, T, gdC, gdCy, gdT, pc, accumulate=True, stream=st.value,
                                ctx=ctx)
    gradP, gradT = zeros(max(3 * (N - 1), 1), ld), new(N, ld)
    ctx.check(ctx.lib.anet_minco_propagate_grad_dev(ctx.handle, s, c, N, B, ld, _tptr(T), _tptr(coeffs), _tptr(gdC), _tptr(gdT),
                                                    _tptr(gradP), _tptr(gradT), st))
    gradPy, gradTy = minco_propagate_grad_scalar_dev(T, ycoeffs, gdCy, None, sy, cy, N, B, stream=st.value, ctx=ctx)
    rho = penalty.rho if penalty is not None else 0.0
    cost = energy + rho * T.sum(0) + pc.sum(0)
    gradT = gradT + gradTy
    if rho != 0.0:
        gradT = gradT + rho
    return cost, gradP, gradPy, gradT, coeffs, ycoeffs


def minco_yaw_cost_grad(head, tail, wps, yhead, ytail, ywps, T, s, sy, yaw_penalty, hpolys=None, penalty=None, ctx=None):
    """Host (numpy, trajectory-major) form of minco_yaw_cost_grad_dev: head, tail (B, 3, c); wps (B, N-1, 3); yhead, ytail (B, cy);
    ywps (B, N-1); T (B, N); hpolys (B, N, M, 4).  Returns cost (B,), gradP (B, N-1, 3), gradPy (B, N-1), gradT (B, N)."""
    import torch
    head = _f64(head)
    B, _, c = head.shape
    tail = _f64(tail, (B, 3, c))
    T = _f64(T)
    N = T.shape[1]
    wps = _f64(wps if wps is not None else np.zeros((B, 0, 3)), (B, N - 1, 3))
    yhead = _f64(yhead)
    cy = yhead.shape[1]
    ytail = _f64(ytail, (B, cy))
    ywps = _f64(ywps if ywps is not None else np.zeros((B, 0)), (B, N - 1))
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
    cost, gP, gPy, gT, _, _ = minco_yaw_cost_grad_dev(up(head.reshape(B, -1)), up(tail.reshape(B, -1)), up(wps.reshape(B, -1)),
                                                      up(yhead), up(ytail), up(ywps), d_T, s, c, sy, cy, N, B, yaw_penalty,
                                                      hpolys=d_hp, penalty=penalty, ctx=ctx)
    gradP = gP[:3 * (N - 1), :B].T.contiguous().cpu().numpy().reshape(B, N - 1, 3)
    gradPy = gPy[:N - 1, :B].T.contiguous().cpu().numpy().reshape(B, N - 1)
    return cost[:B].cpu().numpy(), gradP, gradPy, gT[:, :B].T.contiguous().cpu().numpy()


def yaw_objective_dev(head, tail, yhead, ytail, s, c, sy, cy, N, B, yaw_penalty, hpolys=None, penalty=None, extra_terms=(), ctx=None):
    """The composed objective as an `evaluate(x, f, g)` of lbfgs_optimize_dev: x (3 (N-1) + (N-1) + N, ld) holds the waypoints (the
    rows of minco_cost_grad_dev's wps), below them the N - 1 yaw waypoints and below those the LOG durations, so that every duration
    stays positive; g is the gradient w.r.t. x (dJ/dlog T = T dJ/dT)."""
    import torch
    nw, ny = 3 * (N - 1), N - 1

    def evaluate(x, f, g):
        T = torch.exp(x[nw + ny:nw + ny + N])
        one = lambda: torch.zeros(1, x.shape[1], device=x.device, dtype=torch.float64)
        wps = x[:nw] if nw else one()
        ywps = x[nw:nw + ny] if ny else one()
        cost, gP, gPy, gT, _, _ = minco_yaw_cost_grad_dev(head, tail, wps, yhead, ytail, ywps, T, s, c, sy, cy, N, B, yaw_penalty,
                                                          hpolys=hpolys, penalty=penalty, extra_terms=extra_terms, ctx=ctx)
        f.copy_(cost)
        if nw:
            g[:nw].copy_(gP[:nw])
            g[nw:nw + ny].copy_(gPy[:ny])
        g[nw + ny:nw + ny + N].copy_(gT * T)
    return evaluate


# ---------------------------------------------------------------------------------------------
# the sampled check, flat states
# ---------------------------------------------------------------------------------------------
def traj_yaw_margin_dev(yaw_penalty, v_min, s, sy, N, B, coeffs, ycoeffs, T, margin=None, t=None, rate=None, stream=None, ctx=None):
    """anet_traj_yaw_margin_dev: coeffs (N*3*2s, ld), ycoeffs (N*2sy, ld), T (N, ld) -> margin, t, rate (N, ld).  Only half_fov and
    res of the penalty are read."""
    import torch
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    new = lambda given: given if given is not None else torch.empty(N, ld, device=dev, dtype=torch.float64)
    margin, t, rate = new(margin), new(t), new(rate)
    ctx.check(ctx.lib.anet_traj_yaw_margin_dev(ctx.handle, _ref(yaw_penalty), float(v_min), int(s), int(sy), int(N), int(B), ld,
                                               _tptr(coeffs), _tptr(ycoeffs), _tptr(T), _tptr(margin), _tptr(t), _tptr(rate),
                                               _stream_of(T, stream)))
    return margin, t, rate


def traj_yaw_margin(coeffs, ycoeffs, T, half_fov, v_min=0.0, res=20, ctx=None):
    """The sampled look margin per piece (anet_traj_yaw_margin): coeffs (B, N, 3, D), ycoeffs (B, N, DY), T (B, N) numpy ->
    margin, t, rate (B, N).  margin: the least half_fov - |angle between the horizontal velocity and the heading| over the res + 1
    samples of the piece with |v_xy| >= v_min (+inf without one), t its local time, rate the largest |dpsi| over all samples.
    A SAMPLED check: nothing bounds the angle between samples.  NaN: a non-finite coefficient or duration of that piece, or a
    duration <= 0."""
    ctx = ctx or default_context()
    coeffs = _f64(coeffs); ycoeffs = _f64(ycoeffs); T = _f64(T)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N) or ycoeffs.ndim != 3 or ycoeffs.shape[:2] != (B, N):
        raise ValueError("shape mismatch")
    pen = make_yaw_penalty(0.0, 1.0, half_fov, 0.0, 0.0, 1.0, 1.0, 0.0, res)
    out = [np.empty((B, N)) for _ in range(3)]
    ctx.check(ctx.lib.anet_traj_yaw_margin(ctx.handle, _ref(pen), float(v_min), D // 2, ycoeffs.shape[2] // 2, N, B, _ptr(coeffs),
                                           _ptr(ycoeffs), _ptr(T), *[_ptr(o) for o in out]))
    return tuple(out)


def traj_flat_states_yaw(flatmap, coeffs, ycoeffs, T, tq, ctx=None):
    """traj_flat_states with the yaw (anet_traj_states_yaw): coeffs (B, N, 3, D), ycoeffs (B, N, DY), T (B, N), tq (B, nq)
    absolute times -> (B, nq, 11): thr, q0..q3, omg0..2, speed, tilt, body-rate magnitude, with psi, dpsi of the yaw piece."""
    ctx = ctx or default_context()
    coeffs = _f64(coeffs); ycoeffs = _f64(ycoeffs); T = _f64(T); tq = _f64(tq)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N) or tq.ndim != 2 or tq.shape[0] != B or ycoeffs.ndim != 3 or ycoeffs.shape[:2] != (B, N):
        raise ValueError("shape mismatch")
    nq = tq.shape[1]
    out = np.empty((B, nq, FLAT_STATE_FIELDS))
    ctx.check(ctx.lib.anet_traj_states_yaw(ctx.handle, _ref(_params_of(flatmap)), D // 2, ycoeffs.shape[2] // 2, N, B,
                                                _ptr(coeffs), _ptr(ycoeffs), _ptr(T), nq, _ptr(tq), _ptr(out)))
    return out


# ---------------------------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------------------------
def heading_waypoints(wps, head, tail):
    """The unwrapped tangent headings at the interior nodes, as a start for the yaw: wps (N-1, 3) or (B, N-1, 3), head and tail the
    end POSITIONS (3,) or (B, 3).  The tangent at node k is the chord from node k - 1 to node k + 1; the angles are unwrapped along
    the route, starting from the heading of the first chord.  Returns (heading of the start, (N-1,) or (B, N-1) headings, heading of
    the end), the two end headings being those of the first and the last segment."""
    wps = np.asarray(wps, dtype=np.float64)
    single = wps.ndim == 2
    if single:
        wps = wps[None]
    B = wps.shape[0]
    head = np.broadcast_to(np.asarray(head, dtype=np.float64).reshape(-1, 3), (B, 3))
    tail = np.broadcast_to(np.asarray(tail, dtype=np.float64).reshape(-1, 3), (B, 3))
    nodes = np.concatenate([head[:, None], wps, tail[:, None]], 1)                     # (B, N + 1, 3)
    seg = nodes[:, 1:, :2] - nodes[:, :-1, :2]
    chord = nodes[:, 2:, :2] - nodes[:, :-2, :2]
    ang = np.concatenate([np.arctan2(seg[:, :1, 1], seg[:, :1, 0]), np.arctan2(chord[..., 1], chord[..., 0]),
                          np.arctan2(seg[:, -1:, 1], seg[:, -1:, 0])], 1)
    ang = np.unwrap(ang, axis=1)
    return (ang[0, 0], ang[0, 1:-1], ang[0, -1]) if single else (ang[:, 0], ang[:, 1:-1], ang[:, -1])


class YawTrajectory:
    """The yaw polynomial of a trajectory: coeffs (N, 2 sy), highest power first, and the durations T (N,) it shares with the
    position trajectory.  Times are located as Trajectory locates them."""

    def __init__(self, coeffs, T):
        self.coeffs = _f64(coeffs)
        self.T = _f64(T, (self.coeffs.shape[0],))

    def getDurations(self):
        return self.T.copy()

    def getPieceNum(self):
        return self.T.shape[0]

    def _locate(self, t):
        t = float(t)
        for i, dur in enumerate(self.T):
            if not (t > dur):
                return i, t
            t -= dur
        return len(self.T) - 1, t + self.T[-1]

    def getYaw(self, t):
        i, tl = self._locate(t)
        return float(np.polyval(self.coeffs[i], tl))

    def getYawRate(self, t):
        i, tl = self._locate(t)
        return float(np.polyval(np.polyder(self.coeffs[i]), tl))
