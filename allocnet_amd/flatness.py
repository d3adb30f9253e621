"""Differential flatness of the quadrotor: host mirror of flatness::FlatnessMap (gcopter/flatness.hpp) and what follows
from the same map -- thrust, attitude and body rate along trajectories, a sampled feasibility check in the vehicle's own
terms, and the thrust / tilt / body-rate penalty of the MINCO objective with its gradient.

All arithmetic runs in the HIP kernels of csrc/flatness_kernels.h behind anet_flat_* / anet_traj_flat_* /
anet_minco_flat_partial_grads_dev; nothing here computes the map on the host.
"""
import ctypes
import numpy as np

from ._lib import FlatParams, FlatPenalty
from .context import default_context

FLAT_STATE_FIELDS = 11      # thr, q0..q3, omg0..2, speed, tilt, body-rate magnitude (ANET_FLAT_STATE_FIELDS)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _tptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ref(struct):
    return ctypes.cast(ctypes.pointer(struct), ctypes.c_void_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def make_flat_params(mass=1.0, grav=9.8, horiz_drag=0.7, vert_drag=0.8, paras_drag=0.01, speed_eps=1e-4):
    """struct anet_flat_params.  Defaults: the vehicle of the reference's launch file."""
    return FlatParams(float(mass), float(grav), float(horiz_drag), float(vert_drag), float(paras_drag), float(speed_eps))


def make_flat_penalty(w_thrust=0.0, w_tilt=0.0, w_bdr=0.0, smooth_mu=1e-2, min_thrust=0.0, max_thrust=20.0,
                      max_tilt=1.0, max_bdr=3.0, res=20):
    """struct anet_flat_penalty: weights and limits of J_flat (include/allocnet_amd.h)."""
    return FlatPenalty(float(w_thrust), float(w_tilt), float(w_bdr), float(smooth_mu), float(min_thrust), float(max_thrust),
                       float(max_tilt), float(max_bdr), int(res))


def _params_of(flatmap):
    if isinstance(flatmap, FlatnessMap):
        return flatmap.params
    if isinstance(flatmap, FlatParams):
        return flatmap
    raise TypeError("a FlatnessMap or anet_flat_params expected")


# ---------------------------------------------------------------------------------------------
# pointwise map and adjoint
# ---------------------------------------------------------------------------------------------
def flat_forward(params, vel, acc, jer, psi=None, dpsi=None, ctx=None):
    """Host entry point -> anet_flat_forward.  vel, acc, jer (n, 3); psi, dpsi (n,) or None (= 0).
    Returns thr (n,), quat (n, 4) as (w, x, y, z), omg (n, 3)."""
    ctx = ctx or default_context()
    vel = _f64(vel)
    n = vel.shape[0]
    if vel.shape != (n, 3):
        raise ValueError("vel must be (n, 3)")
    acc = _f64(acc, (n, 3)); jer = _f64(jer, (n, 3))
    psi = _f64(psi, (n,)) if psi is not None else None
    dpsi = _f64(dpsi, (n,)) if dpsi is not None else None
    thr = np.empty(n); quat = np.empty((n, 4)); omg = np.empty((n, 3))
    ctx.check(ctx.lib.anet_flat_forward(ctx.handle, _ref(params), n, _ptr(vel), _ptr(acc), _ptr(jer), _ptr(psi), _ptr(dpsi),
                                        _ptr(thr), _ptr(quat), _ptr(omg)))
    return thr, quat, omg


def flat_backward(params, vel, acc, jer, psi, dpsi, pos_grad, vel_grad, thr_grad, quat_grad, omg_grad, ctx=None):
    """Host entry point -> anet_flat_backward (FlatnessMap::backward, batched and stateless).  pos_grad / vel_grad may be None.
    Returns pos_total, vel_total, acc_total, jer_total (n, 3), psi_total, dpsi_total (n,)."""
    ctx = ctx or default_context()
    vel = _f64(vel)
    n = vel.shape[0]
    acc = _f64(acc, (n, 3)); jer = _f64(jer, (n, 3))
    psi = _f64(psi, (n,)) if psi is not None else None
    dpsi = _f64(dpsi, (n,)) if dpsi is not None else None
    pos_grad = _f64(pos_grad, (n, 3)) if pos_grad is not None else None
    vel_grad = _f64(vel_grad, (n, 3)) if vel_grad is not None else None
    thr_grad = _f64(thr_grad, (n,)); quat_grad = _f64(quat_grad, (n, 4)); omg_grad = _f64(omg_grad, (n, 3))
    pt = np.empty((n, 3)); vt = np.empty((n, 3)); at = np.empty((n, 3)); jt = np.empty((n, 3))
    pst = np.empty(n); dpt = np.empty(n)
    ctx.check(ctx.lib.anet_flat_backward(ctx.handle, _ref(params), n, _ptr(vel), _ptr(acc), _ptr(jer), _ptr(psi), _ptr(dpsi),
                                         _ptr(pos_grad), _ptr(vel_grad), _ptr(thr_grad), _ptr(quat_grad), _ptr(omg_grad),
                                         _ptr(pt), _ptr(vt), _ptr(at), _ptr(jt), _ptr(pst), _ptr(dpt)))
    return pt, vt, at, jt, pst, dpt


def _stream_of(t, stream):
    import torch
    return ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(t.device).cuda_stream)


def flat_forward_dev(params, vel, acc, jer, psi=None, dpsi=None, n=None, thr=None, quat=None, omg=None, stream=None, ctx=None):
    """Device entry point -> anet_flat_forward_dev.  torch CUDA float64, batch-minor: vel, acc, jer (3, ld); psi, dpsi (ld,) or
    None; n elements (default ld).  Returns thr (ld,), quat (4, ld), omg (3, ld)."""
    import torch
    ctx = ctx or default_context(vel.device.index or 0)
    ld = vel.stride(0)
    n = ld if n is None else int(n)
    thr = thr if thr is not None else torch.empty(ld, device=vel.device, dtype=torch.float64)
    quat = quat if quat is not None else torch.empty(4, ld, device=vel.device, dtype=torch.float64)
    omg = omg if omg is not None else torch.empty(3, ld, device=vel.device, dtype=torch.float64)
    ctx.check(ctx.lib.anet_flat_forward_dev(ctx.handle, _ref(params), n, ld, _tptr(vel), _tptr(acc), _tptr(jer), _tptr(psi),
                                            _tptr(dpsi), _tptr(thr), _tptr(quat), _tptr(omg), _stream_of(vel, stream)))
    return thr, quat, omg


def flat_backward_dev(params, vel, acc, jer, psi, dpsi, pos_grad, vel_grad, thr_grad, quat_grad, omg_grad, n=None, stream=None,
                      ctx=None):
    """Device entry point -> anet_flat_backward_dev (layouts of flat_forward_dev).  Returns pos_total, vel_total, acc_total,
    jer_total (3, ld), psi_total, dpsi_total (ld,)."""
    import torch
    ctx = ctx or default_context(vel.device.index or 0)
    ld = vel.stride(0)
    n = ld if n is None else int(n)
    new = lambda *shape: torch.empty(*shape, device=vel.device, dtype=torch.float64)
    pt, vt, at, jt, pst, dpt = new(3, ld), new(3, ld), new(3, ld), new(3, ld), new(ld), new(ld)
    ctx.check(ctx.lib.anet_flat_backward_dev(ctx.handle, _ref(params), n, ld, _tptr(vel), _tptr(acc), _tptr(jer), _tptr(psi),
                                             _tptr(dpsi), _tptr(pos_grad), _tptr(vel_grad), _tptr(thr_grad), _tptr(quat_grad),
                                             _tptr(omg_grad), _tptr(pt), _tptr(vt), _tptr(at), _tptr(jt), _tptr(pst), _tptr(dpt),
                                             _stream_of(vel, stream)))
    return pt, vt, at, jt, pst, dpt


class FlatnessMap:
    """flatness::FlatnessMap (gcopter/flatness.hpp:34-260) for one state: reset / forward / backward.  backward applies to the
    inputs of the last forward, as the reference's cached members imply."""

    def __init__(self, ctx=None):
        self.params = make_flat_params()
        self._ctx = ctx
        self._last = None

    def reset(self, vehicle_mass, gravitational_acceleration, horizontal_drag_coeff, vertical_drag_coeff,
              parasitic_drag_coeff, speed_smooth_factor):
        self.params = make_flat_params(vehicle_mass, gravitational_acceleration, horizontal_drag_coeff, vertical_drag_coeff,
                                       parasitic_drag_coeff, speed_smooth_factor)
        self._last = None

    def forward(self, vel, acc, jer, psi=0.0, dpsi=0.0):
        """-> thr (float), quat (4,) as (w, x, y, z), omg (3,)."""
        v, a, j = (_f64(x).reshape(1, 3) for x in (vel, acc, jer))
        ps, dps = np.array([float(psi)]), np.array([float(dpsi)])
        thr, quat, omg = flat_forward(self.params, v, a, j, ps, dps, ctx=self._ctx)
        self._last = (v, a, j, ps, dps)
        return float(thr[0]), quat[0], omg[0]

    def backward(self, pos_grad, vel_grad, thr_grad, quat_grad, omg_grad):
        """-> pos_total, vel_total, acc_total, jer_total (3,), psi_total, dpsi_total (float)."""
        if self._last is None:
            raise RuntimeError("forward first")
        v, a, j, ps, dps = self._last
        out = flat_backward(self.params, v, a, j, ps, dps, _f64(pos_grad).reshape(1, 3), _f64(vel_grad).reshape(1, 3),
                            np.array([float(thr_grad)]), _f64(quat_grad).reshape(1, 4), _f64(omg_grad).reshape(1, 3),
                            ctx=self._ctx)
        return out[0][0], out[1][0], out[2][0], out[3][0], float(out[4][0]), float(out[5][0])


# ---------------------------------------------------------------------------------------------
# along trajectories
# ---------------------------------------------------------------------------------------------
def traj_flat_states(flatmap, coeffs, T, tq, ctx=None):
    """coeffs (B, N, 3, D), T (B, N), tq (B, nq) absolute times -> (B, nq, 11): thr, q0..q3, omg0..2, speed, tilt, body-rate
    magnitude at each query (psi = dpsi = 0), with Trajectory's piece location."""
    ctx = ctx or default_context()
    coeffs = _f64(coeffs); T = _f64(T); tq = _f64(tq)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N) or tq.ndim != 2 or tq.shape[0] != B:
        raise ValueError("shape mismatch")
    nq = tq.shape[1]
    out = np.empty((B, nq, FLAT_STATE_FIELDS))
    ctx.check(ctx.lib.anet_traj_flat_states(ctx.handle, _ref(_params_of(flatmap)), D // 2, N, B, _ptr(coeffs), _ptr(T), nq,
                                            _ptr(tq), _ptr(out)))
    return out


def traj_flat_extrema(flatmap, coeffs, T, res=20, ctx=None):
    """coeffs (B, N, 3, D), T (B, N) -> (B, 4): min thrust, max thrust, max tilt, max body-rate magnitude over the samples
    t = j T_i / res, j = 0..res, of every piece.  A sampled check (nothing bounds the values between the samples)."""
    ctx = ctx or default_context()
    coeffs = _f64(coeffs); T = _f64(T)
    B, N, three, D = coeffs.shape
    if three != 3 or T.shape != (B, N):
        raise ValueError("shape mismatch")
    out = np.empty((B, 4))
    ctx.check(ctx.lib.anet_traj_flat_extrema(ctx.handle, _ref(_params_of(flatmap)), D // 2, N, B, _ptr(coeffs), _ptr(T), int(res),
                                             _ptr(out)))
    return out


# ---------------------------------------------------------------------------------------------
# the penalty of the MINCO objective
# ---------------------------------------------------------------------------------------------
def minco_flat_partial_grads_dev(params, flat_penalty, s, N, B, coeffs, T, gdC, gdT, piece_cost=None, accumulate=False,
                                 stream=None, ctx=None):
    """anet_minco_flat_partial_grads_dev on batch-minor torch CUDA float64 tensors with the row stride of T."""
    ctx = ctx or default_context(T.device.index or 0)
    ctx.check(ctx.lib.anet_minco_flat_partial_grads_dev(ctx.handle, _ref(params), _ref(flat_penalty), int(s), int(N), int(B),
                                                        T.stride(0), _tptr(coeffs), _tptr(T), 1 if accumulate else 0, _tptr(gdC),
                                                        _tptr(gdT), _tptr(piece_cost), _stream_of(T, stream)))
    return gdC, gdT, piece_cost


def minco_flat_cost_grad_dev(head, tail, wps, T, s, c, N, B, flatmap, flat_penalty, hpolys=None, penalty=None, stream=None,
                             ctx=None):
    """J = int (p^(s))^2 + rho sum T + J_pen + J_flat and its gradient, composed at the C ABI: anet_minco_solve_dev ->
    anet_minco_partial_grads_dev -> anet_minco_flat_partial_grads_dev(accumulate = 1) -> anet_minco_propagate_grad_dev.
    Batch-minor torch CUDA float64 tensors with a common row stride (as minco_cost_grad_dev).
    Returns cost (ld,), gradP (max(3 (N-1), 1), ld), gradT (N, ld), coeffs (N*3*2s, ld)."""
    import torch
    from .minco import minco_solve_dev
    ctx = ctx or default_context(T.device.index or 0)
    ld, dev = T.stride(0), T.device
    st = _stream_of(T, stream)
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
    coeffs, energy = new(N * 3 * 2 * s, ld), new(ld)
    minco_solve_dev(head, tail, wps, T, s, c, N, B, coeffs=coeffs, energy=energy, stream=st.value, ctx=ctx)
    gdC, gdT, pc = new(N * 3 * 2 * s, ld), new(N, ld), torch.zeros(N, ld, device=dev, dtype=torch.float64)
    ctx.check(ctx.lib.anet_minco_partial_grads_dev(ctx.handle, s, N, B, ld, _tptr(coeffs), _tptr(T), _tptr(hpolys),
                                                   _ref(penalty) if penalty is not None else None, 1, _tptr(gdC), _tptr(gdT),
                                                   _tptr(pc), st))
    ctx.check(ctx.lib.anet_minco_flat_partial_grads_dev(ctx.handle, _ref(_params_of(flatmap)), _ref(flat_penalty), s, N, B, ld,
                                                        _tptr(coeffs), _tptr(T), 1, _tptr(gdC), _tptr(gdT), _tptr(pc), st))
    gradP, gradT = torch.zeros(max(3 * (N - 1), 1), ld, device=dev, dtype=torch.float64), new(N, ld)
    ctx.check(ctx.lib.anet_minco_propagate_grad_dev(ctx.handle, s, c, N, B, ld, _tptr(T), _tptr(coeffs), _tptr(gdC), _tptr(gdT),
                                                    _tptr(gradP), _tptr(gradT), st))
    # the adjoint kernel is given no cost to assemble here: the sum of the terms and rho's share of the time gradient
    rho = penalty.rho if penalty is not None else 0.0
    cost = energy + rho * T.sum(0) + pc.sum(0)
    if rho != 0.0:
        gradT = gradT + rho
    return cost, gradP, gradT, coeffs


def minco_flat_cost_grad(head, tail, wps, T, s, flatmap, flat_penalty, hpolys=None, penalty=None, ctx=None):
    """Host (numpy, trajectory-major) form of minco_flat_cost_grad_dev, with minco_cost_grad's shapes: head, tail (B, 3, c);
    wps (B, N-1, 3); T (B, N); hpolys (B, N, M, 4).  Returns cost (B,), gradP (B, N-1, 3), gradT (B, N)."""
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
    cost, gP, gT, _ = minco_flat_cost_grad_dev(up(head.reshape(B, -1)), up(tail.reshape(B, -1)), up(wps.reshape(B, -1)), d_T, s, c,
                                               N, B, flatmap, flat_penalty, hpolys=d_hp, penalty=penalty, ctx=ctx)
    gradP = gP[:3 * (N - 1), :B].T.contiguous().cpu().numpy().reshape(B, N - 1, 3)
    return cost[:B].cpu().numpy(), gradP, gT[:, :B].T.contiguous().cpu().numpy()
