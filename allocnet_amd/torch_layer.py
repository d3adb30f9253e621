"""The QP as a differentiable torch layer on the device: what OsqpLayer is to the reference's training loop
(network/utils/learning/layers.py:51-151 -- forward = solve with OSQP, backward = the -J^-1 grad KKT hook), with the
gradient carried through to the segment times.

    coeffs, obj, status = qp_layer(times, state, hpolys, order=4)       # times.requires_grad -> d loss / d times

forward: anet_qp_solve_time_grad_dev (interior point); backward: anet_qp_solve_vjp_dev for the part of the loss that
reaches the coefficients plus the envelope-theorem gradient for the part that is the optimal cost itself.  Problems the
solver reports unsolved (status != 1: infeasible corridor / limits) get a zero gradient; `status` tells which."""
import torch

from .qp import qp_solve_dev, qp_solve_vjp_dev


class _QPSolve(torch.autograd.Function):
    @staticmethod
    def forward(fctx, times, state, hpolys, order, res, max_vel, max_acc, m34, anet_ctx, rows=None):
        t = times.detach().contiguous()
        out = qp_solve_dev(order, state, t, hpolys, res=res, max_vel=max_vel, max_acc=max_acc, m34=m34, time_grad=True,
                           ctx=anet_ctx, rows=rows)
        fctx.save_for_backward(t, state, hpolys, out["grad_T"], out["status"])
        fctx.meta = (order, res, max_vel, max_acc, m34, anet_ctx, rows)
        fctx.mark_non_differentiable(out["status"])
        # undefined output gradients stay None: a loss that only uses `obj` must not pay the second QP solve of the
        # backward pass through the coefficients
        fctx.set_materialize_grads(False)
        return out["coeffs"], out["obj"], out["status"]

    @staticmethod
    def backward(fctx, g_coeffs, g_obj, _g_status):
        t, state, hpolys, env, status = fctx.saved_tensors
        order, res, max_vel, max_acc, m34, anet_ctx, rows = fctx.meta
        if not fctx.needs_input_grad[0]:
            return (None,) * 10
        grad = torch.zeros_like(t)
        if g_coeffs is not None:
            back = qp_solve_vjp_dev(order, state, t, hpolys, g_coeffs.contiguous(), res=res, max_vel=max_vel,
                                    max_acc=max_acc, m34=m34, ctx=anet_ctx, rows=rows)
            ok = (back["status"] == 1) & (status == 1)
            grad = torch.where(ok[:, None], back["grad_T"], grad)
        if g_obj is not None:
            grad = grad + torch.where((status == 1)[:, None], g_obj[:, None] * env, torch.zeros_like(env))
        return grad, None, None, None, None, None, None, None, None, None


def qp_layer(times, state, hpolys, order=4, res=20, max_vel=4.0, max_acc=6.0, m34=1400.0, ctx=None, rows=None):
    """times (B,N) float64 CUDA (may require grad); state (B,2,3,3) = [start PVA, end PVA]; hpolys (B,N,M,4) planner form,
    zero rows as padding.  rows="control_points": the rows on Bernstein control values (res = qp.control_point_res(order,
    segments)), forward and backward.  Returns (coeffs (B,N,3,2*order), obj (B,), status (B,) int32)."""
    return _QPSolve.apply(times, state.contiguous(), hpolys.contiguous(), int(order), int(res), float(max_vel),
                          float(max_acc), float(m34), ctx, rows)


class _MincoSolve(torch.autograd.Function):
    """coefficients and energy of the minimum-control trajectory through (wps, T) as a differentiable function of the
    interior waypoints and the durations: forward = anet_minco_solve_dev, backward = MINCO's propogateGrad
    (anet_minco_propagate_grad_dev) fed with d loss / d coeffs plus d loss / d energy times the energy's own partials
    (anet_minco_partial_grads_dev).  Batch-minor tensors, common row stride."""

    @staticmethod
    def forward(fctx, wps, T, head, tail, s, c, N, B, anet_ctx):
        import ctypes
        from .context import default_context
        from .minco import minco_solve_dev
        actx = anet_ctx or default_context(T.device.index or 0)
        ld = T.stride(0)
        coeffs = torch.empty(N * 3 * 2 * s, ld, device=T.device, dtype=torch.float64)
        energy = torch.empty(ld, device=T.device, dtype=torch.float64)
        minco_solve_dev(head, tail, wps.detach() if wps is not None else None, T.detach(), s, c, N, B, coeffs=coeffs,
                        energy=energy, ctx=actx)            # (one piece: no interior waypoints, wps may be None)
        fctx.save_for_backward(T.detach(), coeffs)
        fctx.meta = (s, c, N, B, actx)
        fctx.set_materialize_grads(False)
        return coeffs, energy

    @staticmethod
    def backward(fctx, g_coeffs, g_energy):
        import ctypes
        T, coeffs = fctx.saved_tensors
        s, c, N, B, actx = fctx.meta
        ld = T.stride(0)
        dev = T.device
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        q = lambda t: ctypes.c_void_p(t.data_ptr())
        gdC = torch.zeros_like(coeffs) if g_coeffs is None else g_coeffs.contiguous().clone()
        gdT = torch.zeros(N, ld, device=dev, dtype=torch.float64)
        if g_energy is not None:
            eC = torch.empty_like(coeffs); eT = torch.empty(N, ld, device=dev, dtype=torch.float64)
            actx.check(actx.lib.anet_minco_partial_grads_dev(actx.handle, s, N, B, ld, q(coeffs), q(T), None, None, 1, q(eC), q(eT),
                                                            None, st))
            gdC = gdC + g_energy[None, :] * eC
            gdT = gdT + g_energy[None, :] * eT
        gP = torch.zeros(max(3 * (N - 1), 1), ld, device=dev, dtype=torch.float64)
        gT = torch.zeros(N, ld, device=dev, dtype=torch.float64)
        actx.check(actx.lib.anet_minco_propagate_grad_dev(actx.handle, s, c, N, B, ld, q(T), q(coeffs), q(gdC), q(gdT), q(gP), q(gT), st))
        return (gP if N > 1 else None), gT, None, None, None, None, None, None, None


def minco_layer(wps, T, head, tail, s, c, N, B, ctx=None):
    """Batch-minor float64 CUDA tensors with a common row stride ld = T.stride(0): wps ((N-1)*3, ld), T (N, ld),
    head / tail (3c, ld).  Returns coeffs (N*3*2s, ld) and energy (ld,); gradients flow to wps and T."""
    return _MincoSolve.apply(wps, T, head, tail, int(s), int(c), int(N), int(B), ctx)


class _FlatMap(torch.autograd.Function):
    """The flatness map as a differentiable function of (vel, acc, jer, psi, dpsi): forward = anet_flat_forward_dev, backward =
    anet_flat_backward_dev on the saved inputs (the kernel recomputes the forward intermediates)."""

    @staticmethod
    def forward(fctx, vel, acc, jer, psi, dpsi, params, n, anet_ctx):
        from .flatness import flat_forward_dev
        ins = tuple(t.detach().contiguous() for t in (vel, acc, jer, psi, dpsi))
        thr, quat, omg = flat_forward_dev(params, *ins, n=n, ctx=anet_ctx)
        fctx.save_for_backward(*ins)
        fctx.meta = (params, n, anet_ctx)
        return thr, quat, omg

    @staticmethod
    def backward(fctx, g_thr, g_quat, g_omg):
        from .flatness import flat_backward_dev
        vel, acc, jer, psi, dpsi = fctx.saved_tensors
        params, n, anet_ctx = fctx.meta
        _, vt, at, jt, pst, dpt = flat_backward_dev(params, vel, acc, jer, psi, dpsi, None, None, g_thr.contiguous(),
                                                    g_quat.contiguous(), g_omg.contiguous(), n=n, ctx=anet_ctx)
        return vt, at, jt, pst, dpt, None, None, None


def flat_layer(vel, acc, jer, psi, dpsi, params, n=None, ctx=None):
    """Batch-minor float64 CUDA tensors: vel, acc, jer (3, ld), psi, dpsi (ld,); params: anet_flat_params
    (flatness.make_flat_params) or a FlatnessMap.  Returns thr (ld,), quat (4, ld), omg (3, ld); gradients flow to all five
    inputs.  Elements [n, ld) are padding: their outputs and gradients are not computed (n defaults to ld)."""
    from .flatness import _params_of
    return _FlatMap.apply(vel, acc, jer, psi, dpsi, _params_of(params), n, ctx)
