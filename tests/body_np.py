"""Restatement of the whole-body corridor terms for the tests, in torch float64 on the CPU, built on tests/flatness_np.py (forward,
quat_to_rot, piece_derivs, smoothed_l1) and sharing nothing with the product code:

    g[j, r, k] = a_r . (p(t_j) + R(q(t_j)) b_k) - h_r,     q = the quaternion of flatness_np.forward at v, a, j with psi = 0,
    J_body     = sum_i (T_i/res) sum_{j<res} sum_r sum_k w phi(g),      t_j = j T_i / res,
    margin_i   = max over j = 0..res, the non-padding rows and the vertices of g.

R is flatness_np.quat_to_rot, the unit-quaternion form 1 - 2 (y^2 + z^2), ...: on the unit sphere it equals the homogeneous form the
kernels use.  The gradients are torch autograd of this forward at fixed coefficients."""
import numpy as np
import torch

from tests import flatness_np as fnp

_t = fnp._t


def terms(coeffs, T, hpolys, verts, res, closed=False, **par):
    """coeffs (B, N, 3, D), T (B, N), hpolys (B, N, M, 4), verts (K, 3) -> g (B, N, J, M, K) at t = j T_i / res, j < res
    (closed: j <= res); t (B, N, J); pad (B, N, M): the all-zero rows."""
    coeffs, T, hp, verts = _t(coeffs), _t(T), _t(hpolys), _t(verts)
    J = res + 1 if closed else res
    tau = torch.arange(J, dtype=torch.float64) / res
    t = T[..., None] * tau
    p, v, a, j = fnp.piece_derivs(coeffs[:, :, None], t)
    _, quat, _, _ = fnp.forward(v, a, j, **par)
    R = fnp.quat_to_rot(quat)                                              # (B, N, J, 3, 3)
    pts = p[..., None, :] + torch.einsum("bnjxy,ky->bnjkx", R, verts)      # (B, N, J, K, 3)
    g = torch.einsum("bnmx,bnjkx->bnjmk", hp[..., :3], pts) - hp[..., 3][:, :, None, :, None]
    return g, t, (hp == 0.0).all(-1)


def j_body(coeffs, T, hpolys, verts, res, w, mu, **par):
    """J_body per piece, (B, N)."""
    T = _t(T)
    g, _, pad = terms(coeffs, T, hpolys, verts, res, **par)
    phi = fnp.smoothed_l1(g, mu) * (~pad)[:, :, None, :, None]
    return w * (T / res) * phi.sum((-1, -2, -3))


def j_body_grads(coeffs, T, hpolys, verts, res, w, mu, **par):
    """cost per piece (B, N) and autograd partials at fixed coefficients: gdC (B, N, 3, D), gdT (B, N)."""
    c = _t(coeffs).clone().requires_grad_(True)
    t = _t(T).clone().requires_grad_(True)
    pc = j_body(c, t, hpolys, verts, res, w, mu, **par)
    gC, gT = torch.autograd.grad(pc.sum(), [c, t])
    return pc.detach().numpy(), gC.numpy(), gT.numpy()


def active_share(coeffs, T, hpolys, verts, res, **par):
    """the share of the (sample, non-padding row, vertex) terms with g > 0, and their number"""
    g, _, pad = terms(coeffs, T, hpolys, verts, res, **par)
    live = (~pad)[:, :, None, :, None].expand_as(g)
    n = int(live.sum())
    return float(((g > 0.0) & live).sum()) / n, n


def margin(coeffs, T, hpolys, verts, res, **par):
    """The sampled margin per piece over the closed sample set, (B, N) numpy (-inf: only padding rows), the terms g
    (B, N, res + 1, M, K) with padding rows at -inf, and the sample times t (B, N, res + 1)."""
    g, t, pad = terms(coeffs, T, hpolys, verts, res, closed=True, **par)
    g = torch.where(pad[:, :, None, :, None].expand_as(g), torch.full_like(g, -np.inf), g)
    return g.amax((-1, -2, -3)).numpy(), g.numpy(), t.numpy()


def term_at(coeffs, t, row, vert, **par):
    """a . (p(t) + R(q(t)) b) - h for one piece: coeffs (3, D), local time t, row (4,), vert (3,)"""
    p, v, a, j = fnp.piece_derivs(_t(coeffs), _t(np.float64(t)))
    _, quat, _, _ = fnp.forward(v, a, j, **par)
    pt = p + fnp.quat_to_rot(quat) @ _t(vert)
    return float((_t(row)[:3] * pt).sum() - _t(row)[3])
