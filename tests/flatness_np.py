"""Restatement of the differential-flatness map for the tests, in torch float64 on the CPU, written from the formulas and
sharing nothing with the product code:

    w   = (1 + cp sqrt(|v|^2 + eps)) v
    zu  = a + (dh/m) w + g e3,      z = zu / |zu|
    dz  = (I - z z^T)(j + (dh/m) dw/dt) / |zu|
    thr = z . (m a + dv w + m g e3)
    quat = tilt(z) * yaw(psi),      omg = body rate of (z, dz, psi, dpsi)

Its backward is torch autograd of this forward.  The penalty J_flat is the quadrature of include/allocnet_amd.h
(anet_flat_penalty) over polynomial pieces evaluated in torch.  tests/test_flatness_cpu.py checks this file against facts
that do not depend on it (hover, unit quaternion, R(quat) e3 = z, omg = 2 conj(q) (x) dq/dt by finite differences)."""
import math

import numpy as np
import torch

LAUNCH = dict(mass=1.0, grav=9.8, dh=0.7, dv=0.8, cp=0.01, eps=1e-4)     # the launch file's vehicle


def _t(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))


def forward(vel, acc, jer, psi=None, dpsi=None, mass=1.0, grav=9.8, dh=0.7, dv=0.8, cp=0.01, eps=1e-4):
    """vel, acc, jer (..., 3); psi, dpsi (...) or None -> thr (...), quat (..., 4) as (w, x, y, z), omg (..., 3), z (..., 3)."""
    v, a, j = _t(vel), _t(acc), _t(jer)
    psi = torch.zeros(v.shape[:-1], dtype=torch.float64) if psi is None else _t(psi)
    dpsi = torch.zeros(v.shape[:-1], dtype=torch.float64) if dpsi is None else _t(dpsi)
    e3 = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    speed = torch.sqrt((v * v).sum(-1, keepdim=True) + eps)
    w = (1.0 + cp * speed) * v
    dw = (1.0 + cp * speed) * a + cp * ((v * a).sum(-1, keepdim=True) / speed) * v          # d/dt of w
    zu = a + (dh / mass) * w + grav * e3
    L = torch.sqrt((zu * zu).sum(-1, keepdim=True))
    z = zu / L
    u = j + (dh / mass) * dw
    dz = (u - z * (z * u).sum(-1, keepdim=True)) / L
    thr = (z * (mass * a + dv * w + mass * grav * e3)).sum(-1)
    # tilt: the shortest rotation taking e3 to z, (cos(th/2), sin(th/2) axis), axis = e3 x z / |e3 x z|
    den = torch.sqrt(2.0 * (1.0 + z[..., 2]))
    tw, tx, ty = 0.5 * den, -z[..., 1] / den, z[..., 0] / den
    # composed with the yaw (cos(psi/2), 0, 0, sin(psi/2)) on the right: Hamilton product, tilt's z component is 0
    ch, sh = torch.cos(0.5 * psi), torch.sin(0.5 * psi)
    quat = torch.stack([tw * ch, tx * ch + ty * sh, ty * ch - tx * sh, tw * sh], dim=-1)
    # body rate: omg = 2 conj(q) (x) dq/dt worked out for this q(z, psi)
    c, s = torch.cos(psi), torch.sin(psi)
    k = dz[..., 2] / (1.0 + z[..., 2])
    omg = torch.stack([dz[..., 0] * s - dz[..., 1] * c - (z[..., 0] * s - z[..., 1] * c) * k,
                       dz[..., 0] * c + dz[..., 1] * s - (z[..., 0] * c + z[..., 1] * s) * k,
                       (z[..., 1] * dz[..., 0] - z[..., 0] * dz[..., 1]) / (1.0 + z[..., 2]) + dpsi], dim=-1)
    return thr, quat, omg, z


def backward(vel, acc, jer, psi, dpsi, thr_grad, quat_grad, omg_grad, **par):
    """Autograd of `forward`: gradients w.r.t. vel, acc, jer, psi, dpsi of <thr_grad, thr> + <quat_grad, quat> + <omg_grad, omg>."""
    ins = [_t(x).clone().requires_grad_(True) for x in (vel, acc, jer, psi, dpsi)]
    thr, quat, omg, _ = forward(*ins, **par)
    loss = (thr * _t(thr_grad)).sum() + (quat * _t(quat_grad)).sum() + (omg * _t(omg_grad)).sum()
    return [g.numpy() for g in torch.autograd.grad(loss, ins)]


def tilt_of_quat(q):
    """Tilt angle of a unit quaternion (w, x, y, z): sin^2(tilt/2) = x^2 + y^2, cos^2(tilt/2) = w^2 + z^2.  Equal to
    acos(1 - 2 (x^2 + y^2)), the expression process() publishes, but accurate at small tilts (where 1 - 2 (x^2 + y^2) rounds the
    tilt away) and finite next to inversion."""
    q = _t(q)
    return 2.0 * torch.atan2(torch.sqrt(q[..., 1] ** 2 + q[..., 2] ** 2), torch.sqrt(q[..., 0] ** 2 + q[..., 3] ** 2))


def quat_to_rot(q):
    """Rotation matrix of a unit quaternion (w, x, y, z), (..., 3, 3)."""
    q = _t(q)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def quat_mul(p, q):
    p, q = _t(p), _t(q)
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                        pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], -1)


def smoothed_l1(x, mu):
    """firi::smoothedL1: 0 below 0, (mu - x/2) (x/mu)^3 up to mu, x - mu/2 above."""
    xc = torch.clamp(x, min=0.0)
    cubic = (mu - 0.5 * xc) * (xc / mu) ** 3
    return torch.where(x < 0.0, torch.zeros_like(x), torch.where(x > mu, x - 0.5 * mu, cubic))


def piece_derivs(coeffs, t, dmax=3):
    """coeffs (..., 3, D) highest power first, t (...,) local time -> [p, v, a, j, ...][: dmax + 1], each (..., 3)."""
    coeffs, t = _t(coeffs), _t(t)
    D = coeffs.shape[-1]
    out = []
    for d in range(dmax + 1):
        acc = torch.zeros(coeffs.shape[:-1], dtype=torch.float64)
        for col in range(D):
            k = D - 1 - col
            if k >= d:
                acc = acc + math.perm(k, d) * coeffs[..., col] * t[..., None] ** (k - d)
        out.append(acc)
    return out


def traj_samples(coeffs, T, res, closed=False, **par):
    """Flat outputs at t = j T_i / res of every piece, j < res (closed: j <= res).  coeffs (B, N, 3, D), T (B, N) ->
    thr (B, N, J), cos_tilt (B, N, J), bdr2 (B, N, J), speed (B, N, J), |a|_inf, |v|_inf (B, N, J)."""
    coeffs, T = _t(coeffs), _t(T)
    J = res + 1 if closed else res
    tau = torch.arange(J, dtype=torch.float64) / res
    t = T[..., None] * tau                                            # (B, N, J)
    _, v, a, j = piece_derivs(coeffs[:, :, None], t)
    thr, quat, omg, z = forward(v, a, j, **par)
    cos_tilt = 1.0 - 2.0 * (quat[..., 1] ** 2 + quat[..., 2] ** 2)
    return dict(thr=thr, cos_tilt=cos_tilt, bdr2=(omg * omg).sum(-1), speed=torch.sqrt((v * v).sum(-1)),
                vmax=v.abs().amax(-1), amax=a.abs().amax(-1), quat=quat, omg=omg, z=z)


def j_flat(coeffs, T, res, w_thr, w_tilt, w_bdr, mu, thr_min, thr_max, tilt_max, bdr_max, **par):
    """J_flat per piece, (B, N): (T_i/res) sum_{j<res} [w_thr (phi(thr - max) + phi(min - thr)) + w_tilt phi(cos(tilt_max) - cos tilt)
    + w_bdr phi(|omg|^2 - bdr_max^2)]."""
    T = _t(T)
    sm = traj_samples(coeffs, T, res, **par)
    phi = (w_thr * (smoothed_l1(sm["thr"] - thr_max, mu) + smoothed_l1(thr_min - sm["thr"], mu))
           + w_tilt * smoothed_l1(math.cos(tilt_max) - sm["cos_tilt"], mu)
           + w_bdr * smoothed_l1(sm["bdr2"] - bdr_max ** 2, mu))
    return (T / res) * phi.sum(-1)


def j_flat_grads(coeffs, T, res, **kw):
    """cost per piece (B, N) and autograd partials at fixed coefficients: gdC (B, N, 3, D), gdT (B, N)."""
    c = _t(coeffs).clone().requires_grad_(True)
    t = _t(T).clone().requires_grad_(True)
    pc = j_flat(c, t, res, **kw)
    gC, gT = torch.autograd.grad(pc.sum(), [c, t])
    return pc.detach().numpy(), gC.numpy(), gT.numpy()


def scale_into_limits(coeffs_of, T, res=40, vlim=4.0, alim=6.0, factor=1.15, **par):
    """Scale the durations of each trajectory by a common factor until the sampled |v|, |a| per axis are inside the planner's
    boxes (MaxVelBox 4, MaxAccBox 6), so that zu_3 > 0 along it.  coeffs_of(T) -> coeffs (B, N, 3, D)."""
    T = np.array(T, dtype=np.float64)
    for _ in range(60):
        co = coeffs_of(T)
        sm = traj_samples(co, T, res, closed=True, **par)
        bad = ((sm["vmax"].amax((1, 2)) > 0.95 * vlim) | (sm["amax"].amax((1, 2)) > 0.95 * alim)).numpy()
        if not bad.any():
            return T, co
        T[bad] *= factor
    raise AssertionError("could not scale the trajectories into the limits")
