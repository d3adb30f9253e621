"""A float64 numpy restatement of the stop-within-known-space term and its sampled margin (include/allocnet_amd.h:
anet_minco_stop_partial_grads_dev, anet_traj_stop_margin[_dev]) on top of tests/dist_np.py: the field's query, the sample points and
smoothedL1 are that module's.  Trajectory-major arrays: co (B, N, 3, D), T (B, N)."""
import numpy as np

from tests.avoid_np import horner
from tests.dist_np import query, sample_points, smoothed_l1


def accel(co_b, tau):
    """a (N, res, 3) of one trajectory at tau (N, res): columns hold the powers D - 1 - col."""
    D = co_b.shape[-1]
    k = (D - 1 - np.arange(D)).astype(np.float64)
    c2 = co_b[:, None, :, :] * (k * (k - 1.0))                           # (N, 1, 3, D)
    pw = np.maximum(k - 2.0, 0.0)
    return (c2 * tau[:, :, None, None] ** pw).sum(-1)


def stop_distance(vv, a_brake, t_react, speed):
    """t_react * speed + v.v / (2 a_brake); the first term is absent when t_react == 0."""
    out = vv / (2.0 * a_brake)
    return out + t_react * speed if t_react > 0.0 else out


def j_stop_grads(co, T, res, w, mu, clearance, a_brake, t_react, speed_eps, sd2, size, origin, scale, parts=False):
    """-> piece_cost (B, N), gdC (B, N, 3, D), gdT (B, N); parts=True adds the G share of gdC and the per-sample g (B, N, res)."""
    B, N, _, D = co.shape
    pc, gC, gT = np.zeros((B, N)), np.zeros((B, N, 3, D)), np.zeros((B, N))
    gC_G, g_all = np.zeros((B, N, 3, D)), np.full((B, N, res), np.nan)
    k = D - 1 - np.arange(D)
    powers, powers_m1 = k[None, None, :], np.maximum(k - 1, 0)[None, None, :]
    for b in range(B):
        if not (np.isfinite(T[b]).all() and (T[b] > 0.0).all()):
            pc[b], gC[b], gT[b] = np.nan, np.nan, np.nan
            continue
        sigma, tau, p, v = sample_points(co[b], T[b], res)
        a = accel(co[b], tau)
        d, gd = query(sd2, size, origin, scale, p.reshape(-1, 3))
        vv = (v * v).sum(-1)
        # NaN, -inf (the all-blocked map), a velocity or an acceleration that is not finite
        if not ((d > -np.inf).all() and np.isfinite(vv).all() and np.isfinite((a * a).sum(-1)).all()):
            pc[b], gC[b], gT[b] = np.nan, np.nan, np.nan
            continue
        d, gd = d.reshape(N, res), gd.reshape(N, res, 3)
        g = (clearance - d) + vv / (2.0 * a_brake)
        kappa = np.full_like(vv, 1.0 / a_brake)
        if t_react > 0.0:
            s_eps = np.sqrt(vv + speed_eps ** 2)
            g = g + t_react * s_eps
            kappa = kappa + t_react / s_eps
        f, df = smoothed_l1(g, mu)
        Phi, F = w * f, -w * df[..., None] * gd
        G = (w * df * kappa)[..., None] * v
        step = T[b] / res
        pc[b] = step * Phi.sum(1)
        share_G = np.einsum("ija,ijk->iak", G, k[None, None, :] * tau[:, :, None] ** powers_m1)
        gC[b] = step[:, None, None] * (np.einsum("ija,ijk->iak", F, tau[:, :, None] ** powers) + share_G)
        gC_G[b] = step[:, None, None] * share_G
        gT[b] = Phi.sum(1) / res + step * (sigma[None, :] * ((F * v).sum(-1) + (G * a).sum(-1))).sum(1)
        g_all[b] = g
    return (pc, gC, gT, gC_G, g_all) if parts else (pc, gC, gT)


def j_stop(co, T, res, w, mu, clearance, a_brake, t_react, speed_eps, sd2, size, origin, scale):
    """J_stop per trajectory (B,)."""
    return j_stop_grads(co, T, res, w, mu, clearance, a_brake, t_react, speed_eps, sd2, size, origin, scale)[0].sum(1)


def sample_states(co, T, res, sd2, size, origin, scale):
    """d, |v|, v.v and tau at sigma = j / res, j = 0..res of every piece: (B, N, res + 1) each."""
    B, N = T.shape
    out = np.empty((4, B, N, res + 1))
    for b in range(B):
        sigma = np.arange(res + 1, dtype=np.float64) / np.float64(res)
        tau = sigma[None, :] * T[b][:, None]
        p, v = horner(co[b][:, None, :, :], tau[:, :, None])
        vv = (v * v).sum(-1)
        out[0, b] = query(sd2, size, origin, scale, p.reshape(-1, 3))[0].reshape(N, res + 1)
        out[1, b], out[2, b], out[3, b] = np.sqrt(vv), vv, tau
    return out


def stop_margin(co, T, res, clearance, a_brake, t_react, sd2, size, origin, scale, per_sample=False):
    """-> margin, t, speed, dist (B, N): the least d - clearance - t_react |v| - v.v / (2 a_brake) over j = 0..res, the first j on
    ties, with the local time, |v| and d there; NaN for a piece with a non-finite coefficient or duration or a duration <= 0.
    per_sample=True: the (B, N, res + 1) values instead."""
    d, speed, vv, tau = sample_states(co, T, res, sd2, size, origin, scale)
    m = ((d - clearance) - t_react * speed) - vv / (2.0 * a_brake)
    if per_sample:
        return m
    j = np.argmin(np.where(np.isnan(m), -np.inf, m), axis=2)
    take = lambda x: np.take_along_axis(x, j[..., None], 2)[..., 0]
    out = [take(m), take(tau), take(speed), take(d)]
    bad = ~(np.isfinite(co).all((2, 3)) & np.isfinite(T) & (T > 0.0)) | np.isnan(m).any(2)
    for o in out:
        o[bad] = np.nan
    return tuple(out)
