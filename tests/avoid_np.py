"""A vectorised float64 restatement of the trajectory-avoidance penalty (include/allocnet_amd.h, anet_minco_avoid_partial_grads_dev):
J_avoid per piece, its partial gradients w.r.t. the coefficients, the durations and the start time, with the header's sampling and
location rule on the same doubles -- sigma = j / res, tau = sigma * T_i, t = K_i + tau, one rounding each; knots summed in piece
order; L_m <= t < L_(m+1).  Trajectory-major arrays: co (B, N, 3, D), T (B, N), t0 (B,) or None; oco (Bo, No, 3, D), oT (Bo, No),
ot0 (Bo,) or None; the lists in CSR form."""
import numpy as np


def knots(T, t0=0.0):
    """K_0 = t0, K_(i+1) = K_i + T_i, summed in piece order (np.cumsum adds sequentially)."""
    return np.cumsum(np.concatenate([[t0], np.asarray(T, dtype=np.float64)]))


def horner(c, x):
    """c (..., D) with column col holding the power D - 1 - col, x (...): value and first derivative."""
    p, v = c[..., 0], np.zeros_like(x)
    for col in range(1, c.shape[-1]):
        v = v * x + p
        p = p * x + c[..., col]
    return p, v


def smoothed_l1(x, mu):
    """firi::smoothedL1: 0 below 0, x - mu / 2 above mu, the quartic blend between; value and slope."""
    xd = x / mu
    mid = (x >= 0.0) & (x <= mu)
    f = np.where(x > mu, x - 0.5 * mu, np.where(mid, (mu - 0.5 * x) * xd ** 3, 0.0))
    df = np.where(x > mu, 1.0, np.where(mid, xd ** 2 * (3.0 * (mu - 0.5 * x) / mu - 0.5 * xd), 0.0))
    return f, df


def sample_times(T, t0, res):
    """sigma (res,), tau (N, res), t (N, res) of one ego."""
    sigma = np.arange(res, dtype=np.float64) / np.float64(res)
    tau = sigma[None, :] * T[:, None]
    return sigma, tau, knots(T, t0)[:-1, None] + tau


def locate(t, L):
    """t (...), L (No + 1,) -> piece index m with L_m <= t < L_(m+1) (-1: the other is not there) and u = t - L_m."""
    m_at = np.full(t.shape, -1)
    for m in range(len(L) - 1):
        m_at = np.where((t >= L[m]) & (t < L[m + 1]), m, m_at)
    return m_at, t - L[np.maximum(m_at, 0)]


def ego_terms(co_b, T_b, t0_b, oco, oT, ot0, nb, res, z_scale):
    """Every (neighbour, piece, sample) term of one ego: q, the difference r, the other's velocity, `there`; and the ego's
    sigma, tau, velocity.  Shapes (n, N, res[, 3])."""
    sigma, tau, t = sample_times(T_b, t0_b, res)
    pb, vb = horner(co_b[:, None, :, :], tau[:, :, None])                       # (N, res, 3)
    n = len(nb)
    r, vo = np.zeros((n,) + pb.shape), np.zeros((n,) + pb.shape)
    there = np.zeros((n,) + t.shape, dtype=bool)
    for k, o in enumerate(nb):
        m_at, u = locate(t, knots(oT[o], 0.0 if ot0 is None else ot0[o]))
        po, vo[k] = horner(oco[o][np.maximum(m_at, 0)], u[:, :, None])
        r[k], there[k] = pb[None] - po, m_at >= 0
    q = r[..., 0] ** 2 + r[..., 1] ** 2 + (r[..., 2] / z_scale) ** 2
    return dict(q=q, r=r, vo=vo, there=there, sigma=sigma, tau=tau, vb=vb)


def all_q(co, T, t0, oco, oT, ot0, nbr_start, nbr, res, z_scale):
    """q of every (sample, neighbour) term at which the neighbour is there, over the whole batch (what the limits are chosen from)."""
    out = []
    for b in range(len(T)):
        tm = ego_terms(co[b], T[b], 0.0 if t0 is None else t0[b], oco, oT, ot0, nbr[nbr_start[b]:nbr_start[b + 1]], res, z_scale)
        out.append(tm["q"][tm["there"]])
    return np.concatenate(out) if out else np.zeros(0)


def limits_from(q):
    """min_dist^2 at the 40th percentile of q, mu a tenth of the spread to the 60th: (min_dist, mu, the active fraction)."""
    d2, hi = np.percentile(q, 40), np.percentile(q, 60)
    return float(np.sqrt(d2)), float(0.1 * (hi - d2)), float((q < d2).mean())


def ego_bad(T_b, t0_b):
    K = knots(T_b, t0_b)
    return not (np.isfinite(T_b).all() and np.isfinite(K).all() and (T_b > 0.0).all())


def other_bad(oT_o, ot0_o):
    return not (np.isfinite(oT_o).all() and np.isfinite(knots(oT_o, ot0_o)).all() and (oT_o >= 0.0).all())


def j_avoid_grads(co, T, t0, oco, oT, ot0, nbr_start, nbr, res, w, mu, min_dist, z_scale=1.0):
    """-> piece_cost (B, N), gdC (B, N, 3, D), gdT (B, N), gd_t0 (B,)."""
    B, N, _, D = co.shape
    Bo = len(oT)
    pc, gC, gT, g0 = np.zeros((B, N)), np.zeros((B, N, 3, D)), np.zeros((B, N)), np.zeros(B)
    powers = (D - 1 - np.arange(D))[None, None, :]
    for b in range(B):
        nb = np.asarray(nbr[nbr_start[b]:nbr_start[b + 1]])
        t0_b = 0.0 if t0 is None else t0[b]
        if ego_bad(T[b], t0_b) or ((nb < 0) | (nb >= Bo)).any() or any(other_bad(oT[o], 0.0 if ot0 is None else ot0[o]) for o in nb):
            pc[b], gC[b], gT[b], g0[b] = np.nan, np.nan, np.nan, np.nan
            continue
        tm = ego_terms(co[b], T[b], t0_b, oco, oT, ot0, nb, res, z_scale)
        f, df = smoothed_l1(min_dist ** 2 - tm["q"], mu)
        f, df = np.where(tm["there"], f, 0.0), np.where(tm["there"], df, 0.0)
        rt = tm["r"] * np.array([1.0, 1.0, 1.0 / z_scale ** 2])
        fo = -2.0 * w * df[..., None] * rt                                        # (n, N, res, 3)
        Phi, F, G = w * f.sum(0), fo.sum(0), (fo * tm["vo"]).sum(-1).sum(0)       # (N, res), (N, res, 3), (N, res)
        step = T[b] / res
        pc[b] = step * Phi.sum(1)
        gC[b] = step[:, None, None] * np.einsum("ija,ijk->iak", F, tm["tau"][:, :, None] ** powers)
        S = -step * G.sum(1)
        suffix = np.concatenate([np.cumsum(S[::-1])[::-1][1:], [0.0]])
        gT[b] = Phi.sum(1) / res + step * (tm["sigma"][None, :] * ((F * tm["vb"]).sum(-1) - G)).sum(1) + suffix
        g0[b] = S.sum()
    return pc, gC, gT, g0


def j_avoid(co, T, t0, oco, oT, ot0, nbr_start, nbr, res, w, mu, min_dist, z_scale=1.0):
    """J_avoid per ego (B,)."""
    return j_avoid_grads(co, T, t0, oco, oT, ot0, nbr_start, nbr, res, w, mu, min_dist, z_scale)[0].sum(1)


def discontinuous_case(s=3):
    """Ego and other share their knots; the other jumps by 1 m at every knot.  With min_dist = 1.2 m and the other 0.5 m to the
    side on its first piece, 1.5 m on its second, the samples of ego piece 1 cost nothing -- j = 0 included, which sits on the knot
    and sees the piece that STARTS there."""
    D = 2 * s
    T = np.array([[0.7, 1.1, 0.3]])
    co, oco = np.zeros((1, 3, 3, D)), np.zeros((1, 3, 3, D))
    co[0, :, 0, -2] = 1.0                       # x = tau on every piece, y = 0
    oco[0, :, 0, -2] = 1.0
    oco[0, :, 1, -1] = [0.5, 1.5, 0.5]
    return co, T, np.array([0.25]), oco, T.copy(), np.array([0.25]), np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), \
        dict(res=4, w=10.0, mu=0.05, min_dist=1.2, z_scale=1.0)
