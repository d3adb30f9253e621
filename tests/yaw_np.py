"""A float64 numpy restatement of the yaw term, its sampled margin, the evaluation of psi / dpsi and the one-axis MINCO
(include/allocnet_amd.h: anet_minco_yaw_partial_grads_dev, anet_traj_yaw_margin[_dev], anet_traj_states_yaw,
anet_minco_solve_scalar[_dev]).  Trajectory-major arrays: co (B, N, 3, D), cy (B, N, DY), T (B, N).  The one-axis MINCO is the dense
collocation solve of oracle/minco_np.py, called with the yaw data in axis 0 and zeros in the other two."""
from math import factorial

import numpy as np

from tests.avoid_np import smoothed_l1


def horner3(c, x):
    """c (..., D) with column col holding the power D - 1 - col, x (...): value, first and second derivative."""
    p, v, h = c[..., 0], np.zeros_like(x), np.zeros_like(x)
    for col in range(1, c.shape[-1]):
        h = h * x + v
        v = v * x + p
        p = p * x + c[..., col]
    return p, v, 2.0 * h


def samples(co_b, cy_b, T_b, res, end=False):
    """sigma (n,), tau (N, n), h and a (N, n, 2) of the position (x and y), psi, dpsi, ddpsi (N, n) of one trajectory at
    sigma = j / res, tau = sigma * T_i, j < res (end: j <= res)."""
    sigma = np.arange(res + (1 if end else 0), dtype=np.float64) / np.float64(res)
    tau = sigma[None, :] * T_b[:, None]
    _, h, a = horner3(co_b[:, None, :2, :], tau[:, :, None])
    psi, dpsi, ddpsi = horner3(cy_b[:, None, :], tau)
    return sigma, tau, h, a, psi, dpsi, ddpsi


def energy(cy_b, T_b, sy):
    """int (psi^(sy))^2 per piece (N,), its gradient in the coefficients (N, DY) and in the durations (N,)."""
    N, DY = cy_b.shape
    E, gC, gT = np.zeros(N), np.zeros((N, DY)), np.zeros(N)
    f = {j: factorial(j) / factorial(j - sy) for j in range(sy, DY)}
    for i in range(N):
        top = 0.0
        for j in range(sy, DY):
            cj = cy_b[i, DY - 1 - j]
            top += f[j] * cj * T_b[i] ** (j - sy)
            for k in range(sy, DY):
                e = j + k - 2 * sy + 1
                w = f[j] * f[k] * T_b[i] ** e / e
                E[i] += w * cj * cy_b[i, DY - 1 - k]
                gC[i, DY - 1 - j] += 2.0 * w * cy_b[i, DY - 1 - k]
        gT[i] = top * top
    return E, gC, gT


def look_rate_g(co_b, cy_b, T_b, res, half_fov, speed_eps, max_rate):
    """g_look, g_rate (N, res) of one trajectory."""
    _, _, h, _, psi, dpsi, _ = samples(co_b, cy_b, T_b, res)
    s_eps = np.sqrt((h * h).sum(-1) + speed_eps ** 2)
    return np.cos(half_fov) * s_eps - (h[..., 0] * np.cos(psi) + h[..., 1] * np.sin(psi)), dpsi ** 2 - max_rate ** 2


def j_yaw_grads(co, cy, T, res, w_look, mu_look, half_fov, speed_eps, w_rate, mu_rate, max_rate, w_energy, parts=False):
    """-> piece_cost (B, N), gdC (B, N, 3, D), gdCy (B, N, DY), gdT (B, N); parts=True adds g_look, g_rate (B, N, res)."""
    B, N, _, D = co.shape
    DY = cy.shape[-1]
    pc, gC, gCy, gT = np.zeros((B, N)), np.zeros((B, N, 3, D)), np.zeros((B, N, DY)), np.zeros((B, N))
    gl_all, gr_all = np.full((B, N, res), np.nan), np.full((B, N, res), np.nan)
    k, ky = D - 1 - np.arange(D), DY - 1 - np.arange(DY)
    ca = np.cos(half_fov)
    for b in range(B):
        def nan_out():
            pc[b], gC[b], gCy[b], gT[b] = np.nan, np.nan, np.nan, np.nan
        if not (np.isfinite(T[b]).all() and (T[b] > 0.0).all() and np.isfinite(co[b]).all() and np.isfinite(cy[b]).all()):
            nan_out()
            continue
        sigma, tau, h, a, psi, dpsi, ddpsi = samples(co[b], cy[b], T[b], res)
        if not all(np.isfinite(x).all() for x in (h, a, psi, dpsi, ddpsi)):
            nan_out()
            continue
        Phi = np.zeros((N, res))
        G, A, R = np.zeros((N, res, 2)), np.zeros((N, res)), np.zeros((N, res))
        sn, cs = np.sin(psi), np.cos(psi)
        if w_look > 0.0:
            s_eps = np.sqrt((h * h).sum(-1) + speed_eps ** 2)
            g = ca * s_eps - (h[..., 0] * cs + h[..., 1] * sn)
            f, df = smoothed_l1(g, mu_look)
            Phi += w_look * f
            G = (w_look * df)[..., None] * (ca * h / s_eps[..., None] - np.stack([cs, sn], -1))
            A = w_look * df * (h[..., 0] * sn - h[..., 1] * cs)
            gl_all[b] = g
        if w_rate > 0.0:
            g = dpsi ** 2 - max_rate ** 2
            f, df = smoothed_l1(g, mu_rate)
            Phi += w_rate * f
            R = w_rate * df * 2.0 * dpsi
            gr_all[b] = g
        step = T[b] / res
        pc[b] = step * Phi.sum(1)
        tk = lambda kk: tau[:, :, None] ** kk[None, None, :]
        tk1 = lambda kk: kk[None, None, :] * tau[:, :, None] ** np.maximum(kk - 1, 0)[None, None, :]
        gC[b, :, :2] = step[:, None, None] * np.einsum("ija,ijk->iak", G, tk1(k))
        gCy[b] = step[:, None] * (np.einsum("ij,ijk->ik", A, tk(ky)) + np.einsum("ij,ijk->ik", R, tk1(ky)))
        gT[b] = Phi.sum(1) / res + step * (sigma[None, :] * ((G * a).sum(-1) + A * dpsi + R * ddpsi)).sum(1)
        if w_energy > 0.0:
            E, eC, eT = energy(cy[b], T[b], DY // 2)
            pc[b] += w_energy * E
            gCy[b] += w_energy * eC
            gT[b] += w_energy * eT
    return (pc, gC, gCy, gT, gl_all, gr_all) if parts else (pc, gC, gCy, gT)


def j_yaw(co, cy, T, **kw):
    """J_yaw per trajectory (B,)."""
    return j_yaw_grads(co, cy, T, **kw)[0].sum(1)


def yaw_margin(co, cy, T, res, half_fov, v_min, per_sample=False):
    """-> margin, t, rate (B, N): among the samples j = 0..res with |h| >= v_min the least half_fov - |atan2(h x u, h . u)|, the
    first j on ties, with its local time (+inf and 0 without such a sample; a sample at rest counts at v_min = 0 with the angle 0); the largest |dpsi| over all samples.  NaN for a piece
    with a non-finite coefficient or duration or a duration <= 0.  per_sample=True: the (B, N, res + 1) margins and speeds."""
    B, N = T.shape
    m, hn, tau, rate = (np.empty((B, N, res + 1)) for _ in range(4))
    for b in range(B):
        _, tau[b], h, _, psi, dpsi, _ = samples(co[b], cy[b], T[b], res, end=True)
        sn, cs = np.sin(psi), np.cos(psi)
        hn[b] = np.sqrt(h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1])
        ang = np.arctan2(h[..., 0] * sn - h[..., 1] * cs, h[..., 0] * cs + h[..., 1] * sn)
        m[b] = half_fov - np.abs(np.where(hn[b] > 0.0, ang, 0.0))             # at rest there is no direction: the angle is 0
        rate[b] = np.abs(dpsi)
    if per_sample:
        return m, hn
    mm = np.where(hn >= v_min, m, np.inf)
    j = np.argmin(np.where(np.isnan(mm), -np.inf, mm), axis=2)
    take = lambda x: np.take_along_axis(x, j[..., None], 2)[..., 0]
    margin, t, r = take(mm), take(tau), rate.max(2)
    t[np.isinf(margin)] = 0.0
    bad = ~(np.isfinite(co).all((2, 3)) & np.isfinite(cy).all(2) & np.isfinite(T) & (T > 0.0)) | np.isnan(m).any(2) | np.isnan(rate).any(2)
    for o in (margin, t, r):
        o[bad] = np.nan
    return margin, t, r


def locate(T_b, t):
    """Trajectory::locatePieceIdx."""
    idx = 0
    while idx < len(T_b) and t > T_b[idx]:
        t -= T_b[idx]
        idx += 1
    if idx == len(T_b):
        idx -= 1
        t += T_b[idx]
    return idx, t


def yaw_eval(cy, T, tq):
    """psi, dpsi (B, nq) at the absolute times tq (B, nq)."""
    B, nq = tq.shape
    psi, dpsi = np.empty((B, nq)), np.empty((B, nq))
    for b in range(B):
        for q in range(nq):
            i, tl = locate(T[b], tq[b, q])
            psi[b, q], dpsi[b, q], _ = horner3(cy[b, i], np.float64(tl))
    return psi, dpsi


def minco_scalar(s, head, tail, wps, T):
    """The one-axis MINCO as the dense collocation solve of oracle/minco_np.py: head, tail (c,), wps (N-1,), T (N,) ->
    coeffs (N, 2s) highest power first, energy."""
    from oracle import minco_np as mn
    c, N = len(head), len(T)
    h3, t3, w3 = np.zeros((3, c)), np.zeros((3, c)), np.zeros((3, N - 1))
    h3[0], t3[0], w3[0] = head, tail, wps
    out = mn.minco_dense_solve(s, h3, t3, w3, np.asarray(T, dtype=np.float64))
    return out[0][:, 0, :], out[1]


def heading_fit(co, T, sy, rng, noise=0.3):
    """Yaw coefficients (B, N, 2 sy) as a least-squares fit per piece of the unwrapped heading of the horizontal velocity plus
    noise, at 2 sy + 2 points so that the fit keeps most of the noise: what makes both terms partly active (random coefficients
    leave the look term active nearly everywhere)."""
    B, N = T.shape
    DY = 2 * sy
    n_fit = DY + 2
    cy = np.empty((B, N, DY))
    for b in range(B):
        last = None
        for i in range(N):
            tl = np.linspace(0.0, T[b, i], n_fit)
            _, h, _ = horner3(co[b, i, None, :2, :], tl[:, None])
            ang = np.arctan2(h[:, 1], h[:, 0])
            if last is not None:
                ang = np.concatenate([[last], ang])
            ang = np.unwrap(ang)
            if last is not None:
                ang = ang[1:]
            last = ang[-1]
            cy[b, i] = np.polyfit(tl, ang + noise * rng.normal(size=n_fit), DY - 1)
    return cy


def limits_for(co, cy, T, res, speed_eps):
    """half_fov, mu_look, max_rate, mu_rate by the percentile rule of dist_np.limits_from, and the active fractions of the two terms.
    limits_from takes a quantity that must stay ABOVE its limit, puts the limit at its 60th percentile and mu at 0.3 of the spread to
    the 30th; it is given the negatives of what must stay below here: the angle between h and u (its limit is half_fov, capped at
    pi / 2), then g_look at that half_fov (its limit is 0 up to eps; only mu is taken), and dpsi^2 (its limit is max_rate^2).
    One sample has no percentiles: a fixed mu (at most 0.05, and small enough for a half_fov to exist) and the sample in the middle
    of the blend, g = mu / 2, as the distance and stop tests have it."""
    from tests.dist_np import limits_from
    B = len(T)
    smp = [samples(co[b], cy[b], T[b], res) for b in range(B)]
    h = np.concatenate([x[2].reshape(-1, 2) for x in smp])
    psi = np.concatenate([x[4].reshape(-1) for x in smp])
    r2 = np.concatenate([(x[5] ** 2).reshape(-1) for x in smp])
    hu = h[:, 0] * np.cos(psi) + h[:, 1] * np.sin(psi)
    s_eps = np.sqrt((h * h).sum(-1) + speed_eps ** 2)
    if len(psi) < 2:
        mu_look = min(0.05, float(s_eps[0] - hu[0]))
        ca = (hu[0] + 0.5 * mu_look) / s_eps[0]
        assert 0.0 <= ca < 1.0, "the one sample must leave room for a half_fov in (0, pi/2]"
        half_fov = float(np.arccos(ca))
        mu_rate = min(0.05, float(r2[0]))
        max_rate = float(np.sqrt(r2[0] - 0.5 * mu_rate))
    else:
        ang = np.abs(np.arctan2(h[:, 0] * np.sin(psi) - h[:, 1] * np.cos(psi), hu))
        half_fov = min(-limits_from(-ang)[0], 0.5 * np.pi)
        mu_look = limits_from(-(np.cos(half_fov) * s_eps - hu))[1]
        mr2, mu_rate, _ = limits_from(-r2)
        max_rate = float(np.sqrt(-mr2))
    g_look = np.cos(half_fov) * s_eps - hu
    frac_look, frac_rate = float((g_look > 0.0).mean()), float((r2 > max_rate ** 2).mean())
    return dict(half_fov=float(half_fov), mu_look=float(mu_look), max_rate=max_rate, mu_rate=float(mu_rate)), frac_look, frac_rate


def energy_weight(co, cy, T, kw, share=0.5):
    """w_energy that makes the effort term `share` of the look and rate terms together, so that no term drowns the others in the
    differences of J."""
    base = j_yaw(co, cy, T, **dict(kw, w_energy=0.0)).sum()
    E = sum(energy(cy[b], T[b], cy.shape[-1] // 2)[0].sum() for b in range(len(T)))
    return float(share * base / E)
