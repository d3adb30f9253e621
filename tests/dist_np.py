"""A float64 / integer restatement of the distance field of the voxel map, its query and the obstacle penalty (include/allocnet_amd.h:
anet_voxel_distance_dev, anet_voxel_distance_query_dev, anet_minco_obstacle_partial_grads_dev).  Voxel arrays are indexed
[x, y, z] here; `flat` / `unflat` turn them into the x-fastest layout of the device and back.  Trajectory-major arrays as in
tests/avoid_np.py: co (B, N, 3, D), T (B, N)."""
import numpy as np

from tests.avoid_np import horner, smoothed_l1

NONE = 2 ** 31 - 1


def flat(a):
    """[x, y, z] -> the device layout (x fastest)."""
    return np.ascontiguousarray(np.transpose(a, (2, 1, 0))).reshape(-1)


def unflat(v, size):
    return np.transpose(np.asarray(v).reshape(size[2], size[1], size[0]), (2, 1, 0))


# ---------------------------------------------------------------------------------------------
# the field
# ---------------------------------------------------------------------------------------------
def brute_sd2(vox, walls):
    """The definition, by brute force over all pairs: vox [x, y, z] (!= 0 blocked) -> int64 sd2 [x, y, z]."""
    vox = np.asarray(vox)
    size = vox.shape
    blocked = vox != 0
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in size], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    b = blocked.reshape(-1)
    out = np.empty(len(idx), dtype=np.int64)

    def nearest(src, dst):
        if not len(src):
            return np.full(len(dst), NONE, dtype=np.int64)
        best = np.full(len(dst), NONE, dtype=np.int64)
        for lo in range(0, len(src), 64):                               # (dst, chunk of src, 3) at a time
            d = dst[:, None, :] - src[None, lo:lo + 64, :]
            best = np.minimum(best, (d * d).sum(-1).min(1))
        return best
    free_d = nearest(idx[b], idx[~b])
    if walls:
        edge = np.minimum(idx[~b] + 1, np.array(size)[None, :] - idx[~b]).min(1)
        free_d = np.minimum(free_d, edge * edge)
    out[~b] = free_d
    out[b] = -nearest(idx[~b], idx[b])
    return out.reshape(size)


def _pass(s, axis, walls):
    """One pass of the hint: g+ = max(s, 0), g- = max(-s, 0), both lower envelopes out[i] = min_j g[j] + (i - j)^2 along `axis`
    (walls: two virtual sources of g+ with value 0 at -1 and `size`), the signed pair's nonzero member back."""
    s = np.moveaxis(s, axis, -1)
    L = s.shape[-1]
    i = np.arange(L, dtype=np.int64)
    d2 = (i[:, None] - i[None, :]) ** 2                                  # [i, j]

    def env(g):
        fin = g < NONE
        cand = np.where(fin[..., None, :], np.where(fin, g, 0)[..., None, :] + d2, NONE)
        return cand.min(-1)
    gp, gm = env(np.maximum(s, 0)), env(np.maximum(-s, 0))
    if walls:
        gp = np.minimum(gp, np.minimum(i + 1, L - i) ** 2)
    return np.moveaxis(np.where(s > 0, gp, -gm), -1, axis)


def separable_sd2(vox, walls):
    """The three passes on one signed array, as the device runs them."""
    s = np.where(np.asarray(vox) != 0, -NONE, NONE).astype(np.int64)
    for axis in range(3):
        s = _pass(s, axis, walls)
    return s


# ---------------------------------------------------------------------------------------------
# the query
# ---------------------------------------------------------------------------------------------
def centre_values(sd2, scale):
    """D(v) = scale sgn(sd2) sqrt(|sd2|), +-inf for a sentinel."""
    sd2 = np.asarray(sd2, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        D = scale * np.sign(sd2) * np.sqrt(np.abs(sd2).astype(np.float64))
    return np.where(np.abs(sd2) == NONE, np.sign(sd2) * np.inf, D)


def cell_of(pos, size, origin, scale):
    """u, i0, i1, f, moves per axis, (n, 3) each: u = (p - oc) / scale, i0 = clamp(floor(u), 0, max(size - 2, 0)),
    f = clamp(u - i0, 0, 1), i1 = min(i0 + 1, size - 1); moves: f was not clamped and size > 1."""
    size = np.asarray(size, dtype=np.int64)
    oc = np.asarray(origin, dtype=np.float64) + 0.5 * scale
    with np.errstate(invalid="ignore"):
        u = (np.asarray(pos, dtype=np.float64) - oc) / scale
        fl = np.minimum(np.maximum(np.floor(u), 0.0), np.maximum(size - 2, 0).astype(np.float64))
        fr = u - fl
        f = np.minimum(np.maximum(fr, 0.0), 1.0)
        moves = (fr >= 0.0) & (fr <= 1.0) & (size > 1)
    i0 = np.where(np.isfinite(fl), fl, 0).astype(np.int64)
    return u, i0, np.minimum(i0 + 1, size - 1), f, moves


def query(sd2, size, origin, scale, pos):
    """sd2 [x, y, z]; pos (n, 3) -> dist (n,), grad (n, 3), exactly as the header states the query."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    D = centre_values(sd2, scale)
    _, i0, i1, f, moves = cell_of(pos, size, origin, scale)
    ix, iy, iz = [(i0[:, a], i1[:, a]) for a in range(3)]
    c = np.empty((len(pos), 2, 2, 2))
    for a in range(2):
        for b in range(2):
            for k in range(2):
                c[:, a, b, k] = D[ix[a], iy[b], iz[k]]
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(invalid="ignore"):
        cx = c[:, 0] * (1.0 - fx)[:, None, None] + c[:, 1] * fx[:, None, None]            # [y, z]
        cy = cx[:, 0] * (1.0 - fy)[:, None] + cx[:, 1] * fy[:, None]                      # [z]
        dist = cy[:, 0] * (1.0 - fz) + cy[:, 1] * fz
        ex = c[:, 1] - c[:, 0]
        gx = (ex[:, 0, 0] * (1 - fy) + ex[:, 1, 0] * fy) * (1 - fz) + (ex[:, 0, 1] * (1 - fy) + ex[:, 1, 1] * fy) * fz
        ey = cx[:, 1] - cx[:, 0]
        gy = ey[:, 0] * (1 - fz) + ey[:, 1] * fz
        gz = cy[:, 1] - cy[:, 0]
        grad = np.stack([gx, gy, gz], axis=1) / scale
    grad = np.where(moves, grad, 0.0)
    sentinel = np.isinf(c).any(axis=(1, 2, 3))
    dist = np.where(sentinel, c[:, 0, 0, 0], dist)
    grad[sentinel] = 0.0
    bad = ~np.isfinite(pos).all(1)
    dist[bad] = np.nan
    grad[bad] = np.nan
    return dist, grad


# ---------------------------------------------------------------------------------------------
# the penalty
# ---------------------------------------------------------------------------------------------
def sample_points(co_b, T_b, res):
    """sigma (res,), tau (N, res), p and v (N, res, 3) of one trajectory: sigma = j / res, tau = sigma * T_i, one rounding each."""
    sigma = np.arange(res, dtype=np.float64) / np.float64(res)
    tau = sigma[None, :] * T_b[:, None]
    p, v = horner(co_b[:, None, :, :], tau[:, :, None])
    return sigma, tau, p, v


def all_d(co, T, res, sd2, size, origin, scale):
    """d of every sample of the batch (what the limits are chosen from) and the least distance of a sample coordinate to a lattice
    plane, in voxels."""
    d, off = [], []
    for b in range(len(T)):
        _, _, p, _ = sample_points(co[b], T[b], res)
        d.append(query(sd2, size, origin, scale, p.reshape(-1, 3))[0])
        u = cell_of(p.reshape(-1, 3), size, origin, scale)[0]
        off.append(np.abs(u - np.round(u)).min())
    return np.concatenate(d), min(off)


def limits_from(d):
    """clearance at the 60th percentile of d, mu 0.3 of the spread to the 30th: (clearance, mu, the active fraction)."""
    cl, lo = np.percentile(d, 60), np.percentile(d, 30)
    return float(cl), float(0.3 * (cl - lo)), float((d < cl).mean())


def j_obs_grads(co, T, res, w, mu, clearance, sd2, size, origin, scale):
    """-> piece_cost (B, N), gdC (B, N, 3, D), gdT (B, N)."""
    B, N, _, D = co.shape
    pc, gC, gT = np.zeros((B, N)), np.zeros((B, N, 3, D)), np.zeros((B, N))
    powers = (D - 1 - np.arange(D))[None, None, :]
    for b in range(B):
        if not (np.isfinite(T[b]).all() and (T[b] > 0.0).all()):
            pc[b], gC[b], gT[b] = np.nan, np.nan, np.nan
            continue
        sigma, tau, p, v = sample_points(co[b], T[b], res)
        d, gd = query(sd2, size, origin, scale, p.reshape(-1, 3))
        if not (d > -np.inf).all():                                       # NaN: a non-finite position; -inf: the all-blocked map
            pc[b], gC[b], gT[b] = np.nan, np.nan, np.nan
            continue
        d, gd = d.reshape(N, res), gd.reshape(N, res, 3)
        f, df = smoothed_l1(clearance - d, mu)
        Phi, F = w * f, -w * df[..., None] * gd
        step = T[b] / res
        pc[b] = step * Phi.sum(1)
        gC[b] = step[:, None, None] * np.einsum("ija,ijk->iak", F, tau[:, :, None] ** powers)
        gT[b] = Phi.sum(1) / res + step * (sigma[None, :] * (F * v).sum(-1)).sum(1)
    return pc, gC, gT


def j_obs(co, T, res, w, mu, clearance, sd2, size, origin, scale):
    """J_obs per trajectory (B,)."""
    return j_obs_grads(co, T, res, w, mu, clearance, sd2, size, origin, scale)[0].sum(1)
