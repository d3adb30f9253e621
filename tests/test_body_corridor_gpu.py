"""The whole-body corridor terms on the GPU (anet_minco_body_partial_grads_dev, anet_traj_body_margin[_dev] and their facades) against
the torch restatement of tests/body_np.py, which stands on tests/flatness_np.py, and against identities that do not depend on it: a
body that is a point is the corridor share of anet_minco_partial_grads_dev, and a vehicle that climbs without drag keeps R = I.

Inputs: rows with |a_r| = 1, vertices with |b_k| <= 1, trajectories from minco_solve on seeded random walks slowed down into the
planner's boxes (as tests/test_flatness_gpu.py makes them), and corridor offsets taken from the sampled terms' own percentiles so that
10 to 90 % of the (sample, row, vertex) terms are active; that share is asserted.  The one-term shape (res = K = M = 1) cannot have a
share strictly between 0 and 1: its single term is made active, and that is asserted instead."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import body_np as bnp
from tests import flatness_np as fnp
from tests.util import random_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
W, MU = 7.0, 0.2
EPS = 2.220446049250313e-16


def _params(**kw):
    import allocnet_amd as aa
    return aa.make_flat_params(**kw)       # the launch file's vehicle, fnp.LAUNCH, unless told otherwise


def _bm(a, ld, fill=0.0):
    """(n, f) or (n,) numpy -> batch-minor torch tensor (f, ld) or (ld,) on the device."""
    a = np.asarray(a, dtype=np.float64)
    t = torch.full((a.shape[1] if a.ndim == 2 else 1, ld), fill, dtype=torch.float64)
    t[:, :a.shape[0]] = torch.from_numpy(a.reshape(a.shape[0], -1)).T
    t = t.to(DEV)
    return t if a.ndim == 2 else t[0]


_TRAJ = {}


def _trajectories(anet_ctx, s, N, B, seed):
    """Rest-to-rest random-walk problems, durations scaled per trajectory until the restatement's sampled |v|, |a| are inside the
    planner's boxes (zu_3 > 0 everywhere).  Computed once per key and never changed."""
    import allocnet_amd as aa
    key = (s, N, B, seed)
    if key not in _TRAJ:
        rng = np.random.default_rng(seed)
        c = min(s, 3)
        head, tail, wps, T = random_problem(rng, B, N, c, rest=True)
        T, co = fnp.scale_into_limits(lambda t: aa.minco_solve(head, tail, wps, t, s, ctx=anet_ctx)[0], T)
        _TRAJ[key] = (head, tail, wps, T, co)
    return _TRAJ[key]


def _verts(K, seed):
    """K vertices with |b_k| <= 1: a flat box for K = 8, points of the unit ball otherwise"""
    import allocnet_amd as aa
    if K == 8:
        return aa.box_body((0.5, 0.4, 0.1))
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(K, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.2, 1.0, (K, 1))


def _corridor(co, T, verts, res, M, pad, seed, lo=20.0, hi=80.0, closed=False, **par):
    """(B, N, M, 4) rows with unit normals; row (b, i, r) gets the offset at a percentile drawn from [lo, hi] of its own sampled
    terms a_r . (p + R b_k) over (sample, vertex), so that between (100 - hi) and (100 - lo) % of them are active; a row with a single
    term is shifted by mu / 2 so that the term is active.  The last `pad` rows of even pieces and the first of odd pieces are zero.
    Asserts the active share."""
    rng = np.random.default_rng(seed)
    B, N = T.shape
    hp = np.zeros((B, N, M, 4))
    a = rng.normal(size=(B, N, M, 3))
    hp[..., :3] = a / np.linalg.norm(a, axis=-1, keepdims=True)
    g = bnp.terms(co, T, hp, verts, res, closed=closed, **par)[0].numpy()          # (B, N, J, M, K), offsets still 0
    s = np.sort(np.moveaxis(g, 3, 2).reshape(B, N, M, -1), axis=-1)
    n = s.shape[-1]
    pos = rng.uniform(lo, hi, (B, N, M)) / 100.0 * (n - 1)
    i0 = np.floor(pos).astype(int)
    i1 = np.minimum(i0 + 1, n - 1)
    take = lambda i: np.take_along_axis(s, i[..., None], -1)[..., 0]
    hp[..., 3] = take(i0) + (pos - i0) * (take(i1) - take(i0)) - (0.5 * MU if n == 1 else 0.0)
    if pad:
        hp[:, 0::2, M - pad:] = 0.0
        hp[:, 1::2, :pad] = 0.0
    share, count = bnp.active_share(co, T, hp, verts, res, **par)
    print(f"active on {100 * share:.1f} % of {count} (sample, row, vertex) terms")
    assert (0.1 <= share <= 0.9) if count > 1 else share == 1.0, share
    return hp


def _pen(verts, res, M, w=W, mu=MU):
    import allocnet_amd as aa
    return aa.make_body_penalty(verts, w=w, smooth_mu=mu, res=res, poly_rows=M)


def _body_partials(anet_ctx, pen, s, N, B, co, T, hp, params=None, accumulate=False, into=None, fill=float("nan")):
    """anet_minco_body_partial_grads_dev on trajectory-major numpy inputs -> the device tensors gdC, gdT, piece_cost (whole rows,
    padding lanes included), ld and the device inputs."""
    import allocnet_amd as aa
    ld = aa.recommended_ld(B) if B > 1 else 1
    d_co, d_T, d_hp = _bm(co.reshape(B, -1), ld), _bm(T, ld, fill=1.0), _bm(hp.reshape(B, -1), ld)
    if into is None:
        into = tuple(torch.full((r, ld), fill, dtype=torch.float64, device=DEV) for r in (N * 3 * 2 * s, N, N))
    aa.minco_body_partial_grads_dev(params or _params(), pen, s, N, B, d_co, d_T, d_hp, into[0], into[1], into[2],
                                    accumulate=accumulate, ctx=anet_ctx)
    torch.cuda.synchronize()
    return into, ld, d_co, d_T, d_hp


def _point_partials(anet_ctx, s, N, B, ld, d_co, d_T, d_hp, res, M, w=W, mu=MU):
    """the corridor share of anet_minco_partial_grads_dev: no energy, no box rows, no rho"""
    import allocnet_amd as aa
    pen = aa.make_penalty(rho=0.0, w_corridor=w, w_vel=0.0, w_acc=0.0, smooth_mu=mu, res=res, poly_rows=M)
    out = tuple(torch.full((r, ld), float("nan"), dtype=torch.float64, device=DEV) for r in (N * 3 * 2 * s, N, N))
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    anet_ctx.check(anet_ctx.lib.anet_minco_partial_grads_dev(anet_ctx.handle, s, N, B, ld, q(d_co), q(d_T), q(d_hp),
                                                             ctypes.cast(ctypes.pointer(pen), ctypes.c_void_p), 0, q(out[0]),
                                                             q(out[1]), q(out[2]), st))
    torch.cuda.synchronize()
    return out


def _compare(got, ref, B, N, s, what):
    """cost at 1e-9 relative, gdC and gdT at 1e-7 relative to max(1, max |ref|), both reference gradients non-zero: the bars
    test_flat_partial_grads_match_autograd holds the sibling kernel to.  got: device tensors; ref: (pc (B, N), gdC (B, N, 3, D), gdT)."""
    gC, gT, pc = got
    rpc, rgC, rgT = ref
    cost, rcost = pc[:, :B].sum(0).cpu().numpy(), rpc.sum(1)
    rel = np.abs(cost - rcost) / np.maximum(np.abs(rcost), 1e-300)
    rel[rcost == 0.0] = np.abs(cost[rcost == 0.0])
    print(f"{what} cost: worst relative {rel.max():.3e} (bar 1e-9)")
    g = gC[:, :B].T.cpu().numpy().reshape(B, N, 3, 2 * s)
    eC = np.abs(g - rgC).max() / max(1.0, np.abs(rgC).max())
    eT = np.abs(gT[:, :B].T.cpu().numpy() - rgT).max() / max(1.0, np.abs(rgT).max())
    print(f"{what} gdC: {eC:.3e}, gdT: {eT:.3e} (bar 1e-7); |gdC| max {np.abs(rgC).max():.3e}, |gdT| max {np.abs(rgT).max():.3e}")
    assert rel.max() <= 1e-9
    assert np.abs(rgC).max() > 0.0 and np.abs(rgT).max() > 0.0
    assert eC <= 1e-7 and eT <= 1e-7


# 1 ---------------------------------------------------------------------------------------------
# (s, N, B, res, K, M, padding rows among the M)
GRAD_SHAPES = [(3, 1, 1, 1, 1, 1, 0), (3, 2, 65, 5, 8, 7, 2), (4, 3, 130, 20, 8, 16, 5), (4, 8, 70, 4, 16, 50, 30)]


@pytest.mark.parametrize("s,N,B,res,K,M,pad", GRAD_SHAPES)
def test_body_partial_grads_match_autograd(anet_ctx, s, N, B, res, K, M, pad):
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 1000 + 100 * s + N)
    verts = _verts(K, 11 + K)
    hp = _corridor(co, T, verts, res, M, pad, 17 + M)
    got, ld, _, _, _ = _body_partials(anet_ctx, _pen(verts, res, M), s, N, B, co, T, hp)
    _compare(got, bnp.j_body_grads(co, T, hp, verts, res, W, MU), B, N, s, "body")


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,N,B,res,M,pad", [(3, 2, 65, 5, 7, 2), (4, 3, 130, 20, 16, 5)])
def test_a_point_body_is_the_point_corridor_penalty(anet_ctx, s, N, B, res, M, pad):
    """K = 1, b = 0: piece_cost, gdC and gdT equal the corridor share of anet_minco_partial_grads_dev (with_energy = 0, no box rows,
    rho = 0, the same w, mu, res) -- independent of the restatement."""
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 1000 + 100 * s + N)
    verts = np.zeros((1, 3))
    hp = _corridor(co, T, verts, res, M, pad, 23 + M)
    got, ld, d_co, d_T, d_hp = _body_partials(anet_ctx, _pen(verts, res, M), s, N, B, co, T, hp)
    pC, pT, ppc = _point_partials(anet_ctx, s, N, B, ld, d_co, d_T, d_hp, res, M)
    ref = (ppc[:, :B].T.cpu().numpy(), pC[:, :B].T.cpu().numpy().reshape(B, N, 3, 2 * s), pT[:, :B].T.cpu().numpy())
    _compare(got, ref, B, N, s, "point identity")
    # ... piece by piece, not only in the sum over the pieces
    e = (got[2][:, :B] - ppc[:, :B]).abs().max().item() / max(1.0, ppc[:, :B].abs().max().item())
    print(f"piece_cost: {e:.3e} (bar 1e-9)")
    assert e <= 1e-9


# 3 ---------------------------------------------------------------------------------------------
def test_level_flight_is_the_point_penalty_per_vertex(anet_ctx):
    """horiz_drag = 0 and a trajectory that moves in z only with a_z + g > 0: zu is parallel to e3, R = I, and J_body is the sum over
    the vertices of the point penalty against the rows (a_r, h_r - a_r . b_k)."""
    import allocnet_amd as aa
    s, N, B, res, K, M = 4, 3, 70, 20, 8, 7
    rng = np.random.default_rng(31)
    head, tail, wps, T = random_problem(rng, B, N, 3, rest=True)
    head[:, :2, :] = 0.0
    tail[:, :2, :] = 0.0
    wps[:, :, :2] = 0.0
    par = dict(fnp.LAUNCH, dh=0.0)
    T, co = fnp.scale_into_limits(lambda t: aa.minco_solve(head, tail, wps, t, s, ctx=anet_ctx)[0], T, **par)
    assert np.all(co[:, :, :2, :] == 0.0)
    verts = _verts(K, 0)
    hp = _corridor(co, T, verts, res, M, 2, 37, **par)
    params = _params(horiz_drag=0.0)
    (gC, gT, pc), ld, d_co, d_T, _ = _body_partials(anet_ctx, _pen(verts, res, M), s, N, B, co, T, hp, params=params)
    ref = torch.zeros_like(pc[:, :B])
    for b in verts:
        shifted = hp.copy()
        shifted[..., 3] -= hp[..., :3] @ b               # (padding rows stay all zero: a = 0)
        ref += _point_partials(anet_ctx, s, N, B, ld, d_co, d_T, _bm(shifted.reshape(B, -1), ld), res, M)[2][:, :B]
    assert float(ref.sum()) > 0.0
    cost, rcost = pc[:, :B].sum(0).cpu().numpy(), ref.sum(0).cpu().numpy()
    rel = np.abs(cost - rcost) / np.maximum(np.abs(rcost), 1e-300)
    rel[rcost == 0.0] = np.abs(cost[rcost == 0.0])
    print(f"level flight: worst relative {rel.max():.3e} (bar 1e-9)")
    assert rel.max() <= 1e-9


# 4 ---------------------------------------------------------------------------------------------
def test_minco_body_cost_grad_finite_differences(anet_ctx):
    import allocnet_amd as aa
    s, N, B, res, K, M = 4, 4, 8, 7, 8, 7
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 41)
    verts = _verts(K, 0)
    hp = _corridor(co, T, verts, res, M, 2, 43)
    bpen = _pen(verts, res, M)
    pen = aa.make_penalty(rho=2.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=9)
    fm = aa.FlatnessMap(ctx=anet_ctx)
    f = lambda w, t: aa.minco_body_cost_grad(head, tail, w, t, s, fm, bpen, hp, penalty=pen, ctx=anet_ctx)
    cost, gP, gT = f(wps, T)
    base = aa.minco_cost_grad(head, tail, wps, T, s, penalty=pen, ctx=anet_ctx)[0]
    jb = bnp.j_body(co, T, hp, verts, res, W, MU).sum(1).numpy()
    assert (jb > 0.0).all()
    rel = np.abs(cost - (base + jb)) / np.abs(base + jb)
    print(f"cost against minco_cost_grad + J_body: worst relative {rel.max():.3e} (bar 1e-9)")
    assert rel.max() <= 1e-9
    h = 1e-6
    for (k, ax) in [(0, 0), (1, 1), (2, 2)]:
        wp = wps.copy(); wp[:, k, ax] += h; wm = wps.copy(); wm[:, k, ax] -= h
        fd = (f(wp, T)[0] - f(wm, T)[0]) / (2 * h)
        err = np.abs(fd - gP[:, k, ax]).max() / max(1.0, np.abs(gP[:, k, ax]).max())
        print(f"gradP[{k},{ax}]: {err:.3e} (bar 2e-5)")
        assert err <= 2e-5
    for i in (0, 2, 3):
        tp = T.copy(); tp[:, i] += h; tm = T.copy(); tm[:, i] -= h
        fd = (f(wps, tp)[0] - f(wps, tm)[0]) / (2 * h)
        err = np.abs(fd - gT[:, i]).max() / max(1.0, np.abs(gT[:, i]).max())
        print(f"gradT[{i}]: {err:.3e} (bar 2e-5)")
        assert err <= 2e-5


# 5 ---------------------------------------------------------------------------------------------
def test_accumulate_contract(anet_ctx):
    """accumulate = 1 after anet_minco_partial_grads_dev equals the sum of the two separate results to the last bit; lanes in
    [batch, ld) keep their poison value; accumulate = 0 overwrites NaN."""
    import allocnet_amd as aa
    s, N, B, res, K, M = 4, 3, 130, 20, 8, 16
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 1000 + 100 * s + N)
    verts = _verts(K, 0)
    hp = _corridor(co, T, verts, res, M, 5, 17 + M)
    bpen = _pen(verts, res, M)
    (fC, fT, fpc), ld, d_co, d_T, d_hp = _body_partials(anet_ctx, bpen, s, N, B, co, T, hp)          # onto NaN
    assert ld > B
    for t in (fC, fT, fpc):
        assert torch.isfinite(t[:, :B]).all() and torch.isnan(t[:, B:]).all()
    pen = aa.make_penalty(rho=0.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=res)
    eC, eT, epc = (torch.full_like(t, 123.0) for t in (fC, fT, fpc))
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    anet_ctx.check(anet_ctx.lib.anet_minco_partial_grads_dev(anet_ctx.handle, s, N, B, ld, q(d_co), q(d_T), None,
                                                             ctypes.cast(ctypes.pointer(pen), ctypes.c_void_p), 1, q(eC), q(eT), q(epc), st))
    torch.cuda.synchronize()
    sums = [e[:, :B] + f[:, :B] for e, f in ((eC, fC), (eT, fT), (epc, fpc))]
    assert float(epc[:, :B].sum()) > 0.0 and float(fpc[:, :B].sum()) > 0.0
    _body_partials(anet_ctx, bpen, s, N, B, co, T, hp, accumulate=True, into=(eC, eT, epc))
    for got, ref in zip((eC, eT, epc), sums):
        assert torch.equal(got[:, :B], ref)
        assert (got[:, B:] == 123.0).all()


# 6 ---------------------------------------------------------------------------------------------
def test_an_unreachable_corridor_costs_nothing(anet_ctx):
    s, N, B, res, K, M = 3, 2, 65, 5, 8, 7
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 1000 + 100 * s + N)
    verts = _verts(K, 0)
    hp = _corridor(co, T, verts, res, M, 2, 17 + M)
    hp[..., 3] += 1e6 * (np.abs(hp[..., :3]).sum(-1) > 0.0)
    (gC, gT, pc), _, _, _, _ = _body_partials(anet_ctx, _pen(verts, res, M), s, N, B, co, T, hp)
    for t in (gC, gT, pc):
        assert (t[:, :B] == 0.0).all()


def test_a_nan_coefficient_poisons_its_own_piece_only(anet_ctx):
    s, N, B, res, K, M = 3, 2, 65, 5, 8, 7
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 1000 + 100 * s + N)
    verts = _verts(K, 0)
    hp = _corridor(co, T, verts, res, M, 2, 17 + M)
    good = [t[:, :B].clone() for t in _body_partials(anet_ctx, _pen(verts, res, M), s, N, B, co, T, hp)[0]]
    co2 = co.copy()
    co2[7, 1, 2, 3] = np.nan
    gC, gT, pc = (t[:, :B] for t in _body_partials(anet_ctx, _pen(verts, res, M), s, N, B, co2, T, hp)[0])
    assert torch.isnan(pc[1, 7]) and torch.isnan(gT[1, 7]) and torch.isnan(gC[6 * s:12 * s, 7]).all()
    for got, ref, rows in ((gC, good[0], slice(6 * s, 12 * s)), (gT, good[1], 1), (pc, good[2], 1)):
        got, ref = got.clone(), ref.clone()
        got[rows, 7] = ref[rows, 7] = 0.0
        assert torch.equal(got, ref)


# 7 ---------------------------------------------------------------------------------------------
def _margin_scale(co, T, hp):
    """sum_ax |a_ax| sum_k |u_ax,k| + |h|, u the coefficients in normalised time, the largest over the piece's rows: (B, N)"""
    D = co.shape[-1]
    u = np.abs(co * T[:, :, None, None] ** (D - 1 - np.arange(D))).sum(-1)              # (B, N, 3)
    return (np.einsum("bnmx,bnx->bnm", np.abs(hp[..., :3]), u) + np.abs(hp[..., 3])).max(-1)


@pytest.mark.parametrize("s,N,B", [(3, 1, 1), (4, 3, 70)])
def test_body_margin(anet_ctx, s, N, B):
    import allocnet_amd as aa
    res, K, M, pad = 20, 8, 7, 2
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 700 + 10 * s + N)
    verts = _verts(K, 0)
    hp = _corridor(co, T, verts, res, M, pad, 71, closed=True)
    fm = aa.FlatnessMap(ctx=anet_ctx)
    m, t, row, vert = aa.traj_body_margin(fm, verts, co, T, hp, res, ctx=anet_ctx)
    ref, g, ts = bnp.margin(co, T, hp, verts, res)
    bar = 1e-12 * np.maximum(1.0, _margin_scale(co, T, hp))
    err = np.abs(m - ref) / bar
    print(f"margin: worst {err.max():.3e} of the bar 1e-12 max(1, scale)")
    assert err.max() <= 1.0
    # the diagnostics reproduce the margin: t is one of the samples, (row, vert) a non-padding row and a vertex
    for b in range(B):
        for i in range(N):
            assert 0 <= row[b, i] < M and 0 <= vert[b, i] < K and np.any(hp[b, i, row[b, i]] != 0.0)
            j = int(np.argmin(np.abs(ts[b, i] - t[b, i])))
            assert abs(ts[b, i, j] - t[b, i]) <= 4 * EPS * T[b, i]
            assert abs(bnp.term_at(co[b, i], t[b, i], hp[b, i, row[b, i]], verts[vert[b, i]]) - m[b, i]) <= bar[b, i]
    # the device form gives the same bits
    ld = aa.recommended_ld(B) if B > 1 else 1
    dm, dt, drow, dvert = aa.traj_body_margin_dev(fm, _pen(verts, res, M), s, N, B, _bm(co.reshape(B, -1), ld), _bm(T, ld, fill=1.0),
                                                  _bm(hp.reshape(B, -1), ld), ctx=anet_ctx)
    torch.cuda.synchronize()
    assert np.array_equal(dm[:, :B].T.cpu().numpy(), m) and np.array_equal(dt[:, :B].T.cpu().numpy(), t)
    assert np.array_equal(drow[:, :B].T.cpu().numpy(), row) and np.array_equal(dvert[:, :B].T.cpu().numpy(), vert)
    # K = 1, b = 0: the sampled maximum of the point, which the exact margin bounds
    m0 = aa.traj_body_margin(fm, np.zeros((1, 3)), co, T, hp, res, ctx=anet_ctx)[0]
    ref0 = bnp.margin(co, T, hp, np.zeros((1, 3)), res)[0]
    exact = aa.traj_row_margin(co, T, hp, 0, ctx=anet_ctx)[0]
    assert (np.abs(m0 - ref0) <= bar).all()
    assert (m0 <= exact + 32 * EPS * _margin_scale(co, T, hp) + bar).all()
    # a piece with only padding rows: -inf, for that piece only
    hp2 = hp.copy()
    hp2[0, 0] = 0.0
    m2, t2, row2, vert2 = aa.traj_body_margin(fm, verts, co, T, hp2, res, ctx=anet_ctx)
    assert m2[0, 0] == -np.inf and row2[0, 0] == -1 and vert2[0, 0] == -1 and t2[0, 0] == 0.0
    keep = np.ones((B, N), dtype=bool)
    keep[0, 0] = False
    assert np.array_equal(m2[keep], m[keep])
    # a NaN coefficient: NaN, for that piece only
    co2 = co.copy()
    co2[B - 1, N - 1, 1, 2] = np.nan
    m3, _, row3, _ = aa.traj_body_margin(fm, verts, co2, T, hp, res, ctx=anet_ctx)
    assert np.isnan(m3[B - 1, N - 1]) and row3[B - 1, N - 1] == -1
    keep = np.ones((B, N), dtype=bool)
    keep[B - 1, N - 1] = False
    assert np.array_equal(m3[keep], m[keep])
    # the Trajectory facade
    traj = aa.Trajectory([T[0, i] for i in range(N)], [co[0, i] for i in range(N)], ctx=anet_ctx)
    polys = [hp[0, i][np.any(hp[0, i] != 0.0, axis=1)] for i in range(N)]
    assert traj.getBodyMargin(fm, verts, polys, res) == m[0].max()
    assert np.array_equal(traj.getBodyMargin(fm, verts, polys, res, per_piece=True)[0], m[0])
    assert traj.checkBodyCorridor(fm, verts, polys, res, tol=m[0].max()) and not traj.checkBodyCorridor(fm, verts, polys, res, tol=m[0].max() - 1e-9)


# 8 ---------------------------------------------------------------------------------------------
def test_argument_errors(anet_ctx):
    import allocnet_amd as aa
    from allocnet_amd import _lib
    s, N, B, M = 3, 2, 4, 3
    ld = aa.recommended_ld(B)
    z = lambda r: torch.zeros(r, ld, dtype=torch.float64, device=DEV)
    co, T, hp, gC, gT, pc = z(N * 6 * s), z(N) + 1.0, z(N * M * 4), z(N * 6 * s), z(N), z(N)
    q = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ref = lambda x: ctypes.cast(ctypes.pointer(x), ctypes.c_void_p)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    par = _params()

    def grads(pen, s_=s, batch=B, hpolys=hp, coeffs=co):
        return anet_ctx.lib.anet_minco_body_partial_grads_dev(anet_ctx.handle, ref(par), ref(pen), s_, N, batch, ld, q(coeffs), q(T),
                                                              q(hpolys), 0, q(gC), q(gT), q(pc), st)

    def margin(pen, hpolys=hp):
        return anet_ctx.lib.anet_traj_body_margin_dev(anet_ctx.handle, ref(par), ref(pen), s, N, B, ld, q(co), q(T), q(hpolys), q(gT),
                                                      None, None, None, st)
    good = lambda **kw: aa.make_body_penalty(np.array([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0]]), **dict(dict(w=1.0, smooth_mu=0.1, res=5, poly_rows=M), **kw))
    assert grads(good()) == _lib.ANET_OK and margin(good()) == _lib.ANET_OK
    bad = []
    for nv in (0, 17):
        p = good(); p.n_verts = nv; bad.append(p)
    bad += [good(res=0), good(res=4097), good(poly_rows=0), good(poly_rows=51), good(smooth_mu=0.0), good(smooth_mu=-1.0)]
    for v in (np.nan, np.inf):
        p = good(); p.verts[1][2] = v; bad.append(p)
    for p in bad:
        assert grads(p) == _lib.ANET_ERR_INVALID
    for p in bad[:6] + bad[8:]:                      # (the margin does not read smooth_mu)
        assert margin(p) == _lib.ANET_ERR_INVALID
    assert grads(good(), hpolys=None) == _lib.ANET_ERR_INVALID and margin(good(), hpolys=None) == _lib.ANET_ERR_INVALID
    assert grads(good(), s_=2) == _lib.ANET_ERR_UNSUPPORTED
    assert grads(good(), s_=5) == _lib.ANET_ERR_INVALID
    assert grads(good(), coeffs=None) == _lib.ANET_ERR_INVALID
    # batch == 0: ANET_OK after the argument checks, and only after them
    assert grads(good(), batch=0, coeffs=None) == _lib.ANET_OK
    assert grads(good(res=0), batch=0) == _lib.ANET_ERR_INVALID
    with pytest.raises(ValueError):
        aa.make_body_penalty(np.zeros((17, 3)))
    torch.cuda.synchronize()


# 9 ---------------------------------------------------------------------------------------------
def test_lockstep_lbfgs_on_the_body_objective(anet_ctx):
    """lbfgs_optimize_dev on body_objective_dev from trajectories whose body leaves its corridor: every status is non-negative and
    J_body (the restatement's) ends below its start for every problem.  No target value is asserted."""
    import allocnet_amd as aa
    s, c, N, B, res, K, M = 3, 3, 3, 8, 20, 8, 7
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 91)
    verts = _verts(K, 0)
    hp = _corridor(co, T, verts, res, M, 2, 93)
    w = 1e4
    bpen = _pen(verts, res, M, w=w)
    pen = aa.make_penalty(rho=1.0, res=res)
    fm = aa.FlatnessMap(ctx=anet_ctx)
    j0 = bnp.j_body(co, T, hp, verts, res, w, MU).sum(1).numpy()
    assert (j0 > 0.0).all()
    ld = aa.recommended_ld(B)
    nw = 3 * (N - 1)
    x = torch.zeros(nw + N, ld, dtype=torch.float64, device=DEV)
    x[:nw, :B] = torch.from_numpy(wps.reshape(B, -1)).T.to(DEV)
    x[nw:, :B] = torch.from_numpy(np.log(T)).T.to(DEV)
    ev = aa.body_objective_dev(_bm(head.reshape(B, -1), ld), _bm(tail.reshape(B, -1), ld), s, c, N, B, fm, bpen,
                               _bm(hp.reshape(B, -1), ld), penalty=pen, ctx=anet_ctx)
    out = aa.lbfgs_optimize_dev(x, ev, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-5), max_evals=200, ctx=anet_ctx)
    torch.cuda.synchronize()
    status = out["status"][:B].cpu().numpy()
    print(f"status {status.tolist()}, evals {out['evals'][:B].cpu().numpy().tolist()}")
    assert (status >= 0).all()
    w1 = x[:nw, :B].T.cpu().numpy().reshape(B, N - 1, 3)
    t1 = np.exp(x[nw:, :B].T.cpu().numpy())
    co1, _ = aa.minco_solve(head, tail, w1, t1, s, ctx=anet_ctx)
    j1 = bnp.j_body(co1, t1, hp, verts, res, w, MU).sum(1).numpy()
    print("J_body", j0.tolist(), "->", j1.tolist())
    assert (j1 < j0).all()


# 10 --------------------------------------------------------------------------------------------
def test_cpp_body_corridor_program(anet_ctx):
    """tests/cpp/test_body_corridor.cpp: getBodyMargin / checkBodyCorridor of the C++ facade print the bits of the Python facade."""
    import allocnet_amd as aa
    src = os.path.join(ROOT, "tests", "cpp", "test_body_corridor.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "test_body_corridor")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads(res.stdout)
    N = 8
    goal = np.array([8.0, 3.0, 1.0])
    head = np.zeros((1, 3, 3)); tail = np.zeros((1, 3, 3)); tail[0, :, 0] = goal
    wps = (goal[None] * (np.arange(1, N)[:, None] / N))[None]
    T = np.ones((1, N))
    co, _ = aa.minco_solve(head, tail, wps, T, 4, ctx=anet_ctx)
    traj = aa.Trajectory([1.0] * N, [co[0, i] for i in range(N)], ctx=anet_ctx)
    polys = [np.array(h) for h in out["hpolys"]]
    assert [len(h) for h in polys] == [6, 7] * 4
    fm = aa.FlatnessMap(ctx=anet_ctx)
    verts = aa.box_body((0.25, 0.25, 0.05))
    per = traj.getBodyMargin(fm, verts, polys, 20, per_piece=True)[0]
    assert np.isfinite(per).all()
    assert np.array_equal(np.array(out["per_piece"]), per)
    assert out["margin"] == traj.getBodyMargin(fm, verts, polys, 20)
    assert out["check"] == [int(out["margin"] <= 0.0), 1]
