"""The floor under tests/test_costgrad_envelope_gpu.py: on every edge-input family of tests/edge_problems.py the two
independent float64 restatements of cost + gradient -- oracle/minco_np.py (dense pivoted solve, classic adjoint) and
oracle/minco_costgrad.c (banded LU, through cbind.minco_cost_grad_batch) -- agree to 1e-9 (measured: <= 7.5e-11, worst
near a spread of 100), so the C port can judge bars of 1e-9 and looser.  A family the references themselves cannot
resolve fails here, before any kernel is blamed.  Also the generators' own promises."""
import numpy as np
import pytest

from oracle import cbind
from oracle import minco_np as onp
from tests import edge_problems as ep

SHAPES = [(4, 3, 8, 16), (3, 3, 16, 12)]
B = 12
RES = 7


def _numpy_cost_grad(s, head, tail, wps, T, hp, kw):
    cost = np.empty(len(T)); gP = np.empty_like(wps); gT = np.empty_like(T); pen = np.empty(len(T))
    for b in range(len(T)):
        hpb = np.transpose(hp[b], (1, 2, 0))
        co, e, *_ = onp.minco_dense_solve(s, head[b], tail[b], wps[b].T, T[b])
        jp, gC, gTp, _ = onp.penalty_partials(s, co, T[b], hpb, **kw)
        eC, eT = onp.energy_partials(s, co, T[b])
        p, t = onp.minco_dense_propagate(s, head[b], tail[b], wps[b].T, T[b], gC + eC, gTp + eT + ep.RHO)
        cost[b] = e + ep.RHO * T[b].sum() + jp; gP[b] = p.T; gT[b] = t; pen[b] = jp
    return cost, gP, gT, pen


@pytest.mark.parametrize("s,c,N,M", SHAPES)
@pytest.mark.parametrize("family", ep.FAMILIES)
def test_the_two_float64_references_agree_on_every_family(family, s, c, N, M):
    head, tail, wps, T, hp = ep.make(family, 0, B, N, c, M)
    kw = ep.penalty_kw(family, RES)
    c0, gP0, gT0, pen = _numpy_cost_grad(s, head, tail, wps, T, hp, kw)
    c1, gP1, gT1 = cbind.minco_cost_grad_batch(s, head, tail, wps, T, hp, ep.RHO, **kw)
    assert np.isfinite(c1).all() and np.isfinite(gP1).all() and np.isfinite(gT1).all()
    ec = np.abs(c0 - c1) / np.abs(c1)
    eP = np.abs(gP0 - gP1).reshape(B, -1).max(axis=1) / np.maximum(1.0, np.abs(gP1).reshape(B, -1).max(axis=1))
    eT = np.abs(gT0 - gT1).max(axis=1) / np.maximum(1.0, np.abs(gT1).max(axis=1))
    print(f"{family} s={s} N={N}: cost {ec.max():.1e} gradP {eP.max():.1e} gradT {eT.max():.1e} active {(pen > 0).sum()}/{B}")
    assert ec.max() <= 1e-9 and eP.max() <= 1e-9 and eT.max() <= 1e-9
    if family in ep.NO_PENALTY:
        assert (pen == 0).all()
    else:
        assert 2 * (pen > 0).sum() >= B       # the penalty really is active on at least half of the compared trajectories


@pytest.mark.parametrize("family", ep.FAMILIES)
def test_realised_duration_spread(family):
    for (s, c, N, M) in SHAPES:
        T = ep.make(family, 0, 48, N, c, M)[3]
        sp = ep.spread_of(T)
        assert (T > 0).all()
        if family == "alternating":
            assert np.allclose(sp, 50.0, rtol=1e-14)
            assert (np.diff(T, axis=1) != 0).all() and set(np.unique(T)) == {ep.ALT_SHORT, ep.ALT_LONG}
        elif family in ep.SPREAD_H:
            # inside the nominal bound 10^(2h), and the family really reaches the upper half of it (in decades)
            assert (sp <= ep.SPREAD_BOUND[family]).all() and sp.max() >= ep.SPREAD_BOUND[family] ** 0.75
        else:
            k = ep.SCALE_K.get(family, 1.0)
            assert (sp <= 4.0).all() and (T >= 0.5 * k).all() and (T <= 2.0 * k).all()


@pytest.mark.parametrize("family", ["offset1e2", "offset1e4"])
def test_offset_moves_the_polytopes_with_the_positions(family):
    """The same seed without the translation is the generator's own draw: A p - b of every piece's end points is unchanged."""
    import allocnet_amd.synth as synth
    for (s, c, N, M) in SHAPES:
        head, tail, wps, T, hp = ep.make(family, 0, B, N, c, M)
        h0, t0, w0, T0, hp0 = synth.corridor_problem(ep._rng(family, 0, N, c, M), B, N, c, M)
        d = ep.OFFSET_D[family]
        assert np.allclose(head[:, :, 0] - h0[:, :, 0], d, rtol=0, atol=1e-9) and np.allclose(wps - w0, d, rtol=0, atol=1e-9)
        assert np.array_equal(T, T0) and np.array_equal(hp[..., :3], hp0[..., :3])
        assert np.abs(ep.slack(head, tail, wps, hp) - ep.slack(h0, t0, w0, hp0)).max() <= 1e-9
        assert (hp[..., 3][np.abs(hp[..., :3]).sum(axis=-1) == 0] == 0).all()        # padding rows stay padding


def test_degenerate_geometry_is_what_it_says():
    for (s, c, N, M) in SHAPES:
        head, tail, wps, T, hp = ep.make("hover", 0, B, N, c, M)
        pts = ep._points(head, tail, wps)
        seg = np.linalg.norm(np.diff(pts, axis=1), axis=2)
        assert (seg[:, N // 2] == 0).all() and (np.delete(seg, N // 2, axis=1) > 0.1).all()
        head, tail, wps, T, hp = ep.make("stationary", 0, B, N, c, M)
        pts = ep._points(head, tail, wps)
        assert (pts == pts[:, :1]).all() and (head[:, :, 1:] == 0).all() and (tail[:, :, 1:] == 0).all()
        assert (ep.slack(head, tail, wps, hp)[..., :6] == -1.0).all()
        head, tail, wps, T, hp = ep.make("constant_velocity", 0, B, N, c, M)
        assert np.array_equal(head[:, :, 1], tail[:, :, 1]) and (head[:, :, 2:] == 0).all() and (tail[:, :, 2:] == 0).all()
        assert ep.slack(head, tail, wps, hp)[..., :6].max() <= -5.0 + 1e-9


@pytest.mark.parametrize("s,c,N,M", SHAPES)
def test_constant_velocity_has_no_energy_and_stationary_costs_its_duration(s, c, N, M):
    kw = ep.penalty_kw("constant_velocity", RES)
    head, tail, wps, T, hp = ep.make("constant_velocity", 0, B, N, c, M)
    _, en = cbind.minco_solve_batch(s, head, tail, wps, T)
    assert (np.abs(en) <= 1e-12 * ep.RHO * T.sum(axis=1)).all(), np.abs(en).max()
    cost, _, _ = cbind.minco_cost_grad_batch(s, head, tail, wps, T, hp, ep.RHO, **kw)
    assert (np.abs(cost - ep.RHO * T.sum(axis=1)) <= 1e-12 * ep.RHO * T.sum(axis=1)).all()
    head, tail, wps, T, hp = ep.make("stationary", 0, B, N, c, M)
    cost, gP, gT = cbind.minco_cost_grad_batch(s, head, tail, wps, T, hp, ep.RHO, **kw)
    # (zero energy and penalty exactly; the sum of N durations to its own rounding, whatever the order)
    assert (np.abs(cost - ep.RHO * T.sum(axis=1)) <= N * 2.0 ** -52 * cost).all() and (gP == 0).all() and (gT == ep.RHO).all()
