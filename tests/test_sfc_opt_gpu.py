"""GPU suite of the corridor-constrained MINCO L-BFGS (allocnet_amd/sfc_opt.py, anet_sfc_* / anet_lbfgs_minco_sfc*): overlap
vertices against anet_polytope_vertices and Qhull, the transform against the numpy restatement (tests/sfc_np.py), the composed
gradient against the CPU composition and central differences, backward_p, the L-BFGS against the C restatement of lbfgs_optimize
driving the CPU composition, properties of a longer run, a problem without an overlap, the cancel word, the C++ facade.

The four shapes take the four lockstep update forms by their variable count n = (N - 1) K + N:
    N = 2, K = 16: n = 18 two problems per wave;  N = 3, K = 24: n = 51 one variable per lane;
    N = 4, K = 32: n = 100 two per lane;          N = 8, K = 32: n = 232 the lane kernel
(K is what the n of each form needs with the three corridor inputs of tests/sfc_np.py; the four-piece shape is the first four
pieces of the eight-piece input).  B is 1, 65 or 257: across the 64-lane and 256-thread boundaries."""
import os
import subprocess

import numpy as np
import pytest

from oracle import cbind
from tests import polytope_np as pnp
from tests import sfc_np
from tests.util import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6
PEN = dict(rho=50.0, w_corridor=1e3, w_vel=10.0, w_acc=10.0, smooth_mu=1e-2, max_vel=3.0, max_acc=4.0, res=8)
# name -> (input seed, pieces used, order s, batch)
SHAPES = {"n18": (9, 2, 3, 65), "n51": (7, 3, 3, 65), "n100": (1, 4, 4, 65), "n232": (1, 8, 4, 257)}


def _penalty(M):
    import allocnet_amd as aa
    return aa.make_penalty(poly_rows=M, **PEN)


def _problem(name, B=None):
    """The first B problems of a shape, cut to its piece count: head, tail, wps, T, hp (trajectory-major) and s, N, M, K."""
    seed, N, s, B0 = SHAPES[name]
    B = B or B0
    _, Bf, Nf, M = next(i for i in sfc_np.INPUTS if i[0] == seed)
    head, tail, wps, T, hp = (a[:B].copy() for a in sfc_np.corridor(seed, Bf, Nf, M))
    if N < Nf:
        tail = np.zeros_like(tail); tail[:, :, 0] = wps[:, N - 1]
        wps, T, hp = wps[:, :N - 1].copy(), T[:, :N].copy(), hp[:, :N].copy()
    return dict(head=head, tail=tail, wps=wps, T=T, hp=hp, s=s, c=3, N=N, M=M, K=sfc_np.K_OF[seed], B=B)


_cache = {}


def _prepared(name, anet_ctx, B=None):
    """A shape with its overlap vertices and backward_p start from the device, computed once per session."""
    import allocnet_amd as aa
    key = (name, B)
    if key not in _cache:
        p = _problem(name, B)
        ov = aa.sfc_overlap_vertices(p["hp"], max_verts=p["K"], epsilon=EPS, ctx=anet_ctx)
        bp = aa.sfc_backward_p(p["wps"], ov["verts"], ov["count"], ctx=anet_ctx)
        p.update(verts=ov["verts"], count=ov["count"], ostatus=ov["status"], xi0=bp["xi"], residual=bp["residual"])
        _cache[key] = p
    return _cache[key]


def _run_dev(p, anet_ctx, xi0=None, T0=None, hp=None, verts=None, count=None, ostatus=None, **kw):
    """anet_lbfgs_minco_sfc_dev from trajectory-major numpy: returns numpy results, xi (B, N-1, K) and T (B, N) in place."""
    import torch
    import allocnet_amd as aa
    from allocnet_amd.sfc_opt import _bm, _tm
    B, N, K = p["B"], p["N"], p["K"]
    pick = lambda a, k: p[k] if a is None else a
    xi = _bm(pick(xi0, "xi0"), B); T = _bm(pick(T0, "T"), B)
    coeffs = torch.zeros(N * 3 * 2 * p["s"], T.stride(0), device=T.device, dtype=torch.float64)
    out = aa.lbfgs_minco_sfc_dev(_bm(p["head"], B), _bm(p["tail"], B), xi, T, _bm(pick(verts, "verts"), B),
                                 _bm(pick(count, "count"), B, torch.int32), p["s"], p["c"], N, B, K, hpolys=_bm(pick(hp, "hp"), B),
                                 penalty=_penalty(p["M"]), overlap_status=_bm(pick(ostatus, "ostatus"), B, torch.int32),
                                 coeffs=coeffs, ctx=anet_ctx, **kw)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in ("cost", "status", "iters", "evals")}
    res.update(xi=_tm(xi, B, (N - 1, K)), T=_tm(T, B, (N,)), wps=_tm(out["wps"], B, (N - 1, 3)),
               coeffs=_tm(coeffs, B, (N, 3, 2 * p["s"])))
    return res


def _qhull_vertices(pair):
    """Qhull's vertex set of a stacked pair about HiGHS' interior point, merged as pnp.vertices_qhull merges (without its six
    boundedness programmes: every corridor polytope carries its bounding box)."""
    from scipy.spatial import HalfspaceIntersection
    depth, x = pnp.interior(pair)
    assert depth > 0.0 and np.isfinite(depth)
    n, d, _ = pnp.unit_rows(pair)
    pts = HalfspaceIntersection(np.c_[n, d], x).intersections
    return pnp.merge(pts[np.all(np.isfinite(pts), axis=1)])


# ---- overlap vertices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [9, 7, 1])
def test_overlap_vertices_are_the_enumeration_of_the_stacked_pair(anet_ctx, seed):
    import allocnet_amd as aa
    _, B, N, M = next(i for i in sfc_np.INPUTS if i[0] == seed)
    hp = sfc_np.corridor(seed, B, N, M)[4]
    K = sfc_np.K_OF[seed]
    st = sfc_np.stacked_raw(hp)
    ov = aa.sfc_overlap_vertices(hp, max_verts=K, epsilon=EPS, ctx=anet_ctx)
    ref, rstat = aa.polytope_vertices(st.reshape(B * (N - 1), 2 * M, 4), EPS, ctx=anet_ctx, max_vertices=K)
    assert (ov["status"] == 0).all() and (rstat == 0).all()
    worst = 0.0
    for b in range(B):
        for w in range(N - 1):
            v = ref[b * (N - 1) + w]
            k = ov["count"][b, w]
            assert k == len(v) and np.array_equal(ov["verts"][b, w, :k], v), (b, w)      # bit for bit, in the same order
            assert (ov["verts"][b, w, k:] == 0.0).all()
            vq = _qhull_vertices(st[b, w])
            assert len(vq) == k, (b, w)
            tol = 1e-8 * max(1.0, np.abs(vq).max())
            worst = max(worst, pnp.hausdorff(v, vq) / tol)
    print("overlap vertices, seed %d: largest distance to Qhull's set %.3g of its tolerance" % (seed, worst))
    assert worst <= 1.0


def test_overlap_vertices_truncated_to_max_verts_write_nothing_past_it(anet_ctx):
    """K = 8 on the M = 16 corridors: status 2 and counts clamped to 8 where an overlap has more, the first 8 vertices kept, and
    sentinel-filled arrays untouched behind the last slot and in the columns past the batch."""
    import torch
    import allocnet_amd as aa
    from allocnet_amd.sfc_opt import _bm
    seed, B, N, M = sfc_np.INPUTS[0]
    B, K = 65, 8
    hp = sfc_np.corridor(seed, 257, N, M)[4][:B]
    full = aa.sfc_overlap_vertices(hp, max_verts=32, epsilon=EPS, ctx=anet_ctx)
    thp = _bm(hp, B)
    ld = thp.stride(0)
    rows = (N - 1) * K * 3
    verts = torch.full((rows + 7, ld), -7.5, device="cuda", dtype=torch.float64)
    count = torch.full((N - 1 + 2, ld), -9, device="cuda", dtype=torch.int32)
    status = torch.full((N - 1 + 2, ld), -9, device="cuda", dtype=torch.int32)
    aa.sfc_overlap_vertices_dev(thp, N, B, M, K, EPS, verts=verts, count=count, status=status, ctx=anet_ctx)
    torch.cuda.synchronize()
    v, cnt, stt = verts.cpu().numpy(), count.cpu().numpy(), status.cpu().numpy()
    assert (v[rows:] == -7.5).all() and (v[:, B:] == -7.5).all()
    assert (cnt[N - 1:] == -9).all() and (cnt[:, B:] == -9).all() and (stt[N - 1:] == -9).all() and (stt[:, B:] == -9).all()
    big = full["count"] > K                                                       # (B, N-1)
    assert big.any() and (~big).any()
    assert np.array_equal(cnt[:N - 1, :B].T, np.minimum(full["count"], K))
    assert np.array_equal(stt[:N - 1, :B].T, np.where(big, 2, 0))
    got = v[:rows, :B].T.reshape(B, N - 1, K, 3)
    assert np.array_equal(got, full["verts"][:, :, :K])


# ---- forward / backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("n18", 1), ("n18", 65), ("n232", 257)])
def test_forward_and_gradient_match_the_restatement(anet_ctx, name, B):
    import torch
    import allocnet_amd as aa
    from allocnet_amd.sfc_opt import _bm, _tm
    p = _prepared(name, anet_ctx, B)
    N, K = p["N"], p["K"]
    rng = np.random.default_rng(21)
    used = np.arange(K)[None, None, :] < p["count"][:, :, None]
    xi = np.where(used, rng.normal(size=(B, N - 1, K)) * rng.choice([0.1, 0.4, 2.0], size=(B, N - 1, 1)), 0.0)
    gP = rng.normal(size=(B, N - 1, 3)) * 10.0
    w_norm = 0.7

    def device(xi_, verts_, K_):
        txi, tv = _bm(xi_, B), _bm(verts_, B)
        fw = aa.sfc_forward_p_dev(txi, tv, N, B, K_, w_norm, ctx=anet_ctx)
        cost = torch.full((txi.stride(0),), 3.0, device="cuda", dtype=torch.float64)
        g = aa.sfc_backward_grad_p_dev(txi, tv, fw["wps"], fw["norm"], _bm(gP, B), N, B, K_, cost=cost, ctx=anet_ctx)
        torch.cuda.synchronize()
        return _tm(fw["wps"], B, (N - 1, 3)), _tm(fw["norm"], B, (3, N - 1)), _tm(g, B, (N - 1, K_)), cost[:B].cpu().numpy()
    P, nrm, g, cost = device(xi, p["verts"], K)
    P0, S0 = sfc_np.forward(xi, p["verts"])
    g0 = sfc_np.backward(xi, p["verts"], gP, w_norm)
    c0 = sfc_np.norm_term(xi, w_norm)[0]
    near = lambda a, b: (np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b))).all()
    assert near(P, P0) and near(nrm[:, 0], 1.0 / S0) and near(g, g0) and near(nrm[:, 1], c0) and near(cost, 3.0 + c0.sum(1))
    assert (B == 1 or ((S0 > 1.0).any() and (S0 < 1.0).any())) and (g[~used] == 0.0).all()
    # the same problem padded to K + 16: the same bits, exact zeros behind
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:2] + (16,) + a.shape[3:])], axis=2)
    P2, nrm2, g2, cost2 = device(pad(xi), pad(p["verts"]), K + 16)
    assert np.array_equal(P2, P) and np.array_equal(nrm2, nrm) and np.array_equal(g2[:, :, :K], g) and (g2[:, :, K:] == 0.0).all()
    assert np.array_equal(cost2, cost)


@pytest.mark.parametrize("name", ["n51", "n232"])
def test_composed_gradient_on_the_device(anet_ctx, name):
    """forward_p -> anet_minco_cost_grad_dev -> backward_grad_p in (xi, T) against the CPU composition (1e-7 max(1, |g|), the bar
    tests/test_grad_gpu.py holds the kernels to against the oracle) and against central differences of the device cost (h = 1e-6,
    2e-5 max(1, |g|): test_energy_only_gradient_finite_difference).  The chain through T(tau) is the update kernels' and the
    propagate kernel's, covered by the L-BFGS comparison below."""
    import torch
    import allocnet_amd as aa
    from allocnet_amd.sfc_opt import _bm, _tm
    p = _prepared(name, anet_ctx, 65)
    B, N, K, s = p["B"], p["N"], p["K"], p["s"]
    rng = np.random.default_rng(22)
    used = np.arange(K)[None, None, :] < p["count"][:, :, None]
    xi = np.where(used, rng.uniform(0.15, 0.5, size=(B, N - 1, K)), 0.0)
    thead, ttail, tT, tv, thp = (_bm(p[k], B) for k in ("head", "tail", "T", "verts", "hp"))
    pen = _penalty(p["M"])

    def device(xi_, grad=True):
        txi = _bm(xi_, B)
        fw = aa.sfc_forward_p_dev(txi, tv, N, B, K, 1.0, ctx=anet_ctx)
        cost, gP, gT, _ = aa.minco_cost_grad_dev(thead, ttail, fw["wps"], tT, s, 3, N, B, hpolys=thp, penalty=pen, ctx=anet_ctx)
        g = aa.sfc_backward_grad_p_dev(txi, tv, fw["wps"], fw["norm"], gP, N, B, K, cost=cost, ctx=anet_ctx)
        torch.cuda.synchronize()
        return cost[:B].cpu().numpy(), _tm(g, B, (N - 1, K)), _tm(gT, B, (N,))
    cost, g, gT = device(xi)
    live = 0
    for b in range(B):
        f = sfc_np.Composed(s, p["head"][b], p["tail"][b], p["hp"][b], p["verts"][b], PEN, w_norm=1.0, with_times=False)
        f.T_fixed = p["T"][b]
        c0, g0 = f(xi[b].ravel())
        gref = g0.reshape(N - 1, K)
        live += np.square(xi[b]).sum(-1).max() > 1.0
        assert abs(cost[b] - c0) <= 1e-9 * abs(c0), b
        assert np.abs(g[b] - gref).max() <= 1e-7 * max(1.0, np.abs(gref).max()), b
    assert live > 0                                                             # the norm term entered
    h = 1e-6
    for w, j in [(0, 0), (N - 2, 3), ((N - 1) // 2, 1)]:
        e = np.zeros_like(xi); e[:, w, j] = h
        fd = (device(xi + e)[0] - device(xi - e)[0]) / (2 * h)
        assert np.abs(fd - g[:, w, j]).max() <= 2e-5 * max(1.0, np.abs(g[:, w, j]).max()), (w, j)


# ---- backward_p ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n18", "n51", "n100"])
def test_backward_p_reaches_inside_points_and_reports_the_distance_of_outside_ones(anet_ctx, name):
    """forward_p(backward_p(p)) against p.  Inside waypoints: the device's largest distance may be at most ten times the largest of
    the restatement's own run (cbind.lbfgs_optimize on sfc_np.tiny_nls, same parameters, same start): the two stop at different
    iterates of the same stopping test.  Outside ones: the residual is |P - p| to 1e-12, positive, and P is in both polytopes.
    Measured (MI355X, one run): see DESIGN.md 8j."""
    import allocnet_amd as aa
    p = _prepared(name, anet_ctx)
    B, N, K = p["B"], p["N"], p["K"]
    st = sfc_np.stacked_raw(p["hp"])
    P = aa.sfc_forward_p(p["xi0"], p["verts"], ctx=anet_ctx)["wps"]
    dist = np.linalg.norm(P - p["wps"], axis=2)
    assert np.abs(np.square(p["xi0"]).sum(-1) - 1.0).max() <= 1e-14                # unit norm
    inside = np.array([[sfc_np.row_violation(st[b, w], p["wps"][b, w]) <= 0.0 for w in range(N - 1)] for b in range(B)])
    ref = max(sfc_np.backward_p(p["wps"][b, w], p["verts"][b, w], p["count"][b, w])[1]
              for b in range(B) for w in range(N - 1) if inside[b, w])
    print("backward_p %s: largest distance of an inside waypoint: device %.3g, restatement %.3g; %d outside" %
          (name, dist[inside].max(), ref, (~inside).sum()))
    assert dist[inside].max() <= 10.0 * ref
    out = ~inside
    assert out.any()
    assert np.abs(p["residual"] - dist).max() <= 1e-12
    assert (p["residual"][out] > 0.0).all()
    for b, w in zip(*np.nonzero(out)):
        assert sfc_np.row_violation(st[b, w], P[b, w]) <= EPS + 1e-9, (b, w)


# ---- the L-BFGS against the restatement ------------------------------------------------------------------------------------------
def _restatement(p, b, budget, min_duration=0.0):
    N, K = p["N"], p["K"]
    f = sfc_np.Composed(p["s"], p["head"][b], p["tail"][b], p["hp"][b], p["verts"][b], PEN, w_norm=1.0)
    x0 = np.concatenate([p["xi0"][b].ravel(), sfc_np.backward_T(p["T"][b])])
    sb = None
    if min_duration > 0.0:
        tau_min = float(sfc_np.backward_T(min_duration))
        nxi = (N - 1) * K

        def sb(xp, d):
            worst = 0.0
            for i in range(nxi, len(xp)):
                if d[i] < 0.0:
                    worst = max(worst, -d[i] / max(xp[i] - tau_min, 1e-300))
            return 1.0 / worst if worst > 0.0 else np.inf
    ret, x, fx, it, ev = cbind.lbfgs_optimize(x0, f, cbind.lbfgs_default_param(max_iterations=budget), stepbound=sb)
    return ret, x, fx, it, ev


def _compare_with_restatement(p, out, budget, label, min_duration=0.0):
    """The bar of test_generic_device_objective_matches_the_restatement: identical (status, k, evals) in at least B - B // 50
    problems, for those the cost to 1e-9 relative and the iterate to 1e-8; the others the same kind of outcome, within 6
    evaluations and 2 iterations, and a cost of the same order."""
    B = p["B"]
    same = 0
    for b in range(B):
        ret, xo, fo, ito, evo = _restatement(p, b, budget, min_duration)
        xg = np.concatenate([out["xi"][b].ravel(), sfc_np.backward_T(out["T"][b])])
        if (out["status"][b], out["iters"][b], out["evals"][b]) == (ret, ito, evo):
            same += 1
            assert abs(out["cost"][b] - fo) <= 1e-9 * max(1.0, abs(fo)), b
            assert np.abs(xg - xo).max() <= 1e-8 * max(1.0, np.abs(xo).max()), b
        else:
            assert (out["status"][b] < 0) == (ret < 0) and abs(int(out["evals"][b]) - evo) <= 6 and \
                abs(int(out["iters"][b]) - ito) <= 2, (b, out["status"][b], out["iters"][b], out["evals"][b], ret, ito, evo)
            assert out["cost"][b] <= 10.0 * fo + 1.0 and fo <= 10.0 * out["cost"][b] + 1.0, (b, out["cost"][b], fo)
    print("%s: identical (status, k, evals) in %d of %d problems" % (label, same, B))
    assert same >= B - B // 50, (same, B)


@pytest.mark.parametrize("name", ["n18", "n51", "n100", "n232"])
def test_lbfgs_matches_the_restatement_at_a_fixed_budget(anet_ctx, name):
    """max_iterations = 6: device (status, iters, evals) against cbind.lbfgs_optimize driving the CPU composition problem by
    problem -- the bar and the fallback bounds of test_generic_device_objective_matches_the_restatement."""
    import allocnet_amd as aa
    p = _prepared(name, anet_ctx)
    out = _run_dev(p, anet_ctx, param=aa.lbfgs_parameter_t(max_iterations=6), max_evals=400)
    _compare_with_restatement(p, out, 6, "corridor-constrained L-BFGS " + name)


def test_lbfgs_with_a_minimum_duration_matches_the_restatement(anet_ctx):
    """min_duration = 0.3 against the restatement running the same bound as its proc_stepbound: the same bar and fallback bounds as
    the unbounded leg, and no duration below the bound."""
    import allocnet_amd as aa
    p = _prepared("n51", anet_ctx)
    out = _run_dev(p, anet_ctx, param=aa.lbfgs_parameter_t(max_iterations=6), max_evals=400, min_duration=0.3)
    _compare_with_restatement(p, out, 6, "bounded corridor-constrained L-BFGS", min_duration=0.3)
    assert (out["T"] >= 0.3 - 1e-12).all()


# ---- a longer run ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("n18", 1), ("n51", 65), ("n232", 257)])
def test_properties_of_a_longer_run(anet_ctx, name, B):
    import allocnet_amd as aa
    p = _prepared(name, anet_ctx, B)
    N, K, s = p["N"], p["K"], p["s"]
    start = _run_dev(p, anet_ctx, max_evals=1)                                 # one evaluation: the cost of the start point
    out = _run_dev(p, anet_ctx, max_evals=300)
    st = sfc_np.stacked_raw(p["hp"])
    worst = max(sfc_np.row_violation(st[b, w], out["wps"][b, w]) for b in range(B) for w in range(N - 1))
    print("longer run %s: largest row violation at a junction %.3g, cost %.6g -> %.6g (batch mean)" %
          (name, worst, start["cost"].mean(), out["cost"].mean()))
    assert worst <= EPS + 1e-9
    assert (start["evals"] == 1).all() and (out["cost"] <= start["cost"]).all() and (out["cost"] < start["cost"]).any()
    assert (out["T"] > 0.0).all()
    assert np.array_equal(out["wps"], aa.sfc_forward_p(out["xi"], p["verts"], ctx=anet_ctx)["wps"])       # bit for bit
    co, _ = aa.minco_solve(p["head"], p["tail"], out["wps"], out["T"], s, ctx=anet_ctx)
    assert rel_err(out["coeffs"], co) <= 1e-9
    # the host-staged form is the same pipeline: overlaps, backward_p, the optimisation
    if B > 1:
        host = aa.lbfgs_minco_sfc(p["head"], p["tail"], p["hp"], p["T"], s, wps=p["wps"], penalty=_penalty(p["M"]), max_evals=300,
                                  max_verts=K, epsilon=EPS, ctx=anet_ctx)
        for k in ("cost", "status", "iters", "evals", "wps", "T", "xi", "coeffs"):
            assert np.array_equal(host[k], out[k]), k
        assert np.array_equal(host["residual"], p["residual"]) and np.array_equal(host["overlap_status"], p["ostatus"])


def test_default_max_verts_and_mean_start(anet_ctx):
    """max_verts None: the next multiple of 8 above the largest overlap count; wps None: every waypoint starts at its overlap's
    vertex mean, with residual 0 -- the run is the device run started from xi_j = 1 / sqrt(k) (one evaluation, so the cost is the
    start point's; the iterate returned is the line search's first trial point on both sides)."""
    import allocnet_amd as aa
    p = _prepared("n51", anet_ctx)
    res = aa.lbfgs_minco_sfc(p["head"], p["tail"], p["hp"], p["T"], p["s"], penalty=_penalty(p["M"]), max_evals=1, ctx=anet_ctx)
    assert res["max_verts"] == (int(p["count"].max()) // 8 + 1) * 8 == p["K"]
    assert (res["residual"] == 0.0).all() and (res["evals"] == 1).all()
    k = p["count"][:, :, None]
    xi0 = np.where(np.arange(p["K"])[None, None, :] < k, 1.0 / np.sqrt(k), 0.0)
    dev = _run_dev(p, anet_ctx, xi0=xi0, max_evals=1)
    mean = p["verts"].sum(2) / k
    for b in range(0, p["B"], 8):                                                 # the cost of the vertex means, from the CPU composition
        f = sfc_np.Composed(p["s"], p["head"][b], p["tail"][b], p["hp"][b], p["verts"][b], PEN, w_norm=1.0)
        assert np.abs(f.waypoints(np.concatenate([xi0[b].ravel(), np.zeros(p["N"])])) - mean[b]).max() <= 1e-12 * max(1.0, np.abs(mean).max())
        c0 = f(np.concatenate([xi0[b].ravel(), sfc_np.backward_T(p["T"][b])]))[0]
        assert abs(res["cost"][b] - c0) <= 1e-9 * abs(c0), b
    assert np.abs(res["cost"] - dev["cost"]).max() <= 1e-12 * np.abs(dev["cost"]).max()
    assert np.abs(res["xi"] - dev["xi"]).max() <= 1e-12 and np.abs(res["wps"] - dev["wps"]).max() <= 1e-12 * max(1.0, np.abs(mean).max())


# ---- a problem without an overlap ----------------------------------------------------------------------------------------------------
def test_a_problem_without_an_overlap_is_not_run_and_disturbs_nobody(anet_ctx):
    import allocnet_amd as aa
    p = _prepared("n51", anet_ctx)
    B, N, K = p["B"], p["N"], p["K"]
    intact = _run_dev(p, anet_ctx, max_evals=60)
    hp = p["hp"].copy()
    shift = np.array([100.0, 0.0, 0.0])
    hp[17, 2, :, 3] += hp[17, 2, :, :3] @ shift                                     # polytope 2 of problem 17, 100 m away
    assert pnp.interior(sfc_np.stacked_raw(hp)[17, 1])[0] < -40.0                   # empty (HiGHS): the deepest "ball" has a negative radius
    ov = aa.sfc_overlap_vertices(hp, max_verts=K, epsilon=EPS, ctx=anet_ctx)
    assert ov["status"][17, 1] == 1 and ov["count"][17, 1] == 0 and (np.delete(ov["status"], 17, 0) == 0).all()
    bp = aa.sfc_backward_p(p["wps"], ov["verts"], ov["count"], ctx=anet_ctx)
    assert np.isinf(bp["residual"][17, 1]) and (bp["xi"][17, 1] == 0.0).all()
    out = _run_dev(p, anet_ctx, xi0=bp["xi"], hp=hp, verts=ov["verts"], count=ov["count"], ostatus=ov["status"], max_evals=60)
    assert out["status"][17] == aa.SFC_NO_OVERLAP and out["iters"][17] == 0 and out["evals"][17] == 0 and np.isnan(out["cost"][17])
    assert np.array_equal(out["xi"][17], bp["xi"][17]) and np.array_equal(out["T"][17], p["T"][17])      # inputs untouched
    assert "overlap" in aa.lbfgs_strerror(aa.SFC_NO_OVERLAP)
    rest = np.arange(B) != 17
    for k in ("cost", "status", "iters", "evals", "xi", "T", "wps", "coeffs"):
        assert np.array_equal(out[k][rest], intact[k][rest]), k                     # problems are independent: the same bits
    # the host-staged form reports it the same way
    host = aa.lbfgs_minco_sfc(p["head"], p["tail"], hp, p["T"], p["s"], wps=p["wps"], penalty=_penalty(p["M"]), max_evals=60,
                              max_verts=K, epsilon=EPS, ctx=anet_ctx)
    assert host["status"][17] == aa.SFC_NO_OVERLAP and host["overlap_status"][17, 1] == 1 and np.array_equal(host["T"][17], p["T"][17])
    assert np.array_equal(host["cost"][rest], intact["cost"][rest])


# ---- the cancel word -----------------------------------------------------------------------------------------------------------------
def test_cancel_word_stops_every_problem_where_one_iteration_stops(anet_ctx):
    """As test_minco_lbfgs_cancel_word for the existing entry: with the word set from the start every problem is cancelled after
    its first iteration -- iterate, cost and counters those of max_iterations = 1, only the return code differs."""
    import torch
    import allocnet_amd as aa
    from allocnet_amd import lbfgs as L
    p = _prepared("n100", anet_ctx)
    free = _run_dev(p, anet_ctx, max_evals=40)
    one = _run_dev(p, anet_ctx, max_evals=40, param=aa.lbfgs_parameter_t(max_iterations=1))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    anet_ctx.set_cancel_flag(flag)
    try:
        same = _run_dev(p, anet_ctx, max_evals=40)
        for k in ("cost", "evals", "iters", "status", "T", "xi"):
            assert np.array_equal(same[k], free[k]), k
        flag.fill_(1)
        torch.cuda.synchronize()
        can = _run_dev(p, anet_ctx, max_evals=40)
    finally:
        anet_ctx.set_cancel_flag(None)
    ran = one["status"] == L.LBFGSERR_MAXIMUMITERATION
    assert ran.mean() > 0.9
    assert (can["status"][ran] == L.LBFGS_CANCELED).all()
    for k in ("iters", "evals", "cost", "T", "xi", "wps"):
        assert np.array_equal(can[k][ran], one[k][ran]), k
    rest = ~ran
    assert np.isin(can["status"][rest], (L.LBFGS_CANCELED,) + tuple(np.unique(one["status"][rest]))).all()
    assert (can["status"][rest & (one["status"] < 0)] == one["status"][rest & (one["status"] < 0)]).all()
    # cleared: the plain run again
    again = _run_dev(p, anet_ctx, max_evals=40)
    for k in ("cost", "evals", "iters", "status", "T", "xi"):
        assert np.array_equal(again[k], free[k]), k


# ---- the C++ facade ------------------------------------------------------------------------------------------------------------------
def test_cpp_program_prints_the_python_facades_numbers(anet_ctx, tmp_path):
    """tests/cpp/test_sfc_opt.cpp (sfc_opt::forwardP / backwardP / backwardGradP / optimize on problem 0 of the three-piece input,
    read from a text file this test writes) prints with %.17g what the Python facade returns, bit for bit."""
    import allocnet_amd as aa
    from allocnet_amd import _lib
    p = _prepared("n51", anet_ctx)
    N, K, M, s = p["N"], p["K"], p["M"], p["s"]
    exe = str(tmp_path / "test_sfc_opt")
    res = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "tests", "cpp", "test_sfc_opt.cpp"), "-o", exe, "-L", os.path.dirname(_lib.LIB_PATH),
                          "-lallocnet_amd", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    b = 0
    rng = np.random.default_rng(23)
    gP = rng.normal(size=(N - 1, 3))
    inp = tmp_path / "problem.txt"
    with open(inp, "w") as fh:
        fh.write("%d %d %d %d\n" % (s, N, M, K))
        for a in (p["head"][b], p["tail"][b], p["T"][b], p["hp"][b], p["wps"][b], gP):
            fh.write(" ".join("%.17g" % x for x in np.asarray(a).ravel()) + "\n")
    run = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    got = {ln.split(":")[0]: np.array(ln.split(":")[1].split(), dtype=np.float64) for ln in run.stdout.splitlines() if ":" in ln}
    one = lambda a: np.asarray(a)[b:b + 1]
    pen = _penalty(M)
    ov = aa.sfc_overlap_vertices(one(p["hp"]), max_verts=K, epsilon=EPS, ctx=anet_ctx)
    bp = aa.sfc_backward_p(one(p["wps"]), ov["verts"], ov["count"], ctx=anet_ctx)
    fw = aa.sfc_forward_p(bp["xi"], ov["verts"], ctx=anet_ctx)
    import torch
    from allocnet_amd.sfc_opt import _bm, _tm
    txi, tv = _bm(bp["xi"], 1), _bm(ov["verts"], 1)
    f2 = aa.sfc_forward_p_dev(txi, tv, N, 1, K, 1.0, ctx=anet_ctx)
    g = aa.sfc_backward_grad_p_dev(txi, tv, f2["wps"], f2["norm"], _bm(gP[None], 1), N, 1, K, ctx=anet_ctx)
    torch.cuda.synchronize()
    opt = aa.lbfgs_minco_sfc(one(p["head"]), one(p["tail"]), one(p["hp"]), one(p["T"]), s, wps=one(p["wps"]), penalty=pen,
                             max_evals=80, max_verts=K, epsilon=EPS, ctx=anet_ctx)
    want = {"xi": bp["xi"], "residual": bp["residual"], "P": fw["wps"], "grad_xi": _tm(g, 1, (N - 1, K)), "cost": opt["cost"],
            "durations": opt["T"], "wps": opt["wps"], "coeffs": opt["coeffs"],
            "status": [opt["status"][0], opt["iters"][0], opt["evals"][0]]}
    for k, v in want.items():
        assert k in got, (k, list(got))
        assert np.array_equal(got[k], np.asarray(v, dtype=np.float64).ravel()), k
