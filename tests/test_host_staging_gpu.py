"""The trajectory-major host entry points at the shapes their own suites do not reach: one trajectory (row stride 1, inputs packed
into one copy) and three (row stride 64), one piece (no waypoints: zero-width fields) and two, order 3, optional inputs absent.

Each host call is compared with the same entry point's _dev form on torch tensors at the stager's row stride (csrc/staging.h), with
the tolerance of that entry point's oracle test (named at each case); anet_lbfgs_mvie has no _dev form and is compared with the C
restatement at a fixed iteration budget, as tests/test_lbfgs_gpu.py does.  The other suites call these entry points at neither of
these batches with these piece counts (test_ragged_batches solves one trajectory of eight pieces, test_sfc_opt_gpu runs 1, 65 and
257 corridors with start waypoints), so no (entry point, batch) pair is left out here."""
import ctypes

import numpy as np
import pytest

from tests.util import random_problem

pytestmark = pytest.mark.gpu

S, C = 3, 3
BATCHES = [1, 3]
PIECES = [1, 2]


def _abs(got, ref, tol, what):
    """|got - ref| <= tol max(1, |ref|), element by element"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.size:
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        assert err.max() <= tol, (what, err.max())


def _rel(got, ref, tol, what):
    """|got - ref| <= tol |ref|, element by element"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and (np.abs(got - ref) <= tol * np.abs(ref)).all(), (what, np.abs(got - ref).max())


def _tools(anet_ctx):
    import torch
    from allocnet_amd.sfc_opt import _bm, _tm
    dev = torch.device("cuda", anet_ctx.device)
    bm = lambda a, B, dtype=None: _bm(a, B, dtype, ctx=anet_ctx)
    new = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float64)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    return bm, _tm, new, q, stream


def _problem(B, N, seed):
    return random_problem(np.random.default_rng(seed + 10 * B + N), B, N, C)


def _coeffs(anet_ctx, B, N, seed):
    import allocnet_amd as aa
    head, tail, wps, T = _problem(B, N, seed)
    return aa.minco_solve(head, tail, wps, T, S, ctx=anet_ctx)[0], T


@pytest.mark.parametrize("N", PIECES)
@pytest.mark.parametrize("B", BATCHES)
def test_minco_solve(anet_ctx, B, N):
    """test_minco_gpu.test_solve_matches_oracle: 1e-9 relative on coefficients (largest entry) and energy"""
    import allocnet_amd as aa
    bm, tm, new, _, _ = _tools(anet_ctx)
    head, tail, wps, T = _problem(B, N, 1)
    co, en = aa.minco_solve(head, tail, wps, T, S, ctx=anet_ctx)
    d_T = bm(T, B)
    d_co, d_en = new(N * 3 * 2 * S, d_T.shape[1]), new(d_T.shape[1])
    aa.minco_solve_dev(bm(head, B), bm(tail, B), bm(wps, B), d_T, S, C, N, B, coeffs=d_co, energy=d_en, ctx=anet_ctx)
    ref = tm(d_co, B, (N, 3, 2 * S))
    assert np.abs(co - ref).max() <= 1e-9 * np.abs(ref).max()
    _rel(en, d_en[:B].cpu().numpy(), 1e-9, "energy")
    assert aa.minco_solve(head, tail, wps, T, S, want_coeffs=False, ctx=anet_ctx)[0] is None


@pytest.mark.parametrize("N", PIECES)
@pytest.mark.parametrize("B", BATCHES)
def test_minco_sample_costs(anet_ctx, B, N):
    """test_minco_gpu.test_time_allocation_sampling_matches_the_replicated_solve: 1e-13 of the largest cost"""
    import allocnet_amd as aa
    bm, _, _, _, _ = _tools(anet_ctx)
    head, tail, wps, T = _problem(B, N, 2)
    cost = aa.minco_sample_costs(head[0], tail[0], wps[0], T, S, rho=3.0, ctx=anet_ctx)
    ref = aa.minco_sample_costs_dev(bm(head[:1], 1), bm(tail[:1], 1), bm(wps[:1], 1), bm(T, B), S, C, N, 1, B, rho=3.0, ctx=anet_ctx)
    ref = ref.cpu().numpy()
    assert cost.shape == (B,) and np.abs(cost - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("N", PIECES)
@pytest.mark.parametrize("B", BATCHES)
def test_trajectory_entry_points(anet_ctx, B, N):
    """test_trajectory_gpu: evaluation 1e-11, cost 1e-11 relative, duration gradient 1e-10; test_max_rate_gpu: 1e-8"""
    import allocnet_amd as aa
    bm, tm, new, q, stream = _tools(anet_ctx)
    lib, h = anet_ctx.lib, anet_ctx.handle
    co, T = _coeffs(anet_ctx, B, N, 3)
    nq = 3
    tq = np.random.default_rng(30 + B).uniform(0.0, 1.0, (B, nq)) * T.sum(1, keepdims=True)
    d_co, d_T, d_tq = bm(co, B), bm(T, B), bm(tq, B)
    ld = d_T.shape[1]
    for deriv in (0, 2):
        out = new(nq * 3, ld)
        anet_ctx.check(lib.anet_traj_eval_dev(h, S, N, B, ld, q(d_co), q(d_T), nq, q(d_tq), deriv, q(out), stream()))
        _abs(aa.traj_eval(co, T, tq, deriv, ctx=anet_ctx), tm(out, B, (nq, 3)), 1e-11, f"traj_eval deriv {deriv}")
    cost = new(ld)
    anet_ctx.check(lib.anet_traj_cost_dev(h, S, N, B, ld, q(d_co), q(d_T), 1400.0, q(cost), stream()))
    _rel(aa.traj_cost(co, T, S, ctx=anet_ctx), cost[:B].cpu().numpy(), 1e-11, "traj_cost")
    g = new(N, ld)
    anet_ctx.check(lib.anet_traj_cost_grad_T_dev(h, S, N, B, ld, q(d_co), q(d_T), 1400.0, q(g), stream()))
    _abs(aa.traj_cost_grad_T(co, T, ctx=anet_ctx), tm(g, B, (N,)), 1e-10, "traj_cost_grad_T")
    for which in (1, 2):
        r = new(N, ld)
        anet_ctx.check(lib.anet_traj_max_rate_dev(h, S, N, B, ld, q(d_co), q(d_T), which, q(r), stream()))
        _abs(aa.traj_max_rate(co, T, which, ctx=anet_ctx), tm(r, B, (N,)), 1e-8, f"traj_max_rate {which}")


@pytest.mark.parametrize("N", PIECES)
@pytest.mark.parametrize("B", BATCHES)
def test_minco_cost_grad(anet_ctx, B, N):
    """test_grad_gpu.test_cost_grad_matches_oracle: cost 1e-9 relative, gradients 1e-7, coefficients 1e-9 of the largest"""
    import allocnet_amd as aa
    bm, tm, new, _, _ = _tools(anet_ctx)
    head, tail, wps, T = _problem(B, N, 4)
    cost, gP, gT, co = aa.minco_cost_grad(head, tail, wps, T, S, want_coeffs=True, ctx=anet_ctx)
    d_T = bm(T, B)
    d_co = new(N * 3 * 2 * S, d_T.shape[1])
    rc, rP, rT, _ = aa.minco_cost_grad_dev(bm(head, B), bm(tail, B), bm(wps, B), d_T, S, C, N, B, coeffs=d_co, ctx=anet_ctx)
    _rel(cost, rc[:B].cpu().numpy(), 1e-9, "cost")
    _abs(gP, tm(rP[:3 * (N - 1)], B, (N - 1, 3)), 1e-7, "gradP")
    _abs(gT, tm(rT, B, (N,)), 1e-7, "gradT")
    ref = tm(d_co, B, (N, 3, 2 * S))
    assert np.abs(co - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize("B", BATCHES)
def test_lbfgs_mvie(anet_ctx, B):
    """test_lbfgs_gpu.test_mvie_matches_oracle at three iterations: counters exact, iterate and cost 1e-11"""
    import allocnet_amd as aa
    from oracle import cbind
    from tests.test_lbfgs_gpu import _mvie_batch
    A, x0, k = _mvie_batch(np.random.default_rng(50 + B), B, 7)
    kw = dict(mem_size=18, g_epsilon=0.0, min_step=1e-32, past=3, delta=1e-7, max_iterations=3)
    x, f, status, iters, evals = aa.lbfgs_mvie(A, x0, param=aa.lbfgs_parameter_t(**kw), ctx=anet_ctx)
    prm = cbind.lbfgs_default_param(**kw)
    for b in range(B):
        ret, xo, fo, it, ev = cbind.lbfgs_mvie(A[b, :k[b]], 1e-2, 1e3, x0[b], prm)
        assert (status[b], iters[b], evals[b]) == (ret, it, ev), b
        assert np.abs(x[b] - xo).max() <= 1e-11 * max(1.0, np.abs(xo).max()), b
        assert abs(f[b] - fo) <= 1e-11 * max(1.0, abs(fo))


@pytest.mark.parametrize("N", PIECES)
@pytest.mark.parametrize("B", BATCHES)
def test_lbfgs_minco(anet_ctx, B, N):
    """test_lbfgs_gpu.test_minco_lbfgs_matches_oracle: cost and coefficients 1e-8 (waypoints and durations held to the same)"""
    import allocnet_amd as aa
    bm, tm, new, _, _ = _tools(anet_ctx)
    head, tail, wps, T = _problem(B, N, 5)
    pen = aa.make_penalty(rho=40.0, w_vel=10.0, w_acc=10.0, res=8)
    prm = aa.lbfgs_parameter_t(max_iterations=6)
    out = aa.lbfgs_minco(head, tail, wps, T, S, penalty=pen, param=prm, ctx=anet_ctx)
    d_w, d_T = bm(wps, B), bm(T, B)
    d_co = new(N * 3 * 2 * S, d_T.shape[1])
    ref = aa.lbfgs_minco_dev(bm(head, B), bm(tail, B), d_w, d_T, S, C, N, B, penalty=pen, param=prm, coeffs=d_co, ctx=anet_ctx)
    for key in ("status", "iters", "evals"):
        assert np.array_equal(out[key], ref[key].cpu().numpy()), key
    _rel(out["cost"], ref["cost"].cpu().numpy(), 1e-8, "cost")
    _abs(out["wps"], tm(d_w, B, (N - 1, 3)), 1e-8, "wps")
    _abs(out["T"], tm(d_T, B, (N,)), 1e-8, "T")
    rco = tm(d_co, B, (N, 3, 2 * S))
    assert np.abs(out["coeffs"] - rco).max() <= 1e-8 * np.abs(rco).max()


@pytest.mark.parametrize("B", BATCHES)
def test_flat_forward_and_backward(anet_ctx, B):
    """test_flatness_gpu: forward 1e-12, backward 1e-10"""
    import allocnet_amd as aa
    bm, tm, _, _, _ = _tools(anet_ctx)
    rng = np.random.default_rng(60 + B)
    prm = aa.FlatnessMap(ctx=anet_ctx).params
    v, a, j = rng.uniform(-4.0, 4.0, (B, 3)), rng.uniform(-6.0, 6.0, (B, 3)), rng.normal(size=(B, 3)) * 5.0
    got = aa.flat_forward(prm, v, a, j, ctx=anet_ctx)
    ref = aa.flat_forward_dev(prm, bm(v, B), bm(a, B), bm(j, B), n=B, ctx=anet_ctx)
    _abs(got[0], ref[0][:B].cpu().numpy(), 1e-12, "thr")
    _abs(got[1], tm(ref[1], B, (4,)), 1e-12, "quat")
    _abs(got[2], tm(ref[2], B, (3,)), 1e-12, "omg")
    gt, gq, go = rng.normal(size=B), rng.normal(size=(B, 4)), rng.normal(size=(B, 3))
    got = aa.flat_backward(prm, v, a, j, None, None, None, None, gt, gq, go, ctx=anet_ctx)
    ref = aa.flat_backward_dev(prm, bm(v, B), bm(a, B), bm(j, B), None, None, None, None, bm(gt, B), bm(gq, B), bm(go, B), n=B,
                               ctx=anet_ctx)
    for name, g, r in zip(("vel", "acc", "jer"), got[1:4], ref[1:4]):
        _abs(g, tm(r, B, (3,)), 1e-10, name + "_total")
    _abs(got[4], ref[4][:B].cpu().numpy(), 1e-10, "psi_total")
    _abs(got[5], ref[5][:B].cpu().numpy(), 1e-10, "dpsi_total")


@pytest.mark.parametrize("N", PIECES)
@pytest.mark.parametrize("B", BATCHES)
def test_traj_flat_states_and_extrema(anet_ctx, B, N):
    """test_flatness_gpu.test_traj_flat_states / test_traj_flat_extrema_and_limits: 1e-12"""
    import allocnet_amd as aa
    from allocnet_amd.flatness import FLAT_STATE_FIELDS, _ref
    bm, tm, new, q, stream = _tools(anet_ctx)
    lib, h = anet_ctx.lib, anet_ctx.handle
    fm = aa.FlatnessMap(ctx=anet_ctx)
    co, T = _coeffs(anet_ctx, B, N, 7)
    nq = 2
    tq = np.random.default_rng(70 + B).uniform(0.0, 1.0, (B, nq)) * T.sum(1, keepdims=True)
    d_co, d_T, d_tq = bm(co, B), bm(T, B), bm(tq, B)
    ld = d_T.shape[1]
    out = new(nq * FLAT_STATE_FIELDS, ld)
    anet_ctx.check(lib.anet_traj_flat_states_dev(h, _ref(fm.params), S, N, B, ld, q(d_co), q(d_T), nq, q(d_tq), q(out), stream()))
    _abs(aa.traj_flat_states(fm, co, T, tq, ctx=anet_ctx), tm(out, B, (nq, FLAT_STATE_FIELDS)), 1e-12, "flat states")
    ext = new(4, ld)
    anet_ctx.check(lib.anet_traj_flat_extrema_dev(h, _ref(fm.params), S, N, B, ld, q(d_co), q(d_T), 5, q(ext), stream()))
    _abs(aa.traj_flat_extrema(fm, co, T, 5, ctx=anet_ctx), tm(ext, B, (4,)), 1e-12, "flat extrema")


@pytest.mark.parametrize("B", BATCHES)
def test_lbfgs_minco_sfc(anet_ctx, B):
    """Two pieces, no start waypoints: test_sfc_opt_gpu.test_default_max_verts_and_mean_start -- one evaluation from the vertex
    means against the device run from xi_j = 1 / sqrt(k): cost, xi and waypoints 1e-12"""
    import allocnet_amd as aa
    from tests.test_sfc_opt_gpu import _penalty, _prepared, _run_dev
    p = _prepared("n18", anet_ctx, B)
    res = aa.lbfgs_minco_sfc(p["head"], p["tail"], p["hp"], p["T"], p["s"], penalty=_penalty(p["M"]), max_verts=p["K"], max_evals=1,
                             ctx=anet_ctx)
    k = p["count"][:, :, None]
    xi0 = np.where(np.arange(p["K"])[None, None, :] < k, 1.0 / np.sqrt(k), 0.0)
    dev = _run_dev(p, anet_ctx, xi0=xi0, max_evals=1)
    assert (res["residual"] == 0.0).all() and np.array_equal(res["overlap_status"], p["ostatus"])
    for key in ("status", "iters", "evals"):
        assert np.array_equal(res[key], dev[key]), key
    _rel(res["cost"], dev["cost"], 1e-12, "cost")
    _abs(res["T"], dev["T"], 1e-12, "T")
    assert np.abs(res["xi"] - dev["xi"]).max() <= 1e-12
    _abs(res["wps"], dev["wps"], 1e-12, "wps")
    rco = dev["coeffs"]
    assert np.abs(res["coeffs"] - rco).max() <= 1e-9 * np.abs(rco).max()    # (test_properties_of_a_longer_run: 1e-9)
