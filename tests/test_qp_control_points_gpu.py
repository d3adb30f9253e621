"""GPU suite of the control-point row form of the inequality QP (ANET_QP_ROWS_CONTROL_POINTS): the dense assembly
and the interior-point solve against the numpy restatement (tests/qp_control_points_np.py) and the dense interior-point oracle
(oracle/qp_np.py), the guarantee itself against the exact margin kernels, nesting in the number of segments, the time gradient and
the backward pass against central differences, and the contracts of the flag."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import qp_np
from tests import qp_control_points_np as cp
from tests.util import qp_corridor_problem as _corridor_problem          # the generator of tests/test_qp_solve_gpu.py

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMAX, AMAX = 3.0, 4.0                      # the limits of test_interior_point_method_matches_the_oracle_optimum
SOLVE_CASES = [(4, 3, 8, 1), (3, 5, 12, 1), (4, 8, 16, 2), (3, 16, 12, 1)]     # (s, N, M, k)
_cache = {}


def _batch(s, N, M, B=6, seed=None, margin=1.0):
    """B problems of the generator.  Seed 10 s + N, the convention of tests/test_qp_solve_gpu.py: checked on the CPU with the dense
    oracle alone -- it solves 6 of 6 of every set of SOLVE_CASES in the control-point form, and its own sample-form solutions at
    res = 2 s leave the corridor or a box between samples by 1e-1 .. 5e-1 (seeds 43, 35, 48, 46)."""
    rng = np.random.default_rng(10 * s + N if seed is None else seed)
    probs = [_corridor_problem(rng, N, M, margin=margin) for _ in range(B)]
    return tuple(np.array([p[q] for p in probs]) for q in range(4))          # ini, fin, hp, T


def _oracle(s, N, M, K):
    """Per problem of _batch(s, N, M): the dense QP of the restatement and the oracle's optimum on it (computed once)."""
    key = ("oracle", s, N, M, K)
    if key not in _cache:
        ini, fin, hp, T = _batch(s, N, M)
        out = []
        for bb in range(len(T)):
            Q, A, b, G, h, piece, kind = cp.dense_qp(s, ini[bb], fin[bb], hp[bb], T[bb], K, VMAX, AMAX)
            z, lam, nu, fo, it = qp_np.qp_ipm(Q, A, b, G, h)
            ok = not (it >= 199 or qp_np.kkt_violation(Q, A, b, G, h, z) > 1e-7)
            out.append(dict(Q=Q, A=A, b=b, G=G, h=h, piece=piece, kind=kind, z=z, fo=fo, ok=ok))
        _cache[key] = out
    return _cache[key]


def _device(ctx, s, N, M, K):
    key = ("device", s, N, M, K)
    if key not in _cache:
        import allocnet_amd as aa
        ini, fin, hp, T = _batch(s, N, M)
        _cache[key] = aa.qp_solve(s, ini, fin, hp, T, res=aa.qp.control_point_res(s, K), max_vel=VMAX, max_acc=AMAX,
                                  settings=aa.qp_settings(rows="control_points"), ctx=ctx)
    return _cache[key]


# ---- (2) assembly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,N,K", [(3, 1, 1), (4, 2, 1), (4, 3, 2), (3, 5, 3)])
def test_assembly_matches_the_restatement(anet_ctx, s, N, K):
    import allocnet_amd as aa
    rng = np.random.default_rng(100 * s + 10 * N + K)
    res = aa.qp.control_point_res(s, K)
    T = rng.uniform(0.4, 2.5, size=N)
    ini = rng.normal(size=(3, 3)); fin = rng.normal(size=(3, 3))
    m_rows = [5, 3] if (s, N, K) == (4, 2, 1) else list(rng.integers(1, 6, size=N))      # unequal row counts
    polys = [rng.normal(size=(m, 4)) for m in m_rows]
    polys[0][-1] = 0.0                                                                 # a padding row inside a polytope
    for order in (aa.qp.ORDER_CPP, aa.qp.ORDER_PYTHON):
        Q, A, b, G, h = aa.qp_assemble(s, ini, fin, polys, T, res=res, max_vel=VMAX, max_acc=AMAX, row_order=order,
                                       rows="control_points", ctx=anet_ctx)
        Gr, hr = cp.dense_G_h(s, polys, T, K, VMAX, AMAX, order)
        assert G.shape == Gr.shape and h.shape == hr.shape
        eg = np.abs(G - Gr) / np.maximum(1.0, np.abs(Gr))
        print(f"s={s} N={N} k={K} order={order}: max |G - restatement| / max(1, |entry|) = {eg.max():.2e}")
        assert eg.max() <= 1e-12 and np.abs(h - hr).max() <= 1e-12 * max(1.0, np.abs(hr).max())
        assert np.array_equal(G != 0.0, Gr != 0.0)                                    # structural zeros are zeros
        Qs, As, bs, Gs, hs = aa.qp_assemble(s, ini, fin, polys, T, res=res, max_vel=VMAX, max_acc=AMAX, row_order=order, ctx=anet_ctx)
        assert Q.tobytes() == Qs.tobytes() and A.tobytes() == As.tobytes() and b.tobytes() == bs.tobytes()
        assert Gs.shape == G.shape and np.array_equal(hs, h) and not np.array_equal(Gs, G)
    # a batch in the tensor form: trailing zero rows as padding, every trajectory its own durations
    B, M = 2, 4
    hp = rng.normal(size=(B, N, M, 4)); hp[:, :, M - 1] = 0.0
    Tb = rng.uniform(0.4, 2.5, size=(B, N))
    st = rng.normal(size=(2, B, 3, 3))
    Q, A, b, G, h = aa.qp_assemble(s, st[0], st[1], hp, Tb, res=res, max_vel=VMAX, max_acc=AMAX, rows="control_points", ctx=anet_ctx)
    for bb in range(B):
        Gr, hr = cp.dense_G_h(s, [hp[bb, i] for i in range(N)], Tb[bb], K, VMAX, AMAX, 0)
        assert (np.abs(G[bb] - Gr) <= 1e-12 * np.maximum(1.0, np.abs(Gr))).all() and np.array_equal(h[bb], hr)


# ---- (3) solve ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,N,M,K", SOLVE_CASES)
def test_solve_matches_the_oracle_on_the_restatements_matrices(anet_ctx, s, N, M, K):
    """The bars of test_interior_point_method_matches_the_oracle_optimum (tests/test_qp_solve_gpu.py)."""
    out = _device(anet_ctx, s, N, M, K)
    ref = _oracle(s, N, M, K)
    assert sum(r["ok"] for r in ref) >= len(ref) // 2          # the seeds were chosen so that the oracle solves half at least
    for bb, r in enumerate(ref):
        if not r["ok"]:
            continue
        Q, A, b, G, h, z, fo = (r[k] for k in ("Q", "A", "b", "G", "h", "z", "fo"))
        zg = out["coeffs"][bb].reshape(-1)
        viol = (G @ zg - h).max() / max(1.0, np.abs(h).max())
        print(f"s={s} N={N} M={M} k={K} b={bb}: status {out['status'][bb]} iters {out['iters'][bb]} obj rel "
              f"{abs(out['obj'][bb] - fo) / max(1.0, fo):.2e} max(Gz-h)/max(1,|h|) {viol:.2e} coeff rel {np.abs(zg - z).max() / np.abs(z).max():.2e}")
        assert out["status"][bb] == 1 and out["iters"][bb] <= 40, (bb, out["status"][bb], out["iters"][bb])
        assert abs(out["obj"][bb] - 0.5 * zg @ Q @ zg) <= 1e-9 * max(1.0, fo)
        assert abs(out["obj"][bb] - fo) <= 1e-5 * max(1.0, fo), (bb, out["obj"][bb], fo)
        assert np.abs(A @ zg - b).max() <= 1e-8 * max(1.0, np.abs(b).max())
        assert viol <= 1e-6
        assert np.abs(zg - z).max() <= 1e-3 * np.abs(z).max()


# ---- (4) the guarantee -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,N,M,K", SOLVE_CASES)
def test_solved_problems_hold_their_rows_for_every_t(anet_ctx, s, N, M, K):
    """The hull property: the exact margin of a piece (anet_traj_row_margin: the maximum over its rows and over ALL t) is at most
    the largest residual of that piece's rows on the control values.  The sample form at the same row count (res = 2 s) has no such
    bound: at least one of its solved problems leaves its corridor or a box between samples."""
    import allocnet_amd as aa
    ini, fin, hp, T = _batch(s, N, M)
    out = _device(anet_ctx, s, N, M, K)
    ref = _oracle(s, N, M, K)
    solved = np.flatnonzero(out["status"] == 1)
    assert len(solved) >= len(T) // 2
    margins = aa.traj_qp_margins(out["coeffs"], T, hp, VMAX, AMAX, ctx=anet_ctx)
    for bb in solved:
        r = ref[bb]
        resid = r["G"] @ out["coeffs"][bb].reshape(-1) - r["h"]
        slack = 1e-9 * max(1.0, np.abs(r["h"]).max())
        for kind in range(3):
            for i in range(N):
                rows = (r["piece"] == i) & (r["kind"] == kind)
                assert margins[kind][bb, i] <= resid[rows].max() + slack, (bb, kind, i, margins[kind][bb, i], resid[rows].max())
    worst = max(float(m[solved].max()) for m in margins)
    smp = aa.qp_solve(s, ini, fin, hp, T, res=2 * s, max_vel=VMAX, max_acc=AMAX, ctx=anet_ctx)
    ssolved = smp["status"] == 1
    sm = aa.traj_qp_margins(smp["coeffs"], T, hp, VMAX, AMAX, ctx=anet_ctx)
    sworst = np.max([m[ssolved] for m in sm], axis=(0, 2)) if ssolved.any() else np.array([])
    print(f"s={s} N={N} M={M} k={K}: worst exact margin, control points {worst:.2e}; sample form at res {2 * s}: {np.round(sworst, 4)}")
    assert (sworst > 1e-6).any()


# ---- (5) nesting -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,N,M", [(4, 3, 8), (3, 5, 12)])
def test_feasible_sets_are_nested_in_the_number_of_segments(anet_ctx, s, N, M):
    """Halving every segment puts the new control values inside the old hull: the rows of 2 k follow from those of k."""
    import allocnet_amd as aa
    ini, fin, hp, T = _batch(s, N, M)
    tight = aa.qp_settings(rows="control_points", eps_abs=1e-10, eps_rel=1e-10)
    o = {K: aa.qp_solve(s, ini, fin, hp, T, res=aa.qp.control_point_res(s, K), max_vel=VMAX, max_acc=AMAX, settings=tight,
                        ctx=anet_ctx) for K in (1, 2, 4)}
    all3 = (o[1]["status"] == 1) & (o[2]["status"] == 1) & (o[4]["status"] == 1)
    assert all3.sum() >= 3
    print("obj k=1, 2, 4:", o[1]["obj"][all3], o[2]["obj"][all3], o[4]["obj"][all3])
    assert (o[2]["obj"][all3] <= o[1]["obj"][all3] * (1 + 1e-6)).all()
    assert (o[4]["obj"][all3] <= o[2]["obj"][all3] * (1 + 1e-6)).all()
    for bb in np.flatnonzero(o[1]["status"] == 1):
        G2, h2 = cp.dense_qp(s, ini[bb], fin[bb], hp[bb], T[bb], 2, VMAX, AMAX)[3:5]
        assert (G2 @ o[1]["coeffs"][bb].reshape(-1) - h2).max() <= 1e-6 * max(1.0, np.abs(h2).max())


# ---- (6) time gradient and backward pass ------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,N,M", [(4, 3, 9), (3, 4, 8)])
def test_time_gradient_against_central_differences(anet_ctx, s, N, M):
    """Step 1e-5 and bar 2e-4 of the largest component: tests/test_qp_solve_gpu.py:167-174 and :186-188 (the problems of :156-161,
    margin 0.6; the differences of the interior point's own optimal cost at 1e-10 -- ADMM has no control-point form)."""
    import allocnet_amd as aa
    ini, fin, hp, T = _batch(s, N, M, margin=0.6)
    kw = dict(res=aa.qp.control_point_res(s), max_vel=VMAX, max_acc=AMAX, ctx=anet_ctx)
    tight = aa.qp_settings(rows="control_points", eps_abs=1e-10, eps_rel=1e-10)
    out = aa.qp_solve(s, ini, fin, hp, T, settings=aa.qp_settings(rows="control_points"), time_grad=True, **kw)
    g = out["grad_T"]
    fd = np.zeros_like(g)
    ok = out["status"] == 1
    h = 1e-5
    for i in range(N):
        Tp = T.copy(); Tp[:, i] += h
        Tm = T.copy(); Tm[:, i] -= h
        p, m = aa.qp_solve(s, ini, fin, hp, Tp, settings=tight, **kw), aa.qp_solve(s, ini, fin, hp, Tm, settings=tight, **kw)
        ok &= (p["status"] == 1) & (m["status"] == 1)
        fd[:, i] = (p["obj"] - m["obj"]) / (2 * h)
    assert ok.sum() >= 3
    scale = np.abs(fd).max(axis=1, keepdims=True)
    print("grad_T error / scale:", (np.abs(g - fd) / scale)[ok].max(axis=1))
    assert (np.abs(g - fd)[ok] <= 2e-4 * scale[ok]).all(), (np.abs(g - fd) / scale)[ok].max(axis=1)


@pytest.mark.parametrize("s,N,M", [(4, 3, 9), (3, 4, 8)])
def test_backward_pass_against_central_differences(anet_ctx, s, N, M):
    """A random linear loss of the optimal coefficients; step 1e-5 and bar 1e-4 of the largest component:
    tests/test_qp_solve_gpu.py:396-405 (the problems of :377-383: seed 70 + 10 s + N, margin 1.2, re-solves at 1e-10)."""
    import allocnet_amd as aa
    B = 8
    ini, fin, hp, T = _batch(s, N, M, B=B, seed=70 + 10 * s + N, margin=1.2)
    kw = dict(res=aa.qp.control_point_res(s), max_vel=VMAX, max_acc=AMAX, ctx=anet_ctx)
    tight = aa.qp_settings(rows="control_points", eps_abs=1e-10, eps_rel=1e-10)
    w1 = np.random.default_rng(s).normal(size=(N, 3, 2 * s))
    loss = lambda z: (w1 * z).sum(axis=(1, 2, 3))
    base = aa.qp_solve(s, ini, fin, hp, T, settings=tight, **kw)
    out = aa.qp_solve_vjp(s, ini, fin, hp, T, np.repeat(w1[None], B, axis=0), rows="control_points", **kw)
    ok = (base["status"] == 1) & (out["status"] == 1)
    assert np.abs(out["coeffs"] - base["coeffs"])[ok].max() <= 1e-6 * np.abs(base["coeffs"])[ok].max()
    h = 1e-5
    fd = np.zeros((B, N))
    for i in range(N):
        Tp = T.copy(); Tp[:, i] += h
        Tm = T.copy(); Tm[:, i] -= h
        p, m = aa.qp_solve(s, ini, fin, hp, Tp, settings=tight, **kw), aa.qp_solve(s, ini, fin, hp, Tm, settings=tight, **kw)
        ok &= (p["status"] == 1) & (m["status"] == 1)
        fd[:, i] = (loss(p["coeffs"]) - loss(m["coeffs"])) / (2 * h)
    assert ok.sum() >= 4
    scale = np.abs(fd).max(axis=1, keepdims=True)
    err = np.abs(out["grad_T"] - fd) / scale
    print("vjp error / scale:", err[ok].max(axis=1))
    assert (err[ok] <= 1e-4).all(), err[ok].max(axis=1)


# ---- (7) contracts -----------------------------------------------------------------------------------------------------------
def test_flag_contracts(anet_ctx):
    import allocnet_amd as aa
    from allocnet_amd import _lib
    s, N, M = 4, 3, 8
    ini, fin, hp, T = _batch(s, N, M)
    kw = dict(max_vel=VMAX, max_acc=AMAX, ctx=anet_ctx)
    cps = aa.qp_settings(rows="control_points")

    def code(fn):
        with pytest.raises(aa.AnetError) as ei:
            fn()
        return ei.value.code
    for res in (20, 7, 12):                                     # not a multiple of 2 s = 8
        assert code(lambda: aa.qp_solve(s, ini, fin, hp, T, res=res, settings=cps, **kw)) == _lib.ANET_ERR_INVALID
        assert code(lambda: aa.qp_assemble(s, ini, fin, hp, T, res=res, rows="control_points", **kw)) == _lib.ANET_ERR_INVALID
    assert code(lambda: aa.qp_solve(3, ini, fin, hp, T, res=8, settings=cps, **kw)) == _lib.ANET_ERR_INVALID     # 2 s = 6
    admm = aa.qp_settings(method=aa.qp.QP_METHOD_ADMM, rows="control_points")
    assert code(lambda: aa.qp_solve(s, ini, fin, hp, T, res=8, settings=admm, **kw)) == _lib.ANET_ERR_UNSUPPORTED
    assert code(lambda: aa.qp_assemble(s, ini, fin, hp, T, res=8, float_time=True, rows="control_points", **kw)) == _lib.ANET_ERR_UNSUPPORTED
    for method in (7, 7 | 0x100, 1 | 0x200, 2 | 0x100, -1):
        assert code(lambda: aa.qp_solve(s, ini, fin, hp, T, res=8, settings=aa.qp_settings(method=method), **kw)) == _lib.ANET_ERR_INVALID
    assert code(lambda: aa.qp_assemble(s, ini, fin, hp, T, res=8, row_order=2 | 0x100, **kw)) == _lib.ANET_ERR_INVALID
    # the time gradient and the backward pass refuse the same combinations
    assert code(lambda: aa.qp_solve(s, ini, fin, hp, T, res=20, settings=cps, time_grad=True, **kw)) == _lib.ANET_ERR_INVALID
    assert code(lambda: aa.qp_solve_vjp(s, ini, fin, hp, T, np.zeros((len(T), N, 3, 2 * s)), res=20, settings=cps, **kw)) == _lib.ANET_ERR_INVALID


def _same(a, b, keys=("coeffs", "obj", "status", "iters", "residuals")):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def test_results_are_reproducible_bit_for_bit(anet_ctx):
    import torch
    import allocnet_amd as aa
    s, N, M, K = 4, 3, 8, 1
    ini, fin, hp, T = _batch(s, N, M)
    B = len(T)
    res = aa.qp.control_point_res(s, K)
    kw = dict(res=res, max_vel=VMAX, max_acc=AMAX)
    cps = aa.qp_settings(rows="control_points")
    first = _device(anet_ctx, s, N, M, K)
    assert _same(first, aa.qp_solve(s, ini, fin, hp, T, settings=cps, ctx=anet_ctx, **kw))          # a second call
    assert _same(first, aa.qp_solve(s, ini, fin, hp, T, rows="control_points", ctx=anet_ctx, **kw))  # the keyword is the same flag
    for bb in (0, B - 1):                                                                           # alone and inside a batch
        one = aa.qp_solve(s, ini[bb:bb + 1], fin[bb:bb + 1], hp[bb:bb + 1], T[bb:bb + 1], settings=cps, ctx=anet_ctx, **kw)
        assert all(np.asarray(one[k][0]).tobytes() == np.asarray(first[k][bb]).tobytes() for k in ("coeffs", "obj", "status", "iters"))
    dev = torch.device("cuda", 0)
    state = torch.from_numpy(np.ascontiguousarray(np.stack([ini, fin], axis=1))).to(dev)
    thp = torch.from_numpy(np.ascontiguousarray(hp)).to(dev); tT = torch.from_numpy(T.copy()).to(dev)
    plain = aa.qp_solve_dev(s, state, tT, thp, settings=cps, ctx=anet_ctx, **kw)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(B).astype(np.int32)).to(dev)
    ordered = aa.qp_solve_dev(s, state, tT, thp, settings=cps, launch_order=perm, ctx=anet_ctx, **kw)
    torch.cuda.synchronize()
    for k in ("coeffs", "obj", "status", "iters"):
        assert plain[k].cpu().numpy().tobytes() == first[k].tobytes() == ordered[k].cpu().numpy().tobytes(), k
    # the table cache is keyed by the row form: on a fresh context, control points first and samples at the SAME res afterwards
    sample = aa.qp_solve(s, ini, fin, hp, T, ctx=anet_ctx, **kw)
    assert not np.array_equal(sample["coeffs"], first["coeffs"])
    fresh = aa.Context(0)
    assert _same(first, aa.qp_solve(s, ini, fin, hp, T, settings=cps, ctx=fresh, **kw))
    assert _same(sample, aa.qp_solve(s, ini, fin, hp, T, ctx=fresh, **kw))
    assert _same(first, aa.qp_solve(s, ini, fin, hp, T, settings=cps, ctx=fresh, **kw))
    assert _same(sample, aa.qp_solve(s, ini, fin, hp, T, ctx=anet_ctx, **kw))


def test_large_batches_take_the_two_launch_form_to_the_same_optimum(anet_ctx):
    """The launch-form selection is by (s, N, R, M) and the batch as for the sample form; a batch large enough for the throughput
    kernel in two launches reaches the optimum of the fused kernel.  Both meet the oracle's objective to 1e-5 (the bar of the solve
    test), hence each other's to 2e-5."""
    import allocnet_amd as aa
    s, N, M, K = 4, 3, 8, 1
    ini, fin, hp, T = _batch(s, N, M)
    res = aa.qp.control_point_res(s, K)
    rep = 200
    form = aa.qp.qp_ipm_launch_form(s, N, rep * len(T), res=res, M=M, ctx=anet_ctx)
    assert form & aa.qp.IPM_FORM_TWO_LAUNCHES
    small = _device(anet_ctx, s, N, M, K)
    big = aa.qp_solve(s, *(np.tile(x, (rep,) + (1,) * (x.ndim - 1)) for x in (ini, fin, hp, T)), res=res, max_vel=VMAX, max_acc=AMAX,
                      settings=aa.qp_settings(rows="control_points"), ctx=anet_ctx)
    for k in ("coeffs", "obj", "status", "iters"):                  # every copy of a problem: the same bits
        v = big[k].reshape((rep, len(T)) + big[k].shape[1:])
        assert (v == v[0]).all(), k
    assert np.array_equal(big["status"][:len(T)], small["status"])
    ok = small["status"] == 1
    assert (np.abs(big["obj"][:len(T)] - small["obj"])[ok] <= 2e-5 * np.maximum(1.0, small["obj"][ok])).all()


def test_qpsolver_classes_give_the_coefficients_of_qp_solve(anet_ctx):
    """QPSolver.setRowForm (Python) and QPSolver::setRowForm (tests/cpp/test_qp_row_form.cpp, built as C++14)."""
    import allocnet_amd as aa
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "test_qp_row_form.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "test_qp_row_form")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        for s, N, M, K in [(4, 3, 8, 2), (3, 5, 12, 1)]:
            ini, fin, hp, T = _batch(s, N, M)
            kw = dict(res=aa.qp.control_point_res(s, K), max_vel=VMAX, max_acc=AMAX, rows="control_points", ctx=anet_ctx)
            bb = int(np.flatnonzero(aa.qp_solve(s, ini, fin, hp, T, **kw)["status"] == 1)[0])
            polys = [hp[bb, i][np.abs(hp[bb, i]).sum(axis=1) > 0] for i in range(N)]       # (trailing padding rows dropped)
            Mp = max(len(p) for p in polys)                                              # the classes pad to the longest polytope
            one = aa.qp_solve(s, ini[bb:bb + 1], fin[bb:bb + 1], hp[bb:bb + 1, :, :Mp], T[bb:bb + 1], **kw)
            ref = {k: one[k] for k in ("coeffs", "obj", "iters")}
            bb_in = bb
            ini, fin, T, bb = ini[bb_in:bb_in + 1], fin[bb_in:bb_in + 1], T[bb_in:bb_in + 1], 0
            solver = aa.QPSolver(aa.QPConfig(MaxVelBox=VMAX, MaxAccBox=AMAX, ConstRes=20), ctx=anet_ctx)
            solver.setOrder(s)
            solver.setRowForm("control_points", segments=K)
            ok, sol = solver.solve(ini[bb], fin[bb], polys, T[bb])
            assert ok and np.array_equal(sol, ref["coeffs"][bb].reshape(-1)) and solver.getObjCost() == ref["obj"][bb]
            txt = os.path.join(td, f"case_{s}.txt")
            with open(txt, "w") as f:
                f.write(f"{s} {N} {K}\n")
                for a in (ini[bb], fin[bb], T[bb]):
                    f.write(" ".join("%.17g" % x for x in np.asarray(a).ravel()) + "\n")
                for p in polys:
                    f.write(f"{len(p)}\n" + "".join(" ".join("%.17g" % x for x in r) + "\n" for r in p))
            run = subprocess.run([exe, txt], capture_output=True, text=True, timeout=120)
            assert run.returncode == 0, run.stdout + run.stderr
            got = json.loads(run.stdout.strip().splitlines()[-1])
            assert got["ok"] == 1 and got["obj"] == ref["obj"][bb] and got["iters"] == ref["iters"][bb]
            assert got["coeffs"] == [float(x) for x in ref["coeffs"][bb].reshape(-1)]


def test_device_entry_points_and_the_torch_layer_pass_the_form_through(anet_ctx):
    """qp_solve_dev, qp_solve_vjp_dev and torch_layer.qp_layer with rows="control_points": the host-pointer results (tolerances of
    tests/test_qp_solve_gpu.py:513-521), and the layer's gradient = backward pass + 0.3 x envelope gradient of the same form."""
    import torch
    import allocnet_amd as aa
    from allocnet_amd.torch_layer import qp_layer
    s, N, M = 4, 3, 8
    ini, fin, hp, T = _batch(s, N, M)
    kw = dict(res=aa.qp.control_point_res(s), max_vel=VMAX, max_acc=AMAX, rows="control_points")
    dev = torch.device("cuda", 0)
    state = torch.from_numpy(np.ascontiguousarray(np.stack([ini, fin], axis=1))).to(dev)
    thp = torch.from_numpy(np.ascontiguousarray(hp)).to(dev); tT = torch.from_numpy(T.copy()).to(dev)
    host = aa.qp_solve(s, ini, fin, hp, T, time_grad=True, ctx=anet_ctx, **kw)
    assert np.allclose(host["coeffs"], _device(anet_ctx, s, N, M, 1)["coeffs"], rtol=1e-9, atol=1e-11)     # the same solve + an epilogue
    w = np.random.default_rng(9).normal(size=host["coeffs"].shape[1:])
    gz = np.repeat(w[None], len(T), axis=0)
    hv = aa.qp_solve_vjp(s, ini, fin, hp, T, gz, ctx=anet_ctx, **kw)
    dv = aa.qp_solve_vjp_dev(s, state, tT, thp, torch.from_numpy(gz).to(dev), ctx=anet_ctx, **kw)
    assert np.allclose(dv["grad_T"].cpu().numpy(), hv["grad_T"], rtol=1e-8, atol=1e-10) and np.array_equal(dv["status"].cpu().numpy(), hv["status"])
    times = tT.clone().requires_grad_(True)
    co, obj, st = qp_layer(times, state, thp, order=s, ctx=anet_ctx, **kw)
    assert np.array_equal(st.cpu().numpy(), host["status"])
    assert np.allclose(co.detach().cpu().numpy(), host["coeffs"], rtol=1e-9, atol=1e-11)
    ((torch.from_numpy(w).to(dev) * co).sum() + 0.3 * obj.sum()).backward()
    ok = (host["status"] == 1) & (hv["status"] == 1)
    assert ok.sum() >= 3
    want = hv["grad_T"] + 0.3 * host["grad_T"]
    assert np.allclose(times.grad.cpu().numpy()[ok], want[ok], rtol=1e-8, atol=1e-10)
    # and the sample form is what the layer computes without the keyword
    co_s = qp_layer(tT, state, thp, order=s, res=8, max_vel=VMAX, max_acc=AMAX, ctx=anet_ctx)[0]
    assert not np.allclose(co_s.cpu().numpy(), host["coeffs"], rtol=1e-6)
