"""k_traj_row_margin on the GPU: against the multiprecision references of tests/golden/corridor_margin_cases.npz at the a-priori
float64 bound of tests/corridor_margin_mp.margin_bound (met by a float64 restatement of the procedure in
tests/test_corridor_margin_cpu.py); batch shapes, row strides, edge inputs; the sampled view of the same constraints; the host
and device entry points; the Python and C++ facades."""
import ctypes
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import corridor_margin_mp as cmm
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "corridor_margin_cases.npz"))


def _fill(fx, s, d, B, N, M, seed=0):
    """B x N slots filled by cycling through the fixture cases of (s, d) with a stride coprime to their number; the rows of a
    case go to M slots in a shuffled order (its padding rows and M - 5 more among them).  Returns the case of every slot, the
    inputs, and for every slot the position its reference row went to."""
    idx = np.flatnonzero((fx["s"] == s) & (fx["d"] == d))
    stride = next(k for k in range(7, 7 + len(idx)) if math.gcd(k, len(idx)) == 1)
    slot = idx[(np.arange(B * N) * stride) % len(idx)].reshape(B, N)
    assert set(slot.ravel()) == set(idx)
    rng = np.random.default_rng(100 * s + 10 * d + seed)
    R = fx["rows"].shape[1]
    rows = np.zeros((B, N, M, 4))
    ref_row = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        for i in range(N):
            perm = rng.permutation(M)[:R]
            rows[b, i, perm] = fx["rows"][slot[b, i]]
            if fx["ref_row"][slot[b, i]] >= 0:
                ref_row[b, i] = perm[fx["ref_row"][slot[b, i]]]
    return slot, fx["cm"][slot][..., :2 * s].copy(), fx["T"][slot].copy(), rows, ref_row


def _check_against_reference(fx, slot, coeffs, T, rows, ref_row, d, got, row, t, what):
    ref, bound = fx["ref"][slot], cmm.margin_bound(fx["scale"][slot])
    empty = fx["family"][slot] == "empty"
    assert (got[empty] == -np.inf).all() and (row[empty] == -1).all() and (t[empty] == 0.0).all(), what
    ratio = np.abs(got[~empty] - ref[~empty]) / bound[~empty]
    fam = fx["family"][slot][~empty]
    print(what, "worst |err| / bound per family:", {str(f): round(float(ratio[fam == f].max()), 4) for f in np.unique(fam)})
    with np.errstate(invalid="ignore"):      # (-inf) - (-inf) in the empty slots, excluded
        bad = np.argwhere(~empty & ~(np.abs(got - ref) <= bound))
    assert len(bad) == 0, (what, [(int(b), int(i), str(fx["family"][slot[b, i]]), got[b, i], ref[b, i]) for b, i in bad[:8]])
    decided = ~empty & (fx["gap"][slot] > 4.0 * bound)
    assert decided.sum() > 0.5 * decided.size and (row[decided] == ref_row[decided]).all(), what
    assert ((row >= 0) | empty).all() and (0.0 <= t).all() and (t <= T).all(), what
    for b, i in np.argwhere(~empty):
        g = cmm.g_float64(coeffs[b, i], T[b, i], d, rows[b, i, row[b, i]], t[b, i])
        assert abs(g - got[b, i]) <= bound[b, i], (what, b, i, g, got[b, i], bound[b, i])


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_margin_matches_multiprecision_reference(anet_ctx, fx, s, d):
    """Every lane of two full 64-lane blocks and a 7-lane tail, three piece rows, five row slots, against the 60-digit
    reference: |margin - ref| <= 32 eps scale; the row where the gap to the second row exceeds four bounds; (row, t)
    reproduce the margin within one bound."""
    import allocnet_amd as aa
    B, N, M = 135, 3, 5
    slot, coeffs, T, rows, ref_row = _fill(fx, s, d, B, N, M)
    got, row, t = aa.traj_row_margin(coeffs, T, rows, d, ctx=anet_ctx)
    _check_against_reference(fx, slot, coeffs, T, rows, ref_row, d, got, row, t, "s=%d d=%d" % (s, d))


def _dev_call(anet_ctx, coeffs, T, rows, d, ld, want_diag=True):
    """anet_traj_row_margin_dev on torch tensors of row stride ld -> (margin, row, t) as (B, N) arrays"""
    import torch
    dev = torch.device("cuda", anet_ctx.device)
    B, N, _, D = coeffs.shape
    M = rows.shape[2]

    def bm(a, dtype=torch.float64):
        out = torch.full((a.reshape(B, -1).shape[1], ld), 7.0, device=dev, dtype=dtype)     # the tail columns hold junk
        out[:, :B] = torch.as_tensor(np.ascontiguousarray(a.reshape(B, -1).T), device=dev)
        return out
    d_co, d_T, d_rows = bm(coeffs), bm(T), bm(rows)
    d_m = torch.full((N, ld), -7.0, device=dev, dtype=torch.float64)
    d_t = torch.full((N, ld), -7.0, device=dev, dtype=torch.float64)
    d_r = torch.full((N, ld), -7, device=dev, dtype=torch.int32)
    q = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    anet_ctx.check(anet_ctx.lib.anet_traj_row_margin_dev(anet_ctx.handle, D // 2, N, B, ld, q(d_co), q(d_T), d, M, q(d_rows), q(d_m),
                                                         q(d_r) if want_diag else None, q(d_t) if want_diag else None, stream))
    torch.cuda.synchronize(dev)
    # nothing is written behind the batch
    assert (d_m[:, B:] == -7.0).all() and (d_t[:, B:] == -7.0).all() and (d_r[:, B:] == -7).all()
    if not want_diag:
        assert (d_t == -7.0).all() and (d_r == -7).all()
    return d_m[:, :B].T.cpu().numpy(), d_r[:, :B].T.cpu().numpy(), d_t[:, :B].T.cpu().numpy()


@pytest.mark.parametrize("B", [1, 64, 65])
def test_batch_shapes_strides_and_neighbours(anet_ctx, fx, B):
    """ld = batch + 19; host and device entry points return identical bits; a problem gives the same bits alone, among
    other problems and at another place in the batch."""
    import allocnet_amd as aa
    s, d, N, M = 3, 0, 3, 5
    slot, coeffs, T, rows, ref_row = _fill(fx, s, d, 65, N, M, seed=1)
    co, Tb, rw = coeffs[:B], T[:B], rows[:B]
    host = aa.traj_row_margin(co, Tb, rw, d, ctx=anet_ctx)
    devr = _dev_call(anet_ctx, co, Tb, rw, d, B + 19)
    for h, g in zip(host, devr):
        assert h.shape == (B, N) and np.array_equal(h, g)
    _check_against_reference(fx, slot[:B], co, Tb, rw, ref_row[:B], d, *host, "B=%d" % B)
    assert np.array_equal(_dev_call(anet_ctx, co, Tb, rw, d, B + 19, want_diag=False)[0], host[0])
    # alone, and reversed in the batch
    alone = aa.traj_row_margin(co[B - 1:B], Tb[B - 1:B], rw[B - 1:B], d, ctx=anet_ctx)
    rev = aa.traj_row_margin(co[::-1], Tb[::-1], rw[::-1], d, ctx=anet_ctx)
    for h, a1, r in zip(host, alone, rev):
        assert np.array_equal(h[B - 1:B], a1) and np.array_equal(h, r[::-1])


def test_largest_instantiation(anet_ctx, fx):
    """N = 16 pieces, M = 50 rows, order 4, B = 65, all three derivative orders."""
    import allocnet_amd as aa
    for d in (0, 1, 2):
        slot, coeffs, T, rows, ref_row = _fill(fx, 4, d, 65, 16, 50)
        got, row, t = aa.traj_row_margin(coeffs, T, rows, d, ctx=anet_ctx)
        _check_against_reference(fx, slot, coeffs, T, rows, ref_row, d, got, row, t, "N=16 M=50 d=%d" % d)


def test_edge_inputs(anet_ctx, fx):
    """No rows: -inf / -1 / 0.  A NaN or infinite coefficient, duration or row field: NaN for that piece and the reference for
    every other one.  Argument checks."""
    import allocnet_amd as aa
    from allocnet_amd import _lib
    s, d, B, N, M = 3, 0, 70, 3, 5
    slot, coeffs, T, rows, ref_row = _fill(fx, s, d, B, N, M, seed=2)
    clean = aa.traj_row_margin(coeffs, T, rows, d, ctx=anet_ctx)
    hit = np.zeros((B, N), dtype=bool)
    co, Tq, rw = coeffs.copy(), T.copy(), rows.copy()
    co[3, 1, 2, 4] = np.nan; hit[3, 1] = True
    co[64, 0, 0, 0] = np.inf; hit[64, 0] = True
    Tq[10, 2] = np.nan; hit[10, 2] = True
    Tq[11, 0] = np.inf; hit[11, 0] = True
    real = np.argwhere(np.any(rw != 0.0, axis=3))
    for k, (val, f) in enumerate(((np.nan, 0), (np.inf, 3), (-np.inf, 1))):
        b, i, r = real[len(real) * (k + 1) // 4]
        rw[b, i, r, f] = val; hit[b, i] = True
    got, row, t = aa.traj_row_margin(co, Tq, rw, d, ctx=anet_ctx)
    assert np.isnan(got[hit]).all() and (row[hit] == -1).all() and (t[hit] == 0.0).all()
    for g, c in zip((got, row, t), clean):
        assert np.array_equal(g[~hit], c[~hit])
    # the lowest coefficients do not enter a derivative's value, but a NaN there still marks the piece
    co = coeffs.copy(); co[5, 0, 1, -1] = np.nan
    assert np.isnan(aa.traj_row_margin(co, T, rows, 2, ctx=anet_ctx)[0][5, 0])
    none = aa.traj_row_margin(coeffs[:2], T[:2], np.zeros((2, N, 1, 4)), d, ctx=anet_ctx)
    assert (none[0] == -np.inf).all() and (none[1] == -1).all() and (none[2] == 0.0).all()
    lib, h = anet_ctx.lib, anet_ctx.handle
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    m = np.zeros((1, N))
    call = lambda s_, n_, b_, d_, m_: lib.anet_traj_row_margin(h, s_, n_, b_, p(coeffs), p(T), d_, m_, p(rows), p(m), None, None)
    assert call(3, N, 1, 0, M) == _lib.ANET_OK
    for args in ((5, N, 1, 0, M), (1, N, 1, 0, M), (3, 17, 1, 0, M), (3, 0, 1, 0, M), (3, N, -1, 0, M), (3, N, 1, 3, M),
                 (3, N, 1, -1, M), (3, N, 1, 0, 0), (3, N, 1, 0, 51)):
        assert call(*args) == _lib.ANET_ERR_INVALID, args
    assert lib.anet_traj_row_margin(h, 3, N, 0, None, None, 0, M, None, None, None, None) == _lib.ANET_OK
    assert lib.anet_traj_row_margin(h, 3, N, 1, None, p(T), 0, M, p(rows), p(m), None, None) == _lib.ANET_ERR_INVALID
    assert lib.anet_traj_row_margin_dev(h, 3, N, 4, 3, p(coeffs), p(T), 0, M, p(rows), p(m), None, None, None) == _lib.ANET_ERR_INVALID


def test_between_the_samples_through_qp_margins(anet_ctx, fx):
    """The `between` family: every inequality QPSolver::solve would sample at j/20 holds there, and the exact margin of its
    group is positive and within the bound of the reference."""
    import allocnet_amd as aa
    lim = 1.5
    for d in (0, 1, 2):
        sel = np.flatnonzero((fx["family"] == "between") & (fx["d"] == d) & (fx["s"] == 3))
        assert len(sel) == 3
        co, T = fx["cm"][sel][None, :, :, :6], fx["T"][sel][None]
        far = np.zeros((1, 3, 5, 4)); far[..., 0, 0] = 1.0; far[..., 0, 3] = 1e6
        hp = fx["rows"][sel][None] if d == 0 else far
        limits = (1e6, 1e6) if d == 0 else (lim, 1e6) if d == 1 else (1e6, lim)
        box = aa.trajectory.box_rows(lim)
        for k, i in enumerate(sel):
            rows = fx["rows"][i] if d == 0 else box
            assert d == 0 or np.array_equal(rows[:5], fx["rows"][i])
            sampled = max(cmm.g_float64(co[0, k], T[0, k], d, row, j * T[0, k] / 20.0) for j in range(21) for row in rows
                          if not cmm.is_padding(row))
            assert sampled <= 0.0
        margins = aa.traj_qp_margins(co, T, hp, *limits, ctx=anet_ctx)
        got = margins[d][0]
        assert (got > 0.0).all() and (np.abs(got - fx["ref"][sel]) <= cmm.margin_bound(fx["scale"][sel])).all(), (d, got)
        for other in range(3):
            assert other == d or (margins[other] < 0.0).all()


def test_never_below_dense_sampling(anet_ctx):
    """minco_solve output in synthetic corridors, 70 trajectories: at 400 times over each trajectory the constraint values
    from traj_eval never exceed the exact margin of the piece the time falls in.  Tolerance: the local time is the query less
    up to eight durations (8 eps x 16 s = 3e-14 s) times a rate of change of the constrained quantity below 300 per second
    (asserted), 1e-11, plus the bound of the margin itself (1e-13 relative covers it here).  Rows are normalised."""
    import allocnet_amd as aa
    from allocnet_amd.synth import corridor_problem
    rng = np.random.default_rng(11)
    B, N, M, s = 70, 8, 12, 3
    head, tail, wps, T, hp = corridor_problem(rng, B, N, 3, M)
    coeffs, _ = aa.minco_solve(head, tail, wps, T, s, ctx=anet_ctx)
    for d, rows in ((0, hp), (1, np.broadcast_to(aa.trajectory.box_rows(2.0), (B, N, 6, 4)))):
        margin, row, t = aa.traj_row_margin(coeffs, T, rows, d, ctx=anet_ctx)
        knots = np.cumsum(T, axis=1)
        tq = np.linspace(0.0, 1.0, 400)[None] * knots[:, -1:]
        val = aa.traj_eval(coeffs, T, tq, d, ctx=anet_ctx)
        piece = np.minimum((tq[:, :, None] > knots[:, None, :]).sum(axis=2), N - 1)           # locatePieceIdx
        rq = np.take_along_axis(rows, piece[:, :, None, None], axis=1)                       # (B, nq, M, 4)
        g = np.einsum("bqmk,bqk->bqm", rq[..., :3], val) - rq[..., 3]
        g = np.where(np.any(rq != 0.0, axis=3), g, -np.inf).max(axis=2)
        top = np.full((B, N), -np.inf)
        np.maximum.at(top, (np.arange(B)[:, None].repeat(400, 1), piece), g)
        assert np.abs(aa.traj_eval(coeffs, T, tq, d + 1, ctx=anet_ctx)).max() < 300.0
        assert (top <= margin + 1e-11 + 1e-13 * np.abs(margin)).all()
        assert (top > margin - 0.5).mean() > 0.5          # the samples come close: the margin is no loose bound
        assert (row >= 0).all() and (t >= 0).all() and (t <= T).all()


def test_python_facade(anet_ctx, fx):
    """Trajectory.getCorridorMargin / checkCorridor flip between tol = margin -+ bound; Piece.getCorridorMargin; checkBoxLimits
    against the per-axis maxima the reference implies (between family: max |v_ax| = limit + margin)."""
    import allocnet_amd as aa
    sel = np.flatnonzero((fx["s"] == 3) & (fx["d"] == 0) & np.isin(fx["family"], ["interior", "graze", "cheb"]))[[0, 4, 7]]
    polys = [fx["rows"][i][np.any(fx["rows"][i] != 0.0, axis=1)] for i in sel]
    traj = aa.Trajectory([fx["T"][i] for i in sel], [fx["cm"][i][:, :6] for i in sel], ctx=anet_ctx)
    ref = fx["ref"][sel].max()
    bound = float(cmm.margin_bound(fx["scale"][sel]).max())
    m = traj.getCorridorMargin(polys)
    assert abs(m - ref) <= bound
    per, row, t = traj.getCorridorMargin(polys, per_piece=True)
    assert (np.abs(per - fx["ref"][sel]) <= cmm.margin_bound(fx["scale"][sel])).all() and per.max() == m
    assert row.dtype == np.int32 and t.shape == (3,)
    assert traj.checkCorridor(polys, tol=ref + bound) and not traj.checkCorridor(polys, tol=ref - bound)
    assert traj.checkCorridor(polys) == (m <= 0.0)
    for k, i in enumerate(sel):
        assert traj[k].getCorridorMargin(polys[k]) == per[k]
    with pytest.raises(ValueError):
        traj.getCorridorMargin(polys[:2])
    for d in (1, 2):
        for i in np.flatnonzero((fx["family"] == "between") & (fx["d"] == d) & (fx["s"] == 3)):
            one = aa.Trajectory([fx["T"][i]], [fx["cm"][i][:, :6]], ctx=anet_ctx)
            peak, b2 = 1.5 + fx["ref"][i], 2.0 * float(cmm.margin_bound(fx["scale"][i]))
            lims = lambda x: (x, 1e6) if d == 1 else (1e6, x)
            assert one.checkBoxLimits(*lims(peak + b2)) and not one.checkBoxLimits(*lims(peak - b2))
            assert not one.checkBoxLimits(*lims(1.5))          # every sample at j/20 is inside this box


def test_cpp_facade_program(anet_ctx, fx):
    """tests/cpp/test_corridor_margin.cpp: both overloads of Piece / Trajectory::getCorridorMargin and checkCorridor print
    (%.17g) what the Python facade returns."""
    import allocnet_amd as aa
    sel = np.flatnonzero((fx["s"] == 3) & (fx["d"] == 0) & np.isin(fx["family"], ["interior", "endpoint", "pad", "cheb"]))[[1, 3, 6, 8]]
    polys = [fx["rows"][i][np.any(fx["rows"][i] != 0.0, axis=1)] for i in sel]
    traj = aa.Trajectory([fx["T"][i] for i in sel], [fx["cm"][i][:, :6] for i in sel], ctx=anet_ctx)
    per = traj.getCorridorMargin(polys, per_piece=True)[0]
    tol = float(per.max()) + 1e-9
    src = os.path.join(ROOT, "tests", "cpp", "test_corridor_margin.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        exe, txt = os.path.join(td, "test_corridor_margin"), os.path.join(td, "case.txt")
        with open(txt, "w") as f:
            f.write("%d\n" % len(sel))
            for i, h in zip(sel, polys):
                f.write("%.17g\n" % fx["T"][i] + " ".join("%.17g" % x for x in fx["cm"][i][:, :6].ravel()) + "\n")
                f.write(f"{len(h)}\n" + "".join(" ".join("%.17g" % x for x in r) + "\n" for r in h))
            f.write("%.17g\n" % tol)
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe, txt], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads(res.stdout)
    assert out["margin"] == out["margin_plain"] == float(per.max())
    assert out["per_piece"] == [float(x) for x in per]
    assert out["pieces"] == [[float(x), float(x)] for x in per]
    assert out["check_default"] == int(per.max() <= 0.0) and out["check_tol"] == 1 and out["check_plain_tol"] == 1
