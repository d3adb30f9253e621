"""k_traj_clearance on the GPU: against the multiprecision references of tests/golden/traj_clearance_cases.npz at the a-priori
bound of tests/traj_clearance_mp.clearance_bound (met by a float64 restatement of the procedure in
tests/test_traj_clearance_cpu.py); batch shapes, row strides, counts and edge inputs; the voxel map's surface and gather_boxes
end to end; what sampling overestimates; the Python and C++ facades."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import traj_clearance_mp as cl
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, ORIGIN, SCALE = (16, 12, 8), (-2.0, -1.5, 0.0), 0.25


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "traj_clearance_cases.npz"))


def case(fx, i):
    """(cm (3, 2s), T, the points the kernel may use)"""
    s = int(fx["s"][i])
    off = int(fx["npts"][:i].sum())
    pts = fx["pts"][off:off + int(fx["npts"][i])]
    if fx["count"][i] >= 0:
        pts = pts[:int(fx["count"][i])]
    return fx["cm"][i][:, :2 * s], float(fx["T"][i]), pts


@pytest.fixture(scope="module")
def host_answers(anet_ctx, fx):
    """(a)'s answers, computed once: every fixture case alone through the host form -> (clearance, point, t) arrays"""
    import allocnet_amd as aa
    n = len(fx["T"])
    c, p, t = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n)
    for i in range(n):
        cm, T, pts = case(fx, i)
        r = aa.traj_clearance(cm[None, None], np.array([[T]]), pts, ctx=anet_ctx)
        c[i], p[i], t[i] = r[0][0, 0], r[1][0, 0], r[2][0, 0]
    return c, p, t


@pytest.mark.parametrize("s", [2, 3, 4])
def test_clearance_matches_multiprecision_reference(fx, host_answers, s):
    """(a) every case of the fixture through the host form: |clearance - ref| <= bound and clearance >= ref - bound; +inf cases
    exact; the point of the reference where the runner-up is farther than twice the bound; always || p(t) - q_point || reproduces
    the value within the bound and 0 <= t <= T.  That distance is formed by traj_clearance_mp.dist_exact, in exact rational
    arithmetic rounded once, instead of at 60 digits: at least as strict, and no mpmath is needed where this test runs (the CPU
    suite checks dist_exact against the 60-digit dist_mp)."""
    c, p, t = host_answers
    sc = np.array([cl.scales(*case(fx, i)) for i in range(len(fx["T"]))])
    bound = cl.clearance_bound(sc[:, 0], sc[:, 1], fx["speed"], fx["kappa"], fx["d"], fx["interior"])
    worst = {}
    for i in np.flatnonzero(fx["s"] == s):
        cm, T, pts = case(fx, i)
        fam = str(fx["families"][fx["family"][i]])
        if fx["point"][i] < 0:
            assert c[i] == np.inf and p[i] == -1 and t[i] == 0.0, (i, fam)
            continue
        err = abs(c[i] - fx["d"][i])
        worst[fam] = max(worst.get(fam, 0.0), err / bound[i])
        print("case %d %s err %.3g bound %.3g" % (i, fam, err, bound[i]))
        assert err <= bound[i] and c[i] >= fx["d"][i] - bound[i], (i, fam, c[i], fx["d"][i], bound[i])
        assert 0 <= p[i] < len(pts) and 0.0 <= t[i] <= T, (i, fam)
        if fx["runner"][i] - fx["d"][i] > 2.0 * bound[i]:
            assert p[i] == fx["point"][i], (i, fam)
        assert abs(cl.dist_exact(cm, T, t[i], pts[p[i]]) - c[i]) <= bound[i], (i, fam)
    print("s=%d worst |err| / bound per family:" % s, {k: "%.3g" % v for k, v in worst.items()})
    assert len(worst) >= 13


def _sets(fx, ids, pmax):
    """the point sets of the fixture cases ids, padded to pmax rows with junk behind their counts -> (len(ids), pmax, 3), counts"""
    out = np.full((len(ids), pmax, 3), 0.123)
    counts = np.zeros(len(ids), dtype=np.int32)
    for k, i in enumerate(ids):
        pts = case(fx, i)[2][:pmax]
        out[k, :len(pts)] = pts
        counts[k] = len(pts)
    return out, counts


@pytest.mark.parametrize("B", [1, 65, 130])
@pytest.mark.parametrize("N,per_piece", [(1, False), (3, False), (3, True)])
def test_device_form_shapes_strides_and_neighbours(anet_ctx, fx, host_answers, B, N, per_piece):
    """(b) ld = batch + 19 with junk behind the batch, point / t wanted or NULL: nothing is written behind the batch, and every
    (curve, set) problem gives the bits it gives alone through the host form, whatever its neighbours."""
    import allocnet_amd as aa
    import torch
    dev = torch.device("cuda", anet_ctx.device)
    s, ld = 3, B + 19
    ids = np.flatnonzero((fx["s"] == s) & (fx["point"] >= 0))
    curves = ids[(np.arange(B * N) * 7) % len(ids)].reshape(B, N)
    set_ids = ids[[5, 11, 23]][:N] if per_piece else ids[[5]]
    curves[0, 0] = set_ids[0]
    sets, counts = _sets(fx, set_ids, 48)
    coeffs = np.stack([[fx["cm"][i][:, :2 * s] for i in row] for row in curves])
    T = fx["T"][curves]

    def bm(a):
        out = torch.full((a.reshape(B, -1).shape[1], ld), 7.0, device=dev, dtype=torch.float64)
        out[:, :B] = torch.as_tensor(np.ascontiguousarray(a.reshape(B, -1).T), device=dev)
        return out
    d_pts = torch.as_tensor(sets if per_piece else sets[0], device=dev).contiguous()
    d_cnt = torch.as_tensor(counts, device=dev)
    d_c = torch.full((N, ld), -7.0, device=dev, dtype=torch.float64)
    d_p = torch.full((N, ld), -7, device=dev, dtype=torch.int32)
    d_t = torch.full((N, ld), -7.0, device=dev, dtype=torch.float64)
    aa.traj_clearance_dev(bm(coeffs), bm(T), d_pts, s, N, B, counts=d_cnt, clearance=d_c, point=d_p, t=d_t, ctx=anet_ctx)
    torch.cuda.synchronize(dev)
    assert (d_c[:, B:] == -7.0).all() and (d_p[:, B:] == -7).all() and (d_t[:, B:] == -7.0).all()
    d_c2 = torch.full((N, ld), -7.0, device=dev, dtype=torch.float64)
    aa.traj_clearance_dev(bm(coeffs), bm(T), d_pts, s, N, B, counts=d_cnt, clearance=d_c2, point=False, t=False, ctx=anet_ctx)
    torch.cuda.synchronize(dev)
    assert torch.equal(d_c, d_c2)
    c, p, t = d_c[:, :B].T.cpu().numpy(), d_p[:, :B].T.cpu().numpy(), d_t[:, :B].T.cpu().numpy()
    host = aa.traj_clearance(coeffs, T, sets if per_piece else sets[0], counts=counts, ctx=anet_ctx)
    for h, g in zip(host, (c, p, t)):
        assert h.shape == (B, N) and np.array_equal(h, g)
    alone = {}
    for b in range(B):
        for i in range(N):
            key = (int(curves[b, i]), i if per_piece else 0)
            if key not in alone:
                k = key[1]
                r = aa.traj_clearance(coeffs[b, i][None, None], T[b, i].reshape(1, 1), sets[k][:counts[k]], ctx=anet_ctx)
                alone[key] = (r[0][0, 0], r[1][0, 0], r[2][0, 0])
            assert (c[b, i], p[b, i], t[b, i]) == alone[key], (b, i)
    # a curve against its own fixture set reproduces (a) bit for bit
    for b in np.flatnonzero(curves[:, 0] == set_ids[0]):
        assert (c[b, 0], p[b, 0], t[b, 0]) == (host_answers[0][set_ids[0]], host_answers[1][set_ids[0]], host_answers[2][set_ids[0]])


def test_counts_and_edge_inputs(anet_ctx, fx):
    """(c) counts above max_points are clamped; counts NULL uses every row; max_points 0 is +inf; a NaN coefficient, an infinite
    or negative duration poison their piece only; n_sets = 2 with N = 3 and other bad arguments are ANET_ERR_INVALID."""
    import allocnet_amd as aa
    from allocnet_amd import _lib
    s, N, B = 3, 3, 70
    ids = np.flatnonzero((fx["s"] == s) & (fx["point"] >= 0))
    curves = ids[(np.arange(B * N) * 5) % len(ids)].reshape(B, N)
    coeffs = np.stack([[fx["cm"][i][:, :2 * s] for i in row] for row in curves])
    T = fx["T"][curves]
    sets, counts = _sets(fx, ids[[2, 9, 17]], 16)
    counts = np.minimum(counts, 16)
    clean = aa.traj_clearance(coeffs, T, sets, counts=counts, ctx=anet_ctx)
    assert np.isfinite(clean[0]).all()
    # clamped: counts far above the rows == counts NULL == counts equal to the rows
    full = aa.traj_clearance(coeffs, T, sets, counts=np.full(N, 16, dtype=np.int32), ctx=anet_ctx)
    for other in (aa.traj_clearance(coeffs, T, sets, counts=np.array([17, 1000, 2 ** 31 - 1], dtype=np.int32), ctx=anet_ctx),
                  aa.traj_clearance(coeffs, T, sets, ctx=anet_ctx)):
        for a, b in zip(full, other):
            assert np.array_equal(a, b)
    # a negative count is an empty set
    neg = aa.traj_clearance(coeffs, T, sets, counts=np.array([-3, 16, 0], dtype=np.int32), ctx=anet_ctx)
    assert (neg[0][:, [0, 2]] == np.inf).all() and (neg[1][:, [0, 2]] == -1).all() and (neg[2][:, [0, 2]] == 0.0).all()
    assert np.array_equal(neg[0][:, 1], full[0][:, 1])
    # max_points == 0
    c, p, t = aa.traj_clearance(coeffs, T, np.zeros((0, 3)), ctx=anet_ctx)
    assert (c == np.inf).all() and (p == -1).all() and (t == 0.0).all()
    c, p, t = aa.traj_clearance(coeffs, T, np.zeros((N, 0, 3)), ctx=anet_ctx)
    assert (c == np.inf).all() and (p == -1).all() and (t == 0.0).all()
    # poisoned pieces
    bad = np.zeros((B, N), dtype=bool)
    co, Tq = coeffs.copy(), T.copy()
    co[3, 1, 2, 4] = np.nan; bad[3, 1] = True
    co[64, 0, 0, 0] = np.inf; bad[64, 0] = True
    co[65, 2, 1, 5] = -np.inf; bad[65, 2] = True
    Tq[10, 2] = np.nan; bad[10, 2] = True
    Tq[11, 0] = np.inf; bad[11, 0] = True
    Tq[12, 1] = -0.5; bad[12, 1] = True
    c, p, t = aa.traj_clearance(co, Tq, sets, counts=counts, ctx=anet_ctx)
    assert np.isnan(c[bad]).all() and (p[bad] == -1).all() and (t[bad] == 0.0).all()
    for a, b in zip((c, p, t), clean):
        assert np.array_equal(a[~bad], b[~bad])
    # T = 0: the point p(0)
    c, p, t = aa.traj_clearance(coeffs, np.zeros_like(T), sets, counts=counts, ctx=anet_ctx)
    fin = [sets[i, :counts[i]][np.isfinite(sets[i, :counts[i]]).all(axis=1)] for i in range(N)]
    want = np.array([[np.linalg.norm(fin[i] - coeffs[b, i, :, -1], axis=1).min() for i in range(N)] for b in range(B)])
    assert np.allclose(c, want, rtol=0, atol=1e-13) and (t == 0.0).all()
    # argument checks
    lib, h = anet_ctx.lib, anet_ctx.handle
    q = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((1, N))

    def call(s_, n_, b_, nsets_, maxp_, pts_=q(sets)):
        return lib.anet_traj_clearance(h, s_, n_, b_, q(coeffs), q(T), nsets_, maxp_, pts_, None, q(out), None, None)
    assert call(3, N, 1, N, 16) == _lib.ANET_OK and np.array_equal(out[0], full[0][0])          # point, t = NULL
    assert call(3, N, 1, 1, 16) == _lib.ANET_OK
    for args in ((3, N, 1, 2, 16), (3, N, 1, 0, 16), (3, N, 1, N, -1), (3, N, 1, N, 2 ** 31), (5, N, 1, N, 16), (1, N, 1, N, 16),
                 (3, 17, 1, 17, 16), (3, 0, 1, 1, 16), (3, N, -1, N, 16)):
        assert call(*args) == _lib.ANET_ERR_INVALID, args
    assert call(3, N, 1, N, 16, None) == _lib.ANET_ERR_INVALID
    assert call(3, N, 1, N, 0, None) == _lib.ANET_OK and (out == np.inf).all()
    assert lib.anet_traj_clearance(h, 3, N, 0, None, None, N, 16, None, None, None, None, None) == _lib.ANET_OK
    assert lib.anet_traj_clearance(h, 3, N, 0, None, None, 2, 16, None, None, None, None, None) == _lib.ANET_ERR_INVALID
    assert lib.anet_traj_clearance_dev(h, 3, N, 4, 3, q(coeffs), q(T), N, 16, q(sets), None, q(out), None, None, None) == _lib.ANET_ERR_INVALID


def _map_and_pieces(anet_ctx):
    """the 16 x 12 x 8 map filled at random to 3 % and dilated once; 40 trajectories of 3 order-3 pieces, piece i inside the
    i-th third of the map along x; the three boxes (6 rows h . [p; 1] < 0 inside) that hold those thirds and 0.5 m around them"""
    import allocnet_amd as aa
    rng = np.random.default_rng(77)
    vm = aa.VoxelMap(SIZE, ORIGIN, SCALE, ctx=anet_ctx)
    ids = np.argwhere(rng.random(SIZE) < 0.03)
    vm.setOccupied(ids.astype(np.int32))
    vm.dilate(1)
    B, N, D = 40, 3, 6
    lo, hi = np.array(ORIGIN), np.array(ORIGIN) + np.array(SIZE) * SCALE
    third = (hi[0] - lo[0]) / 3.0
    from math import comb
    coeffs = np.zeros((B, N, 3, D))
    T = rng.uniform(0.4, 2.5, (B, N))
    bd = np.zeros((N, 6, 4))
    for i in range(N):
        blo = np.array([lo[0] + i * third, lo[1], lo[2]])
        bhi = np.array([lo[0] + (i + 1) * third, hi[1], hi[2]])
        for ax in range(3):
            bd[i, 2 * ax, ax], bd[i, 2 * ax, 3] = 1.0, -(bhi[ax] + 0.5)
            bd[i, 2 * ax + 1, ax], bd[i, 2 * ax + 1, 3] = -1.0, blo[ax] - 0.5
        for b in range(B):
            bq = rng.uniform(blo + 0.1, bhi - 0.1, (D, 3)).T
            for ax in range(3):
                for k in range(D):
                    u = sum(comb(D - 1, k) * comb(k, j) * (-1) ** (k - j) * bq[ax, j] for j in range(k + 1))
                    coeffs[b, i, ax, D - 1 - k] = u / T[b, i] ** k
    return vm, coeffs, T, bd


def test_voxel_map_surface_and_gather_boxes_end_to_end(anet_ctx):
    """(d) The output of gather_boxes, fed straight in (device tensors, counts as they come), agrees with the shared-cloud call
    wherever the shared call's minimising point lies in the piece's box; the sampled route (21 samples per piece, traj_eval and a
    distance matrix) is never below the exact clearance minus the bound, and lies above it somewhere."""
    import allocnet_amd as aa
    import torch
    vm, coeffs, T, bd = _map_and_pieces(anet_ctx)
    B, N = T.shape
    surf = vm.getSurf()
    assert len(surf) > 100
    shared = aa.traj_clearance(coeffs, T, vm, ctx=anet_ctx)
    again = aa.traj_clearance(coeffs, T, surf, ctx=anet_ctx)
    for a, b in zip(shared, again):
        assert np.array_equal(a, b)                     # the device cloud and its host copy: the same bits
    pc, counts = vm.gather_boxes(bd)
    assert pc.is_cuda and tuple(pc.shape[::2]) == (N, 3) and (counts > 20).all()
    boxed = aa.traj_clearance(coeffs, T, pc, counts=counts, ctx=anet_ctx)
    assert np.isfinite(shared[0]).all() and np.isfinite(boxed[0]).all()
    pch = pc.cpu().numpy()
    n_in = 0
    for b in range(B):
        for i in range(N):
            q = surf[shared[1][b, i]]
            bound = cl.bound_float64(coeffs[b, i], T[b, i], surf, shared[1][b, i], shared[2][b, i], shared[0][b, i])
            assert bound <= cl.CAP
            assert boxed[0][b, i] >= shared[0][b, i] - 2.0 * bound          # a subset of the cloud
            if (bd[i, :, :3] @ q + bd[i, :, 3] < 0.0).all():
                n_in += 1
                assert abs(boxed[0][b, i] - shared[0][b, i]) <= 2.0 * bound, (b, i)
                qb = pch[i, boxed[1][b, i]]
                assert abs(cl.dist_exact(coeffs[b, i], T[b, i], boxed[2][b, i], qb) - boxed[0][b, i]) <= bound
    assert n_in > B * N // 2
    # the sampled route
    knots = np.cumsum(T, axis=1)
    tq = (knots - T)[:, :, None] + T[:, :, None] * np.linspace(0.0, 1.0, 21)[None, None]
    pos = aa.traj_eval(coeffs, T, np.minimum(tq.reshape(B, -1), knots[:, -1:]), 0, ctx=anet_ctx).reshape(B, N, 21, 3)
    # (a sample on a junction belongs to the earlier piece for traj_eval: the first sample of pieces 1.. is taken from Horner)
    for b in range(B):
        for i in range(1, N):
            pos[b, i, 0] = coeffs[b, i, :, -1]
    d = torch.cdist(torch.as_tensor(pos.reshape(-1, 3)), torch.as_tensor(surf)).min(dim=1).values.reshape(B, N, 21).min(dim=2).values.numpy()
    assert (d >= shared[0] - 1e-9).all()
    over = d - shared[0]
    print("sampled minus exact clearance: median %.3g m, worst %.3g m" % (np.median(over), over.max()))
    assert over.max() > 1e-4


def test_python_facade(anet_ctx):
    """(e) Trajectory / Piece getClearance, checkClearance on the map, on a cloud and on per-piece sets."""
    import allocnet_amd as aa
    vm, coeffs, T, bd = _map_and_pieces(anet_ctx)
    surf = vm.getSurf()
    c, p, t = aa.traj_clearance(coeffs[:1], T[:1], vm, ctx=anet_ctx)
    traj = aa.Trajectory(list(T[0]), list(coeffs[0]), ctx=anet_ctx)
    cc, pp, tt = traj.getClearance(vm, per_piece=True)
    assert np.array_equal(cc, c[0]) and np.array_equal(pp, p[0]) and np.array_equal(tt, t[0])
    i = int(np.argmin(c[0]))
    start = float(np.sum(T[0, :i]))
    assert traj.getClearance(vm) == (float(c[0, i]), start + float(t[0, i]), i, int(p[0, i]))
    assert traj.getClearance(surf) == traj.getClearance(vm)
    assert traj[1].getClearance(vm) == (float(c[0, 1]), float(t[0, 1]), int(p[0, 1]))
    assert traj.checkClearance(vm, float(c[0, i])) and not traj.checkClearance(vm, float(c[0, i]) * (1 + 1e-12) + 1e-300)
    assert traj[1].checkClearance(surf, float(c[0, 1])) and not traj[1].checkClearance(surf, float(c[0, 1]) + 1e-9)
    pc, counts = vm.gather_boxes(bd)
    cb = traj.getClearance(pc, per_piece=True)[0]
    assert (cb >= c[0] - 1e-9).all()
    assert traj.getClearance(np.zeros((0, 3))) == (np.inf, 0.0, -1, -1) and traj.checkClearance(np.zeros((0, 3)), 1e9)
    bad = aa.Trajectory([1.0, 1.0], [coeffs[0, 0], np.full((3, 6), np.nan)], ctx=anet_ctx)
    assert np.isnan(bad.getClearance(surf)[0]) and bad.getClearance(surf)[2] == 1 and not bad.checkClearance(surf, 0.0)


def test_cpp_facade_program(anet_ctx):
    """(e) tests/cpp/test_traj_clearance.cpp: getClearance / checkClearance on a trajectory and on its pieces, against a vector of
    points, against the map's surface and against no point, print (%.17g) what the Python facade returns."""
    import allocnet_amd as aa
    rng = np.random.default_rng(78)
    vm, coeffs, T, bd = _map_and_pieces(anet_ctx)
    ids = np.argwhere(np.random.default_rng(77).random(SIZE) < 0.03)
    cloud = np.round(rng.uniform(np.array(ORIGIN), np.array(ORIGIN) + np.array(SIZE) * SCALE, (30, 3)) * 1024) / 1024
    traj = aa.Trajectory(list(T[1]), list(coeffs[1]), ctx=anet_ctx)
    src = os.path.join(ROOT, "tests", "cpp", "test_traj_clearance.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    min_dist = 0.2
    with tempfile.TemporaryDirectory() as td:
        exe, txt = os.path.join(td, "test_traj_clearance"), os.path.join(td, "case.txt")
        with open(txt, "w") as f:
            f.write("%d %d %d %.17g %.17g %.17g %.17g\n%d\n" % (SIZE + ORIGIN + (SCALE, len(ids))))
            for v in ids:
                f.write("%d %d %d\n" % tuple(v))
            f.write("1 %d\n" % len(cloud))
            for q in cloud:
                f.write("%.17g %.17g %.17g\n" % tuple(q))
            f.write("%.17g %d\n" % (min_dist, T.shape[1]))
            for d, m in zip(T[1], coeffs[1]):
                f.write("%.17g\n" % d + " ".join("%.17g" % x for x in m.ravel()) + "\n")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe, txt], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads(res.stdout)
    for name, pts in (("points", cloud), ("map", vm)):
        d, t, piece, point = traj.getClearance(pts)
        o = out[name]
        assert (o["d"], o["t"], o["piece"], o["point"]) == (d, t, piece, point), name
        assert o["ok"] == int(traj.checkClearance(pts, min_dist))
        for i in range(T.shape[1]):
            dp, tp, pp = traj[i].getClearance(pts)
            assert o["pieces"][i] == [dp, tp, pp, int(traj[i].checkClearance(pts, min_dist))], (name, i)
    o = out["none"]
    assert o["d"] == np.inf and o["t"] == 0.0 and o["piece"] == -1 and o["point"] == -1 and o["ok"] == 1
