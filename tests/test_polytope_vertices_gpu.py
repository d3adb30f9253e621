"""anet_polytope_vertices (geo_utils::enumerateVs on the device) against tests/polytope_np.py: positions, counts and active rows
against HiGHS + Qhull, the order against the plain numpy enumeration of row triples -- never against the kernel itself.

Position tolerance 1e-8 * max(1, |v|_inf): every triple that produces a vertex of these inputs has |det| >= 1e-3 (asserted with
the numpy enumeration), so the solve's error is below about 4 / |det| * 10 eps_mach * |v| = 4e-10 at 50 m; 1e-8 leaves a factor 20
and is 100 times finer than the merge resolution."""
import ctypes
import functools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import polytope_np as pnp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLIDS = {"cube": (pnp.cube, 8), "tetrahedron": (pnp.tetrahedron, 4), "octahedron": (pnp.octahedron, 6),
          "dressed_cube": (pnp.dressed_cube, 8), "cone": (pnp.cone, 41), "cone_shifted": (lambda: pnp.cone((37.0, -41.0, 3.0)), 41),
          "sphere_50": (lambda: pnp.sphere_tangents(50, 5), 96), "sphere_64": (lambda: pnp.sphere_tangents(64, 6), 124),
          "sphere_65": (lambda: pnp.sphere_tangents(65, 7), 126), "sphere_128": (lambda: pnp.sphere_tangents(128, 8), 252)}
EMPTY = np.array([[1.0, 0.0, 0.0, 1.0], [-1.0, 0.0, 0.0, 1.0]])
FLAT = np.vstack([pnp.box([-1.0] * 3, [1.0] * 3), [[1.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0]]])
SLAB = np.array([[1.0, 0.0, 0.0, -1.0], [-1.0, 0.0, 0.0, -1.0]])


@functools.lru_cache(maxsize=None)
def _solid(name):
    """(hpoly, Qhull's vertices, the numpy enumeration's vertices in order, its smallest |det|), computed once."""
    h = SOLIDS[name][0]()
    ve, min_det = pnp.enumerate_triples(h)
    return h, pnp.vertices_qhull(h), ve, min_det


@functools.lru_cache(maxsize=None)
def _corridors():
    hp = pnp.corridor_polytopes()
    return hp, [pnp.vertices_qhull(h) for h in hp], [pnp.enumerate_triples(h) for h in hp]


def _tol(ref):
    return 1e-8 * np.maximum(1.0, np.abs(ref).max(1))


def _check(name, v, act, h, vq, ve, min_det):
    """positions against Qhull, order against the numpy enumeration, active rows against the residual test at Qhull's vertices"""
    assert min_det >= 1e-3, (name, min_det)
    assert len(v) == len(vq) == len(ve), (name, len(v), len(vq), len(ve))
    idx = pnp.match(v, vq)
    assert sorted(idx.tolist()) == list(range(len(vq))), name
    err_q, err_e = np.abs(v - vq[idx]).max(1), np.abs(v - ve).max(1)
    print(f"{name}: {len(v)} vertices, min |det| {min_det:.3g}, max error vs Qhull {err_q.max():.3g}, vs the enumeration {err_e.max():.3g}")
    assert (err_q <= _tol(vq[idx])).all(), name
    assert (err_e <= _tol(ve)).all(), name                                     # the same vertex at the same place of the list
    if act is not None:
        assert np.array_equal(act, pnp.active_rows(h, vq[idx])), name


@pytest.mark.parametrize("name", list(SOLIDS))
def test_known_solids_cone_and_spheres(anet_ctx, name):
    import allocnet_amd as aa
    h, vq, ve, min_det = _solid(name)
    assert len(vq) == SOLIDS[name][1]
    (v,), (act,), status = aa.polytope_vertices([h], with_active=True, ctx=anet_ctx)
    assert status[0] == 0
    _check(name, v, act, h, vq, ve, min_det)
    assert (np.array([bin(int(a[0])).count("1") + bin(int(a[1])).count("1") for a in act]) >= 3).all()
    if name == "cone_shifted":
        v0 = aa.polytope_vertices([_solid("cone")[0]], ctx=anet_ctx)[0][0]
        assert np.abs(v - (v0 + [37.0, -41.0, 3.0])).max() <= 1e-8 * 41.0
    ok, v1 = aa.enumerate_vs(h, ctx=anet_ctx)
    assert ok and np.array_equal(v1, v)


def test_random_corridor_polytopes(anet_ctx):
    import allocnet_amd as aa
    from scipy.spatial import ConvexHull
    hp, vqs, ves = _corridors()
    vs, acts, status = aa.polytope_vertices(hp, with_active=True, ctx=anet_ctx)
    assert (status == 0).all()
    worst = 0.0
    for b in range(len(hp)):
        assert 8 <= len(vqs[b]) <= 18
        _check(f"corridor {b}", vs[b], acts[b], hp[b], vqs[b], ves[b][0], ves[b][1])
        faces = aa.polytope_faces(hp[b], vs[b], acts[b])
        edges = {frozenset((f[i], f[(i + 1) % len(f)])) for f in faces.values() for i in range(len(f))}
        assert len(vs[b]) - len(edges) + len(faces) == 2, b
        vol = ConvexHull(vqs[b]).volume
        worst = max(worst, abs(aa.polytope_volume(hp[b], vs[b], acts[b]) - vol) / vol)
    print(f"largest relative volume error against ConvexHull: {worst:.3g}")
    assert worst <= 1e-9
    assert min(e[1] for e in ves) >= 1e-3


def test_cube_volume_and_faces(anet_ctx):
    import allocnet_amd as aa
    h = pnp.dressed_cube()
    (v,), (act,), _ = aa.polytope_vertices([h], with_active=True, ctx=anet_ctx)
    assert abs(aa.polytope_volume(h, v, act) - 8.0) <= 8.0 * 1e-9
    assert abs(aa.polytope_volume(pnp.cube(), ctx=anet_ctx) - 8.0) <= 8.0 * 1e-9
    faces = aa.polytope_faces(h, v, act)
    assert sorted(faces) == list(range(8)) and all(len(f) == 4 for f in faces.values())
    for r, f in faces.items():
        assert np.cross(v[f[1]] - v[f[0]], v[f[2]] - v[f[1]]) @ h[r, :3] > 0.0


def test_statuses(anet_ctx):
    import allocnet_amd as aa
    vs, status = aa.polytope_vertices([EMPTY, FLAT, np.zeros((3, 4)), SLAB, SLAB[:1], pnp.cube()], ctx=anet_ctx)
    assert status.tolist() == [1, 1, 1, 1, 1, 0]
    assert [len(v) for v in vs] == [0, 0, 0, 0, 0, 8]
    assert aa.enumerate_vs(EMPTY, ctx=anet_ctx)[0] is False and aa.enumerate_vs(SLAB, ctx=anet_ctx)[0] is False


def test_max_vertices_is_a_hard_bound(anet_ctx):
    """max_vertices = 5 on the cube: status 2, count 8, five vertices, and the words behind verts[0][5] / active[0][5] untouched in
    the host caller's arrays."""
    h = np.ascontiguousarray(pnp.cube())
    verts = np.full(5 * 3 + 3, 777.0); act = np.full(5 * 2 + 2, 99, dtype=np.uint64)
    count = np.zeros(1, dtype=np.int32); status = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    anet_ctx.check(anet_ctx.lib.anet_polytope_vertices(anet_ctx.handle, 1, 6, p(h), 1e-6, 5, p(verts), p(count), p(act), p(status)))
    assert status[0] == 2 and count[0] == 8
    assert (verts[15:] == 777.0).all() and (act[10:] == 99).all()
    ve = _solid("cube")[2]
    assert np.abs(verts[:15].reshape(5, 3) - ve[:5]).max() <= 1e-8


@pytest.mark.parametrize("wpp", ["1", "4"])
def test_kernel_never_writes_past_max_vertices(anet_ctx, monkeypatch, wpp):
    """The device entry point on sentinel-filled device arrays, three polytopes with more vertices than max_vertices = 5 (cube 8,
    octahedron 6, cube 8): behind slot 5 of the last one the sentinel stands, and every polytope's five slots hold ITS first five
    vertices and masks -- an overrun of polytope b would land in the slots of b + 1 or in the tail."""
    import torch
    monkeypatch.setenv("ANET_POLYTOPE_VERTICES_WPP", wpp)
    names = ["cube", "octahedron", "cube"]
    hp = np.zeros((3, 8, 4))
    for b, n in enumerate(names):
        h = _solid(n)[0]
        hp[b, :len(h)] = h
    B, mv, tail = 3, 5, 64
    d_hp = torch.from_numpy(hp).cuda()
    verts = torch.full((B * mv * 3 + tail,), 777.0, device="cuda", dtype=torch.float64)
    act = torch.full((B * mv * 2 + tail,), 99, device="cuda", dtype=torch.int64)
    count = torch.zeros(B, device="cuda", dtype=torch.int32); status = torch.zeros(B, device="cuda", dtype=torch.int32)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    anet_ctx.check(anet_ctx.lib.anet_polytope_vertices_dev(anet_ctx.handle, B, 8, q(d_hp), 1e-6, mv, q(verts), q(count), q(act),
                                                           q(status), st))
    torch.cuda.synchronize()
    assert count.tolist() == [8, 6, 8] and status.tolist() == [2, 2, 2]
    v, a = verts.cpu().numpy(), act.cpu().numpy()
    assert (v[B * mv * 3:] == 777.0).all() and (a[B * mv * 2:] == 99).all()
    v, a = v[:B * mv * 3].reshape(B, mv, 3), a[:B * mv * 2].reshape(B, mv, 2).view(np.uint64)
    for b, n in enumerate(names):
        h, vq, ve, _ = _solid(n)
        assert np.abs(v[b] - ve[:mv]).max() <= 1e-8, (b, n)                       # the numpy enumeration's first five, in order
        assert np.array_equal(a[b], pnp.active_rows(h, ve[:mv])), (b, n)


def test_more_vertices_than_two_rows_minus_four(anet_ctx):
    """A pyramid whose four sides miss a common apex by 2.2e-6 has 8 vertices by the stated rule, from 5 rows: the facade's first
    call (max_vertices = 2 * 5 - 4 = 6) reports status 2 and count 8, its second pass returns all eight, in the numpy
    enumeration's order; with max_vertices given there is no second pass."""
    import allocnet_amd as aa
    h = pnp.split_apex_pyramid()
    ve, min_det = pnp.enumerate_triples(h)
    assert len(ve) == 8 and min_det >= 1e-3
    (v,), (act,), status = aa.polytope_vertices([h], with_active=True, ctx=anet_ctx)
    assert status[0] == 0 and v.shape == (8, 3)
    assert np.abs(v - ve).max() <= 1e-8
    assert np.array_equal(act, pnp.active_rows(h, ve))
    (v6,), status = aa.polytope_vertices([h], max_vertices=6, ctx=anet_ctx)
    assert status[0] == 2 and np.array_equal(v6, v[:6])
    ok, v1 = aa.enumerate_vs(h, ctx=anet_ctx)
    assert ok and np.array_equal(v1, v)


def test_default_dispatch_of_a_large_batch(anet_ctx, monkeypatch):
    """1152 polytopes of 16 rows take the one-wave-per-polytope shape by the library's own threshold (no override): the same bits
    as each polytope run alone (which takes the four-wave shape)."""
    import allocnet_amd as aa
    monkeypatch.delenv("ANET_POLYTOPE_VERTICES_WPP", raising=False)
    hp = _corridors()[0]
    alone = [aa.polytope_vertices(hp[b:b + 1], with_active=True, ctx=anet_ctx) for b in range(len(hp))]
    big = np.ascontiguousarray(np.tile(hp, (9, 1, 1))[np.random.default_rng(5).permutation(9 * len(hp))])
    pick = np.tile(np.arange(len(hp)), 9)[np.random.default_rng(5).permutation(9 * len(hp))]
    vs, acts, status = aa.polytope_vertices(big, with_active=True, ctx=anet_ctx)
    assert len(vs) == 1152 and (status == 0).all()
    for b, i in enumerate(pick):
        assert np.array_equal(vs[b], alone[i][0][0]) and np.array_equal(acts[b], alone[i][1][0]), (b, i)


def _pool():
    hp = _corridors()[0]
    return [SOLIDS[n][0]() for n in SOLIDS] + [EMPTY, FLAT, SLAB, np.zeros((2, 4))] + [hp[i] for i in range(0, 128, 9)]


@pytest.mark.parametrize("wpp", [None, "1", "4"])
def test_batches_give_the_bits_of_single_runs(anet_ctx, monkeypatch, wpp):
    """Batches of 0, 1 and 257 polytopes (not a multiple of the four waves of a workgroup), the inputs above mixed and permuted:
    every result is the same bits as that polytope run alone, with one wave or four waves per polytope."""
    import allocnet_amd as aa
    pool = _pool()
    monkeypatch.delenv("ANET_POLYTOPE_VERTICES_WPP", raising=False)
    alone = [aa.polytope_vertices([h], with_active=True, ctx=anet_ctx) for h in pool]
    if wpp is not None:
        monkeypatch.setenv("ANET_POLYTOPE_VERTICES_WPP", wpp)
    vs, status = aa.polytope_vertices([], ctx=anet_ctx)
    assert vs == [] and status.shape == (0,)
    pick = np.random.default_rng(2).permutation(np.arange(257) % len(pool))
    for batch in (pick[:1], pick):
        vs, acts, status = aa.polytope_vertices([pool[i] for i in batch], with_active=True, ctx=anet_ctx)
        for b, i in enumerate(batch):
            assert status[b] == alone[i][2][0], (b, i)
            assert np.array_equal(vs[b], alone[i][0][0]), (b, i)
            assert np.array_equal(acts[b], alone[i][1][0]), (b, i)


def test_device_entry_point_matches_the_host_one(anet_ctx):
    import torch
    import allocnet_amd as aa
    hp = _corridors()[0]
    vs, acts, status = aa.polytope_vertices(hp, with_active=True, ctx=anet_ctx)
    out = aa.polytope_vertices_dev(torch.from_numpy(hp).cuda(), with_active=True, ctx=anet_ctx)
    torch.cuda.synchronize()
    cnt = out["count"].cpu().numpy()
    assert np.array_equal(out["status"].cpu().numpy(), status)
    for b in range(len(hp)):
        assert cnt[b] == len(vs[b])
        assert np.array_equal(out["verts"][b, :cnt[b]].cpu().numpy(), vs[b])
        assert np.array_equal(out["active"][b, :cnt[b]].cpu().numpy().view(np.uint64), acts[b])


def test_corridor_vertices(anet_ctx):
    import allocnet_amd as aa
    from allocnet_amd.synth import qp_corridor_problem
    hp = qp_corridor_problem(np.random.default_rng(4), 4, 16)[2].copy()
    hp[:, :, 3] *= -1.0                                                         # a.x <= b  ->  a.x - b <= 0
    vps, status = aa.corridor_vertices(hp, ctx=anet_ctx)
    assert len(vps) == 7 and (status == 0).all()
    for k, v in enumerate(vps):
        parents = [k // 2] if k % 2 == 0 else [k // 2, k // 2 + 1]
        assert len(v) >= 4
        for q in parents:
            n, d, _ = pnp.unit_rows(hp[q])
            assert (v @ n.T + d).max() <= 1e-6
        vq = pnp.vertices_qhull(np.vstack([hp[q] for q in parents]))
        assert len(v) == len(vq) and pnp.hausdorff(v, vq) <= 1e-8 * max(1.0, np.abs(vq).max())


def test_argument_errors(anet_ctx):
    from allocnet_amd import _lib
    lib, hnd = anet_ctx.lib, anet_ctx.handle
    h = np.ascontiguousarray(pnp.cube()); v = np.zeros((8, 3)); c = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for fn, tail in ((lib.anet_polytope_vertices, ()), (lib.anet_polytope_vertices_dev, (None,))):
        call = lambda batch, rows, hp, eps, mv, vv, cc: fn(hnd, batch, rows, hp, eps, mv, vv, cc, None, None, *tail)
        assert call(-1, 6, p(h), 1e-6, 8, p(v), p(c)) == _lib.ANET_ERR_INVALID
        assert call(1, 0, p(h), 1e-6, 8, p(v), p(c)) == _lib.ANET_ERR_INVALID
        assert call(1, 6, p(h), 1e-6, 0, p(v), p(c)) == _lib.ANET_ERR_INVALID
        for eps in (0.0, -1e-6, float("nan"), float("inf")):
            assert call(1, 6, p(h), eps, 8, p(v), p(c)) == _lib.ANET_ERR_INVALID
        assert call(1, 6, None, 1e-6, 8, p(v), p(c)) == _lib.ANET_ERR_INVALID
        assert call(1, 6, p(h), 1e-6, 8, None, p(c)) == _lib.ANET_ERR_INVALID
        assert call(1, 6, p(h), 1e-6, 8, p(v), None) == _lib.ANET_ERR_INVALID
        assert call(1, 129, p(h), 1e-6, 8, p(v), p(c)) == _lib.ANET_ERR_UNSUPPORTED
        assert call(0, 6, None, 1e-6, 8, None, None) == _lib.ANET_OK
    assert lib.anet_polytope_vertices(None, 1, 6, p(h), 1e-6, 8, p(v), p(c), None, None) == _lib.ANET_ERR_INVALID


def test_cpp_vertices_program(anet_ctx):
    """Both overloads, the std::vector one and filterVs on the cube, the cone and three corridor polytopes: the C++ facade's
    output (%.17g) is the Python facade's, bit for bit."""
    import allocnet_amd as aa
    hp = _corridors()[0]
    polys = [pnp.cube(), pnp.cone(), hp[0][np.any(hp[0] != 0.0, axis=1)], hp[50], hp[127], EMPTY, pnp.split_apex_pyramid()]
    src = os.path.join(ROOT, "tests", "cpp", "test_geo_vertices.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        exe, txt = os.path.join(td, "test_geo_vertices"), os.path.join(td, "polytopes.txt")
        with open(txt, "w") as f:
            for h in polys:
                f.write(f"{len(h)}\n" + "".join(" ".join("%.17g" % x for x in row) + "\n" for row in h))
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe, txt], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = json.loads(res.stdout)["polytopes"]
    assert len(got) == len(polys)
    vs, status = aa.polytope_vertices(polys, ctx=anet_ctx)
    for g, v, st in zip(got, vs, status):
        assert g["ok"] == g["ok_vector"] == g["interior"] == (st == 0)
        for key in ("two", "four", "vector", "filtered"):
            assert np.array_equal(np.array(g[key], dtype=np.float64).reshape(-1, 3), v), key
    assert [len(g["two"]) for g in got] == [8, 41, len(vs[2]), len(vs[3]), len(vs[4]), 0, 8]     # the last: vertices_of's second pass
