"""GPU suite of the device voxel map against the numpy restatement (tests/voxel_np.py): fill, dilation, surface, query,
the box gather of convexCover, convex_cover with the map, and the C++ header driven like the ROS node."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.voxel_np import VoxelMapNP, box_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GRIDS = [((1, 1, 1), (0.0, 0.0, 0.0), 0.1), ((37, 23, 11), (-1.3, 0.7, -0.25), 0.1), ((64, 64, 8), (2.0, -3.0, 0.0), 0.05),
         ((400, 400, 50), (-20.0, -20.0, 0.0), 0.1)]


@pytest.fixture(scope="module")
def ctx():
    import allocnet_amd as aa
    return aa.default_context()


def _cloud(rng, size, origin, scale, n, step_floats):
    """float32 records: inside, below the origin, on the upper faces, outside, NaN and inf."""
    o = np.asarray(origin); ext = np.asarray(size) * scale
    p = o + rng.uniform(-0.1, 1.1, (n, 3)) * ext
    k = n // 10
    p[:k] = o - rng.uniform(0.0, 1.5, (k, 3)) * scale               # up to 1.5 voxels below the origin
    p[k:2 * k] = o + ext * rng.integers(0, 2, (k, 3))                # corners and upper faces
    rec = np.zeros((n, step_floats), dtype=np.float32)
    rec[:, :3] = p
    rec[2 * k:2 * k + 5, 1] = np.nan
    rec[2 * k + 5:2 * k + 9, 2] = np.inf
    rec[2 * k + 9:2 * k + 12, 0] = -np.inf
    return rec


def _check_surface(vm, ref):
    assert np.array_equal(vm.getVoxels(), ref.vox)
    ids = vm.getSurfIds()
    assert np.array_equal(ids, ref.surf)
    assert np.all(np.diff(ids) > 0)
    got = vm.getSurf()
    assert got.tobytes() == ref.surf_points().tobytes()


@pytest.mark.parametrize("gi", range(len(GRIDS)))
@pytest.mark.parametrize("step_floats", [4, 8])
def test_fill_cloud(ctx, gi, step_floats):
    import allocnet_amd as aa
    size, origin, scale = GRIDS[gi]
    rng = np.random.default_rng(gi * 10 + step_floats)
    n = 200_000 if np.prod(size) > 10 ** 6 else 3000
    rec = _cloud(rng, size, origin, scale, n, step_floats)
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    ref = VoxelMapNP(size, origin, scale)
    vm.setOccupiedCloud(rec.tobytes(), step_floats * 4)
    ref.set_occupied_cloud(rec)
    assert np.array_equal(vm.getVoxels(), ref.vox)
    # float64 rows through setOccupied (also non-finite rows: skipped)
    p64 = _cloud(rng, size, origin, scale, 1000, 3).astype(np.float64)
    p64[:, :3] += rng.normal(0.0, 1e-9, (1000, 3))
    vm.setOccupied(p64)
    ref.set_occupied_cloud(p64)
    assert np.array_equal(vm.getVoxels(), ref.vox)


def test_fill_edges(ctx):
    import allocnet_amd as aa
    o = np.array([1.0, -2.0, 0.25]); s = 0.1
    vm = aa.VoxelMap((4, 5, 6), o, s, ctx=ctx)
    ref = VoxelMapNP((4, 5, 6), o, s)
    pts = np.array([o - 0.5 * s, o - 1.5 * s, o + np.array([4, 5, 6]) * s, o + np.array([4, 5, 6]) * s - 1e-12,
                    o + np.array([3.999, 0.0, 0.0]) * s, [1e300, 0, 0], [-1e300, 0, 0]])
    vm.setOccupied(pts); ref.set_occupied(pts)
    assert np.array_equal(vm.getVoxels(), ref.vox)
    assert vm.getVoxels()[0] == 1


def test_fill_index_triples(ctx):
    """setOccupied with integer rows: the reference's setOccupied(Eigen::Vector3i), bounds per axis."""
    import allocnet_amd as aa
    import torch
    size, origin, scale = GRIDS[1]
    rng = np.random.default_rng(4)
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    ref = VoxelMapNP(size, origin, scale)
    ids = rng.integers(-3, np.asarray(size) + 3, (4000, 3))
    ids[:3] = [[2 ** 31 + 5, 0, 0], [-2 ** 40, 1, 1], [0, 0, 0]]
    vm.setOccupied(ids); ref.set_occupied_id(ids)
    assert np.array_equal(vm.getVoxels(), ref.vox)
    vm.setOccupied(torch.tensor([[36, 22, 10]], dtype=torch.int32, device=vm.device)); ref.set_occupied_id([[36, 22, 10]])
    assert np.array_equal(vm.getVoxels(), ref.vox)


def test_surface_capacity_below_the_count(ctx):
    """anet_voxel_surface_dev with cap < count: exactly the first cap ascending ids, the rest untouched, the true count."""
    import allocnet_amd as aa
    import torch
    size, origin, scale = GRIDS[2]
    rng = np.random.default_rng(6)
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    ref = VoxelMapNP(size, origin, scale)
    p = np.asarray(origin) + rng.uniform(0.0, 1.0, (300, 3)) * np.asarray(size) * scale
    vm.setOccupied(p); ref.set_occupied(p)
    vm.dilate(2); ref.dilate(2)
    n = len(ref.surf)
    assert n > 5000
    for cap in (0, 1, 4095, 4097, n - 1):
        ids = torch.full((n + 8,), -7, dtype=torch.int32, device=vm.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=vm.device)
        ctx.check(ctx.lib.anet_voxel_surface_dev(ctx.handle, ctypes.byref(vm._grid), ctypes.c_void_p(vm._work.data_ptr()), cap,
                                                 ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(cnt.data_ptr()),
                                                 ctypes.c_void_p(torch.cuda.current_stream(vm.device).cuda_stream)))
        got = ids.cpu().numpy()
        assert int(cnt.item()) == n
        assert np.array_equal(got[:cap], ref.surf[:cap])
        assert (got[cap:] == -7).all()


def _random_map(rng, size, density):
    m = (rng.uniform(size=int(np.prod(size))) < density).astype(np.uint8)
    return m


@pytest.mark.parametrize("gi", [1, 2, 3])
@pytest.mark.parametrize("kind", ["empty", "full", "random"])
def test_dilate_sequences(ctx, gi, kind):
    import allocnet_amd as aa
    import torch
    size, origin, scale = GRIDS[gi]
    rng = np.random.default_rng(gi * 3 + len(kind))
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    ref = VoxelMapNP(size, origin, scale)
    big = gi == 3
    init = {"empty": np.zeros(ref.vox.size, np.uint8), "full": np.ones(ref.vox.size, np.uint8),
            "random": _random_map(rng, size, 2e-4 if big else 0.01)}[kind]
    vm.voxels_dev.copy_(torch.from_numpy(init))
    ref.vox[:] = init
    rs = [2, 0, 1] if big else [1, 0, 2, 3, 5, max(size) + 3]
    for r in rs:
        vm.dilate(r); ref.dilate(r)
        _check_surface(vm, ref)
        c = rng.integers(0, size)
        assert vm.getSurfInBox(c, 3).tobytes() == ref.surf_in_box(c, 3).tobytes()
        # setOccupied between calls overwrites 2 with 1 and leaves the surface as it is
        p = np.asarray(origin) + rng.uniform(0.0, 1.0, (5, 3)) * np.asarray(size) * scale
        vm.setOccupied(p); ref.set_occupied(p)
        assert np.array_equal(vm.getVoxels(), ref.vox)
        assert np.array_equal(vm.getSurfIds(), ref.surf)


def test_query(ctx):
    import allocnet_amd as aa
    size, origin, scale = GRIDS[1]
    rng = np.random.default_rng(5)
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    ref = VoxelMapNP(size, origin, scale)
    p = np.asarray(origin) + rng.uniform(0.0, 1.0, (200, 3)) * np.asarray(size) * scale
    vm.setOccupied(p); ref.set_occupied(p)
    vm.dilate(1); ref.dilate(1)
    q = np.asarray(origin) + rng.uniform(-0.2, 1.2, (5000, 3)) * np.asarray(size) * scale
    q[:10] = np.asarray(origin) - 0.5 * scale
    q[10, 0] = np.nan
    assert np.array_equal(vm.query(q), ref.query(q))
    assert vm.query(q[0]) == bool(ref.query(q[:1])[0])
    assert vm.query(np.asarray(origin) - 5.0) is True


def test_runs_are_bitwise_identical(ctx):
    import allocnet_amd as aa
    from allocnet_amd.synth import forest_cloud
    size, origin, scale = GRIDS[3]
    rec = forest_cloud(np.random.default_rng(1), n_points=300_000)
    outs = []
    for _ in range(2):
        vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
        vm.setOccupiedCloud(rec.tobytes(), 16)
        vm.dilate(2)
        outs.append((vm.getVoxels().tobytes(), vm.getSurfIds().tobytes(), vm.getSurf().tobytes()))
    assert outs[0] == outs[1]
    ref = VoxelMapNP(size, origin, scale)
    ref.set_occupied_cloud(rec)
    ref.dilate(2)
    assert outs[0][0] == ref.vox.tobytes() and outs[0][2] == ref.surf_points().tobytes()


def _boxes(rng, K, lo, hi):
    bd = np.zeros((K, 6, 4))
    for k in range(K):
        a, b = rng.uniform(lo, hi, 3), rng.uniform(lo, hi, 3)
        l, h = np.minimum(a, b), np.maximum(a, b)
        for ax in range(3):
            bd[k, 2 * ax, ax] = 1.0; bd[k, 2 * ax, 3] = -h[ax]
            bd[k, 2 * ax + 1, ax] = -1.0; bd[k, 2 * ax + 1, 3] = l[ax]
    bd[0, 0, 3] = -(lo - 1.0)   # an empty box
    return bd


def test_gather_boxes(ctx):
    import torch
    from allocnet_amd import gather_boxes_dev
    rng = np.random.default_rng(9)
    pts = rng.uniform(-5.0, 5.0, (50_000, 3))
    pts[:1000] = np.round(pts[:1000], 1)             # exact ties with the box faces
    bd = _boxes(rng, 9, -5.0, 5.0)
    bd[1, :, 3] = np.round(bd[1, :, 3], 1)
    dev = torch.device("cuda", ctx.device)
    pc, counts = gather_boxes_dev(torch.from_numpy(bd).to(dev), torch.from_numpy(pts).to(dev), ctx=ctx)
    pc = pc.cpu().numpy()
    want = [box_filter(pts, bd[k]) for k in range(len(bd))]
    assert counts[0] == 0
    assert pc.shape[1] == max(1, max(len(w) for w in want))
    for k, w in enumerate(want):
        assert counts[k] == len(w)
        assert pc[k, :len(w)].tobytes() == w.tobytes()
        assert not pc[k, len(w):].any()
    # capacity overflow: min(count, cap) rows written, the true counts reported
    cap = 7
    work = torch.empty(int(ctx.lib.anet_voxel_gather_workspace(len(bd), len(pts))), dtype=torch.uint8, device=dev)
    out = torch.zeros((len(bd), cap, 3), dtype=torch.float64, device=dev)
    n_out = torch.zeros(len(bd), dtype=torch.int32, device=dev)
    bdt = torch.from_numpy(bd).to(dev); pt = torch.from_numpy(pts).to(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    ctx.check(ctx.lib.anet_voxel_gather_boxes_dev(ctx.handle, len(bd), vp(bdt), vp(pt), len(pts), cap, vp(work), vp(out),
                                                  vp(n_out), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    out = out.cpu().numpy()
    assert list(n_out.cpu().numpy()) == [len(w) for w in want]
    for k, w in enumerate(want):
        assert out[k, :min(cap, len(w))].tobytes() == w[:cap].tobytes()


def test_convex_cover_with_the_map_equals_the_points_path(ctx):
    import allocnet_amd as aa
    from allocnet_amd.synth import forest_cloud, forest_route
    size, origin, scale = GRIDS[3]
    route = forest_route()
    rec = forest_cloud(np.random.default_rng(3), n_points=300_000, clear_route=route)
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    vm.setOccupiedCloud(rec.tobytes(), 16)
    vm.dilate(2)
    lo, hi = vm.getOrigin(), vm.getCorner()
    hm = aa.convex_cover(route, vm, lo, hi, 7.0, 3.0, ctx=ctx)
    hp = aa.convex_cover(route, vm.getSurf(), lo, hi, 7.0, 3.0, ctx=ctx)
    assert len(hm) == len(hp) >= 5
    for a, b in zip(hm, hp):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


CPP_INDEX_FILLS = [[0, 0, 0], [59, 49, 11], [60, 0, 0], [-1, 3, 3], [10, 50, 2], [30, 20, 11]]   # as test_voxel_map.cpp


def test_cpp_voxel_map_program(ctx):
    src = os.path.join(ROOT, "tests", "cpp", "test_voxel_map.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "test_voxel_map")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe, td], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
        rd = lambda f, dt: np.fromfile(os.path.join(td, f), dtype=dt)  # noqa: E731
        ref = VoxelMapNP((60, 50, 12), (-3.0, -2.5, 0.0), 0.1)
        ref.set_occupied_cloud(rd("cloud.bin", np.float32).reshape(-1, 4))
        ref.set_occupied_id(CPP_INDEX_FILLS)
        ref.dilate(2)
        assert np.array_equal(rd("voxels.bin", np.uint8), ref.vox)
        assert rd("surf.bin", np.float64).tobytes() == ref.surf_points().tobytes()
        assert rd("inbox.bin", np.float64).tobytes() == ref.surf_in_box((40, 28, 3), 4).tobytes()
        q = rd("qpos.bin", np.float64).reshape(-1, 3)
        assert np.array_equal(rd("query.bin", np.uint8).astype(bool), ref.query(q))
