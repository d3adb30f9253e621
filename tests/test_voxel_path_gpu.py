"""GPU suite of the path search (sfc_gen::planPath on the device voxel map) against the numpy / scipy restatement
(tests/voxel_path_np.py): the field equals Dijkstra's exactly, paths / costs / statuses bit for bit, independent safety
checks, the edge cases, the launch-file forest map, the corridor after it, and the C++ header."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.voxel_np import VoxelMapNP
from tests.voxel_path_np import PathNP, EXACT, APPROXIMATE, INVALID_START, INF32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import allocnet_amd as aa
    return aa.default_context()


def _pair(ctx, size, origin, scale, vox):
    import allocnet_amd as aa
    import torch
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    vm.voxels_dev.copy_(torch.from_numpy(vox))
    ref = VoxelMapNP(size, origin, scale)
    ref.vox[:] = vox
    return vm, ref


def _free_points(rng, p, k):
    """k random positions in free voxels of the restatement's box"""
    ids = np.flatnonzero(p.free.reshape(-1))
    pick = rng.choice(ids, size=k, replace=False)
    out = []
    for i in pick:
        x, y, z = p.xyz(i)
        out.append((np.array([x, y, z]) + rng.uniform(0.05, 0.95, 3)) * p.scale + np.array(p.o))
    return np.array(out)


def _maze(size):
    """walls every third x, each with a gap at alternating ends of y: the shortest path crosses the map many times"""
    sx, sy, sz = size
    v = np.zeros((sz, sy, sx), dtype=np.uint8)
    for k, x in enumerate(range(2, sx - 1, 3)):
        v[:, :, x] = 1
        if k % 2 == 0:
            v[:, sy - 3:, x] = 0
        else:
            v[:, :3, x] = 0
    return v.reshape(-1)


def _scene(name, ctx):
    from allocnet_amd.synth import forest_cloud
    rng = np.random.default_rng(sum(map(ord, name)))
    lb = hb = None
    if name == "odd_random25":
        size, origin, scale = (37, 29, 11), (-1.3, 0.7, -0.25), 0.1
        vox = (rng.uniform(size=int(np.prod(size))) < 0.25).astype(np.uint8)
        vm, ref = _pair(ctx, size, origin, scale, vox)
    elif name == "odd_dilated":
        size, origin, scale = (130, 70, 9), (2.0, -3.0, 0.5), 0.05
        vox = (rng.uniform(size=int(np.prod(size))) < 0.02).astype(np.uint8)
        vm, ref = _pair(ctx, size, origin, scale, vox)
        vm.dilate(1); ref.dilate(1)
    elif name == "maze":
        size, origin, scale = (96, 128, 2), (0.0, 0.0, 0.0), 0.1
        vm, ref = _pair(ctx, size, origin, scale, _maze(size))
    elif name == "sub_box":
        size, origin, scale = (50, 40, 12), (-2.5, -2.0, 0.0), 0.1
        vox = (rng.uniform(size=int(np.prod(size))) < 0.05).astype(np.uint8)
        vm, ref = _pair(ctx, size, origin, scale, vox)
        lb, hb = np.array([-1.93, -1.5, 0.21]), np.array([1.77, 1.25, 0.95])
    elif name == "forest":
        size, origin, scale = (200, 200, 25), (-20.0, -20.0, 0.0), 0.2
        rec = forest_cloud(np.random.default_rng(5), n_points=200_000)
        vm, ref = _pair(ctx, size, origin, scale, np.zeros(int(np.prod(size)), np.uint8))
        vm.setOccupiedCloud(rec.tobytes(), 16); ref.set_occupied_cloud(rec)
        vm.dilate(1); ref.dilate(1)
    p = PathNP(ref, lb, hb)
    if name == "maze":
        starts = np.array([[0.05, 0.05, 0.05], [4.0, 3.0, 0.15], [9.35, 0.05, 0.15]])
        goals = np.array([[9.55, 12.75, 0.15], [0.05, 12.75, 0.05], [0.15, 0.15, 0.15]])
    else:
        starts, goals = _free_points(rng, p, 3), _free_points(rng, p, 3)
    assert np.array_equal(vm.getVoxels(), ref.vox)
    return vm, p, starts, goals, lb, hb


SCENES = ["odd_random25", "odd_dilated", "maze", "sub_box", "forest"]


@pytest.fixture(scope="module")
def scenes(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            vm, p, starts, goals, lb, hb = _scene(name, ctx)
            fields = p.fields(starts)
            cache[name] = (vm, p, starts, goals, lb, hb, fields)
        return cache[name]
    return get


def _check_safe(vm, path, scale):
    for a, b in zip(path[:-1], path[1:]):
        n = max(2, int(math.ceil(np.linalg.norm(b - a) / (scale / 8.0))) + 1)
        q = a + np.linspace(0.0, 1.0, n)[:, None] * (b - a)
        assert not vm.query(q).any(), (a, b)


@pytest.mark.parametrize("name", SCENES)
def test_field_equals_dijkstra(scenes, name):
    vm, p, starts, goals, lb, hb, fields = scenes(name)
    f, rounds = vm.path_field_dev(starts, lb, hb)
    assert tuple(f.shape) == (3, p.n)
    got = f.cpu().numpy()
    assert np.array_equal(got, fields)
    assert rounds >= 1
    if name == "maze":
        assert rounds >= 100
    # B = 3 in one call equals three single calls
    for b in range(3):
        fb, _ = vm.path_field_dev(starts[b:b + 1], lb, hb)
        assert np.array_equal(fb.cpu().numpy()[0], fields[b])


@pytest.mark.parametrize("name", SCENES)
def test_paths_equal_the_restatement(scenes, name):
    import allocnet_amd as aa
    vm, p, starts, goals, lb, hb, fields = scenes(name)
    costs, paths, status = aa.plan_paths(starts, goals, vm, lb, hb)
    for b in range(3):
        c, path, st = p.plan(starts[b], goals[b], fields[b])
        assert status[b] == st
        assert paths[b].tobytes() == path.tobytes(), (b, paths[b], path)
        assert costs[b] == c
        # independent checks
        _check_safe(vm, paths[b], p.scale)
        assert paths[b][0].tobytes() == starts[b].tobytes()
        if st == EXACT:
            assert paths[b][-1].tobytes() == goals[b].tobytes()
        seg = np.linalg.norm(np.diff(paths[b], axis=0), axis=1).sum()
        assert costs[b] == pytest.approx(seg, rel=1e-12, abs=1e-300)
        assert costs[b] >= np.linalg.norm(paths[b][-1] - starts[b]) * (1 - 1e-12)
        tgt = p.free_voxel(paths[b][-1]) if st == EXACT else None
        dt = fields[b][tgt] if tgt is not None else fields[b][p.target(fields[b], starts[b], goals[b])[1]]
        assert costs[b] <= 1.02 * float(dt) * p.scale / 10.0 + 2.0 * math.sqrt(3.0) * p.scale


def test_edge_cases(ctx):
    import allocnet_amd as aa
    size, origin, scale = (20, 16, 6), (0.0, 0.0, 0.0), 0.5
    ref = VoxelMapNP(size, origin, scale)
    v = ref.vox.reshape(6, 16, 20)
    v[:, :, 6] = 1                     # a full wall: x in [3, 3.5) is occupied
    v[1:5, 5:11, 12:18] = 1            # a sealed room: shell of a box, hollow inside
    v[2:4, 6:10, 13:17] = 0
    vm, _ = _pair(ctx, size, origin, scale, ref.vox.copy())
    p = PathNP(ref)
    cases = [
        ([1.2, 1.3, 1.4], [1.2, 1.3, 1.4]),          # s == g
        ([1.1, 1.3, 1.4], [1.4, 1.2, 1.1]),          # one voxel
        ([3.2, 1.0, 1.0], [1.0, 1.0, 1.0]),          # start occupied
        ([-5.0, 1.0, 1.0], [1.0, 1.0, 1.0]),         # start outside the map
        ([8.0, 1.0, 1.0], [3.2, 1.0, 1.0]),          # goal occupied
        ([8.0, 1.0, 1.0], [30.0, 1.0, 1.0]),         # goal outside the map
        ([8.0, 1.0, 1.0], [7.2, 3.7, 1.6]),          # goal in the sealed room
        ([1.0, 1.0, 1.0], [8.0, 1.0, 1.0]),          # behind the full wall
    ]
    want_status = [EXACT, EXACT, INVALID_START, INVALID_START, APPROXIMATE, APPROXIMATE, APPROXIMATE, APPROXIMATE]
    for (s, g), ws in zip(cases, want_status):
        s, g = np.array(s), np.array(g)
        cost, path = aa.plan_path(s, g, None, None, vm)
        c, rp, st = p.plan(s, g)
        assert st == ws, (s, g)
        if st == INVALID_START:
            assert math.isinf(cost) and path.shape == (0, 3)
            continue
        assert path.tobytes() == rp.tobytes() and cost == c
        _check_safe(vm, path, scale)
        if st == EXACT:
            assert path[0].tobytes() == s.tobytes() and path[-1].tobytes() == g.tobytes()
    cost, path = aa.plan_path([1.2, 1.3, 1.4], [1.2, 1.3, 1.4], None, None, vm)
    assert cost == 0.0 and len(path) == 2


def test_runs_are_bitwise_identical(scenes):
    import allocnet_amd as aa
    vm, p, starts, goals, lb, hb, fields = scenes("forest")
    a = aa.plan_paths(starts, goals, vm, lb, hb)
    b = aa.plan_paths(starts, goals, vm, lb, hb)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


@pytest.fixture(scope="module")
def launch_map(ctx):
    import allocnet_amd as aa
    from allocnet_amd.synth import forest_cloud, forest_route
    route = forest_route()
    rec = forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=route)
    vm = aa.VoxelMap((400, 400, 50), (-20.0, -20.0, 0.0), 0.1, ctx=ctx)
    vm.setOccupiedCloud(rec.tobytes(), 16)
    vm.dilate(2)
    return vm, route


def test_launch_file_forest_map(launch_map):
    import allocnet_amd as aa
    vm, route = launch_map
    costs, paths, status, rounds = aa.plan_paths(route[:1], route[-1:], vm, with_rounds=True)
    assert status[0] == EXACT and rounds >= 1
    path = paths[0]
    assert path[0].tobytes() == route[0].tobytes() and path[-1].tobytes() == route[-1].tobytes()
    _check_safe(vm, path, 0.1)
    length = np.linalg.norm(np.diff(route, axis=0), axis=1).sum()
    assert costs[0] <= 1.15 * length + 1.0
    assert costs[0] >= np.linalg.norm(route[-1] - route[0])


def test_plan_then_corridor(launch_map):
    import allocnet_amd as aa
    vm, route = launch_map
    cost, path = aa.plan_path(route[0], route[-1], vm.getOrigin(), vm.getCorner(), vm)
    polys = aa.short_cut(aa.convex_cover(path, vm, vm.getOrigin(), vm.getCorner(), 7.0, 3.0))
    assert len(polys) >= 1
    for q in path:
        inside = [np.max(h[:, :3] @ q + h[:, 3]) <= 1e-9 for h in polys]
        assert any(inside), q


def test_cpp_plan_path_program(ctx):
    import allocnet_amd as aa
    src = os.path.join(ROOT, "tests", "cpp", "test_voxel_path.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "test_voxel_path")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe, td], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
        vox = np.fromfile(os.path.join(td, "voxels.bin"), dtype=np.uint8)
        got = np.fromfile(os.path.join(td, "path.bin"), dtype=np.float64)
    size, origin, scale = (60, 50, 12), (-3.0, -2.5, 0.0), 0.1
    vm, ref = _pair(ctx, size, origin, scale, vox)
    cost, path = aa.plan_path([-2.73, -2.21, 0.55], [2.61, 2.07, 0.43], vm.getOrigin(), vm.getCorner(), vm)
    assert got[:-1].tobytes() == path.reshape(-1).tobytes()
    assert got[-1] == cost
    c, rp, st = PathNP(ref).plan(np.array([-2.73, -2.21, 0.55]), np.array([2.61, 2.07, 0.43]))
    assert st == EXACT and rp.tobytes() == path.tobytes() and c == cost
