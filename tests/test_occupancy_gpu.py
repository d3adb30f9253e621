"""GPU suite of the device occupancy grid against the numpy restatement (tests/occupancy_np.py, pinned by test_occupancy_cpu.py):
scans in every record format, sequences with revision and reset, order-independence, both forms of the marks, the hand-over to
VoxelMap, depth unprojection, the first-hit ray query, the refusals, and the C++ header.  Every comparison is exact."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import occupancy_np as onp
from tests.voxel_np import VoxelMapNP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GRIDS = [((1, 1, 1), (0.0, 0.0, 0.0), 0.1), ((37, 23, 11), (-1.3, 0.7, -0.25), 0.1), ((64, 64, 8), (2.0, -3.0, 0.0), 0.05)]
N_RECORDS = [3000, 3000, 4000]


@pytest.fixture(scope="module")
def ctx():
    import allocnet_amd as aa
    return aa.default_context()


def _params(gi, **kw):
    """(device struct, restatement's) -- ranges that cut into the map: max_range about half its longest side."""
    import allocnet_amd as aa
    size, _, scale = GRIDS[gi]
    ext = max(size) * scale
    d = dict(hit=847, miss=-405, lo=-1100, hi=2000, min_range=0.05 * ext, max_range=0.55 * ext)
    d.update(kw)
    prm = aa.occupancy_params()
    for k, v in d.items():
        setattr(prm, k, v)
    return prm, onp.Params(**d)


def _centre(gi, cell):
    _, origin, scale = GRIDS[gi]
    return np.asarray(origin) + (np.asarray(cell, dtype=np.float64) + 0.5) * scale


def _sensors(gi):
    """A sensor at a cell centre inside the map (ties with centre end points), one outside it whose rays enter, one off-centre."""
    size, origin, scale = GRIDS[gi]
    size = np.asarray(size); ext = size * scale
    inside = _centre(gi, size // 3)
    outside = np.asarray(origin) + np.array([-0.15, 0.4, 0.6]) * ext
    off = np.asarray(origin) + np.array([0.71, 0.52, 0.33]) * ext
    return [inside, outside, off]


def _scan(rng, gi, sensor, n):
    """(n, 3) float64 end points from `sensor`: random inside and up to 20 % outside, axis-parallel, centre-to-centre diagonals,
    on cell faces and map faces, beyond max_range and below min_range (the ranges of _params cut into the map), NaN and +-inf."""
    size, origin, scale = GRIDS[gi]
    size = np.asarray(size); o = np.asarray(origin); ext = size * scale
    p = o + rng.uniform(-0.2, 1.2, (n, 3)) * ext
    k = n // 10
    ax = rng.integers(0, 3, k)                                           # axis-parallel
    p[:k] = sensor
    p[np.arange(k), ax] += rng.uniform(-0.6, 0.6, k) * ext.max()
    cell = np.floor((sensor - o) / scale)                                # diagonals from the sensor's cell centre (ties when it is one)
    d = rng.integers(-12, 13, (k, 1)) * rng.choice([-1, 1], (k, 3))
    p[k:2 * k] = o + (cell + d + 0.5) * scale
    p[2 * k:3 * k] = o + rng.integers(-2, size + 3, (k, 3)) * scale      # on cell corners
    f = 3 * k + np.arange(k)                                             # on one cell face / on the map's faces
    p[f, rng.integers(0, 3, k)] = (o + rng.integers(0, size + 1, (k, 3)) * scale)[np.arange(k), rng.integers(0, 3, k)]
    p[4 * k:4 * k + k // 2] = o + ext * rng.integers(0, 2, (k // 2, 3))
    p[5 * k:5 * k + k // 2] = sensor + rng.normal(0.0, 0.04, (k // 2, 3)) * ext.max()   # around min_range
    p[5 * k + k // 2:6 * k] = sensor                                     # zero length
    p[6 * k:6 * k + 5, 1] = np.nan
    p[6 * k + 5:6 * k + 9, 2] = np.inf
    p[6 * k + 9:6 * k + 12, 0] = -np.inf
    p[6 * k + 12] = [1e300, -1e300, 1e300]
    return p


def _feed(om, fmt, pts, sensor):
    """The records in one of the three formats -> (what the restatement reads)."""
    if fmt == "f64":
        om.integrate(pts, sensor)
        return pts
    floats = {"f32x16": 4, "f32x32": 8}[fmt]
    with np.errstate(over="ignore"):
        rec = np.full((len(pts), floats), 7.0, dtype=np.float32)
        rec[:, :3] = pts
    om.integrateCloud(rec.tobytes(), floats * 4, sensor)
    return rec


@pytest.mark.parametrize("fmt", ["f32x16", "f32x32", "f64"])
@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_scan_sequences(ctx, gi, fmt):
    """Three scans from three origins into one map, compared after each (marks cleared, clamps, revision), reset, and again; the
    third sensor sits in a cell the map holds as occupied."""
    import allocnet_amd as aa
    size, origin, scale = GRIDS[gi]
    rng = np.random.default_rng(100 * gi + len(fmt))
    prm, ref_prm = _params(gi)
    om = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
    L = np.full(int(np.prod(size)), onp.UNKNOWN, dtype=np.int16)
    assert np.array_equal(om.getLogOdds(), L) and om.known_fraction() == 0.0
    sensors = _sensors(gi)
    for k in range(3):
        if k == 2 and (L > 0).any():
            v = int(np.flatnonzero(L > 0)[len(np.flatnonzero(L > 0)) // 2])
            sensors[2] = _centre(gi, (v % size[0], (v // size[0]) % size[1], v // (size[0] * size[1]))) + 0.013 * scale
        pts = _scan(rng, gi, sensors[k], N_RECORDS[gi])
        rec = _feed(om, fmt, pts, sensors[k])
        onp.integrate(L, size, origin, scale, ref_prm, sensors[k], rec)
        assert np.array_equal(om.getLogOdds(), L), (gi, fmt, k)
        assert not om._work.any(), "marks left behind"
    assert (L != onp.UNKNOWN).any() and abs(om.known_fraction() - (L != onp.UNKNOWN).mean()) < 1e-12
    if gi > 0:
        assert (L == ref_prm.lo).any() and (L > 0).any()
    om.reset()
    L[:] = onp.UNKNOWN
    assert np.array_equal(om.getLogOdds(), L)
    pts = _scan(rng, gi, sensors[0], N_RECORDS[gi])
    rec = _feed(om, fmt, pts, sensors[0])
    onp.integrate(L, size, origin, scale, ref_prm, sensors[0], rec)
    assert np.array_equal(om.getLogOdds(), L)


@pytest.mark.parametrize("gi", [1, 2])
def test_order_and_duplicates_change_nothing(ctx, gi):
    import allocnet_amd as aa
    size, origin, scale = GRIDS[gi]
    rng = np.random.default_rng(7 + gi)
    prm, ref_prm = _params(gi)
    sensor = _sensors(gi)[0]
    pts = _scan(rng, gi, sensor, N_RECORDS[gi])
    L = onp.integrate(np.full(int(np.prod(size)), onp.UNKNOWN, dtype=np.int16), size, origin, scale, ref_prm, sensor, pts)
    for variant in (pts, pts[rng.permutation(len(pts))], np.repeat(pts, 2, axis=0), np.concatenate([pts[::-1], pts])):
        om = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
        om.integrate(variant, sensor)
        assert np.array_equal(om.getLogOdds(), L)


@pytest.mark.parametrize("gi", [0, 1, 2])
def test_both_mark_forms_give_the_same_grid(ctx, gi):
    """ANET_OCC_MARKS_ATOMIC: one launch of atomicOr on flag bits instead of two launches of byte stores."""
    import allocnet_amd as aa
    size, origin, scale = GRIDS[gi]
    rng = np.random.default_rng(17 + gi)
    prm, ref_prm = _params(gi)
    L = np.full(int(np.prod(size)), onp.UNKNOWN, dtype=np.int16)
    om = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
    assert "ANET_OCC_MARKS_ATOMIC" not in os.environ
    os.environ["ANET_OCC_MARKS_ATOMIC"] = "1"
    try:
        for sensor in _sensors(gi)[:2]:
            pts = _scan(rng, gi, sensor, N_RECORDS[gi])
            om.integrate(pts, sensor)
            onp.integrate(L, size, origin, scale, ref_prm, sensor, pts)
            assert np.array_equal(om.getLogOdds(), L)
            assert not om._work.any()
    finally:
        del os.environ["ANET_OCC_MARKS_ATOMIC"]


@pytest.mark.parametrize("gi", [1, 2])
def test_hand_over_to_voxel_map(ctx, gi):
    import allocnet_amd as aa
    size, origin, scale = GRIDS[gi]
    rng = np.random.default_rng(27 + gi)
    prm, ref_prm = _params(gi)
    om = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
    L = np.full(int(np.prod(size)), onp.UNKNOWN, dtype=np.int16)
    for sensor in _sensors(gi):
        pts = _scan(rng, gi, sensor, N_RECORDS[gi])
        om.integrate(pts, sensor)
        onp.integrate(L, size, origin, scale, ref_prm, sensor, pts)
    reuse = aa.VoxelMap(size, origin, scale, ctx=ctx)
    reuse.setOccupied(np.asarray(origin) + 0.5 * scale)               # overwritten: every byte is written
    for unknown in ("blocked", "free"):
        for occ in (0, 900):
            want = onp.to_voxels(L, occ, unknown == "blocked")
            vm = om.to_voxel_map(occ=occ, unknown=unknown)
            assert np.array_equal(vm.getVoxels(), want)
            assert om.to_voxel_map(occ=occ, unknown=unknown, out=reuse) is reuse
            assert np.array_equal(reuse.getVoxels(), want)
            ref = VoxelMapNP(size, origin, scale)
            ref.vox[:] = want
            vm.dilate(1); ref.dilate(1)
            assert np.array_equal(vm.getVoxels(), ref.vox)
            assert np.array_equal(vm.getSurfIds(), ref.surf)
            vd = om.to_voxel_map(occ=occ, unknown=unknown, dilate=1)
            assert np.array_equal(vd.getVoxels(), ref.vox) and np.array_equal(vd.getSurfIds(), ref.surf)
    assert 0 < onp.to_voxels(L, 0, False).sum() < onp.to_voxels(L, 0, True).sum() < L.size


def _rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("kind", ["float32", "uint16"])
@pytest.mark.parametrize("step", [1, 3])
def test_depth_unprojection(ctx, kind, step):
    import allocnet_amd as aa
    import torch
    gi = 1
    size, origin, scale = GRIDS[gi]
    rng = np.random.default_rng(40 + step + len(kind))
    H, W = 48, 64
    K = (61.3, 59.8, 31.7, 23.2)
    R = _rotation(rng)
    t = np.asarray(origin) + np.array([0.3, 0.5, 0.5]) * np.asarray(size) * scale
    if kind == "float32":
        depth = rng.uniform(0.2, 3.0, (H, W)).astype(np.float32)
        depth[rng.uniform(size=(H, W)) < 0.05] = 0.0
        depth[rng.uniform(size=(H, W)) < 0.05] = np.nan
        depth[0, 0] = np.inf
        ds, lo, hi = 1.0, 0.25, 2.5
    else:
        depth = rng.integers(200, 3000, (H, W)).astype(np.uint16)
        depth[rng.uniform(size=(H, W)) < 0.05] = 0
        depth[1, 1] = 65535
        ds, lo, hi = 0.001, 0.25, 2.5
    want = onp.depth_to_points(depth, K, R, t, step, ds, lo, hi)
    assert np.isnan(want).any() and np.isfinite(want).any()
    dev = torch.from_numpy(depth.view(np.int16) if kind == "uint16" else depth).to(torch.device("cuda", ctx.device))
    got = aa.depth_to_points_dev(dev, K, (R, t), step, ds, lo, hi, ctx=ctx).cpu().numpy()
    assert got.shape == want.shape == (((W + step - 1) // step) * ((H + step - 1) // step), 3)
    assert got.tobytes() == want.tobytes()
    # the 3 x 3 / 4 x 4 matrix forms of the same camera
    K3 = np.array([[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]])
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = t
    assert aa.depth_to_points_dev(dev, K3, M, step, ds, lo, hi, ctx=ctx).cpu().numpy().tobytes() == want.tobytes()
    # integrateDepth is the unprojection followed by integrate, from the camera centre
    prm, ref_prm = _params(gi)
    a = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
    b = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
    pts = a.integrateDepth(depth, K, (R, t), step, ds, lo, hi)
    assert pts.cpu().numpy().tobytes() == want.tobytes()
    b.integrate(want, t)
    L = onp.integrate(np.full(int(np.prod(size)), onp.UNKNOWN, dtype=np.int16), size, origin, scale, ref_prm, t, want)
    assert np.array_equal(a.getLogOdds(), L) and np.array_equal(b.getLogOdds(), L)
    assert (L != onp.UNKNOWN).sum() > 100


def test_first_hit_ray_query(ctx):
    import allocnet_amd as aa
    import torch
    size, origin, scale = GRIDS[1]
    rng = np.random.default_rng(55)
    og = np.asarray(origin); ext = np.asarray(size) * scale
    vox = (rng.uniform(size=int(np.prod(size))) < 0.05).astype(np.uint8)
    vox[rng.integers(0, vox.size, 40)] = 2                              # dilated bytes block as well
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    vm.voxels_dev.copy_(torch.from_numpy(vox))
    n = 2000
    o = og + rng.uniform(-0.2, 1.2, (n, 3)) * ext
    q = og + rng.uniform(-0.2, 1.2, (n, 3)) * ext
    blocked = np.flatnonzero(vox)
    for i in range(20):                                                   # start cell blocked
        v = int(blocked[i])
        o[i] = og + (np.array([v % size[0], (v // size[0]) % size[1], v // (size[0] * size[1])]) + rng.uniform(0.1, 0.9, 3)) * scale
    o[20:30] = og - rng.uniform(0.1, 0.5, (10, 3)) * ext                  # wholly outside
    q[20:30] = og - rng.uniform(0.1, 0.5, (10, 3)) * ext
    q[30:40] = o[30:40]                                                   # zero length
    c = (o[40:60] - og) / scale                                           # centre to centre: ties
    o[40:60] = og + (np.floor(c) + 0.5) * scale
    q[40:60] = o[40:60] + rng.integers(-9, 10, (20, 1)) * rng.choice([-1, 1], (20, 3)) * scale
    o[60], q[61], o[62], q[63] = [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e300, 0, 0]
    o[64] = [2.0 ** 30 * scale * 1.5, 0, 0]                               # a cell index of 2^30 or more
    o[65], q[65] = og, og + np.array([65537.5, 0.5, 0.5]) * scale         # a span of more than 65536 cells
    o[66], q[66] = og + np.array([-70000.5, 0.5, 0.5]) * scale, og + np.array([-69000.5, 0.5, 0.5]) * scale   # far, but walkable
    want_v, want_t = onp.raycast(vox, size, origin, scale, o, q)
    got_v, got_t = vm.raycast(o, q)
    assert got_v.dtype == np.int32 and np.array_equal(got_v, want_v)
    assert got_t.tobytes() == want_t.tobytes()
    assert (want_v[:20] == blocked[:20]).all() and (want_t[:20] == 0.0).all()
    assert (want_v[20:30] == onp.HIT_FREE).all() and (want_t[20:30] == 1.0).all()
    assert (want_v[60:66] == onp.HIT_INVALID).all() and np.isnan(want_t[60:66]).all() and want_v[66] == onp.HIT_FREE
    assert (want_v >= 0).sum() > 500 and (want_v == onp.HIT_FREE).sum() > 100
    # through an empty map without a hit, and the single-segment form
    empty = aa.VoxelMap(size, origin, scale, ctx=ctx)
    v, t = empty.raycast(og - 0.1 * ext, og + 1.1 * ext)
    assert (v, t) == (onp.HIT_FREE, 1.0)
    v, t = vm.raycast(o[0], q[0])
    assert v == want_v[0] and t == want_t[0]


def test_refusals_leave_the_grid_untouched(ctx):
    import allocnet_amd as aa
    from allocnet_amd import _lib
    gi = 1
    size, origin, scale = GRIDS[gi]
    rng = np.random.default_rng(66)
    prm, _ = _params(gi)
    om = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
    sensor = _sensors(gi)[0]
    pts = _scan(rng, gi, sensor, 500)
    om.integrate(pts, sensor)
    before = om.getLogOdds()
    assert (before != onp.UNKNOWN).any()
    bad = [dict(hit=0), dict(hit=-5), dict(miss=0), dict(miss=3), dict(lo=0), dict(lo=-32768), dict(lo=5), dict(hi=0), dict(hi=32768),
           dict(hi=-1), dict(min_range=-1e-9), dict(min_range=np.nan), dict(min_range=np.inf), dict(max_range=0.0),
           dict(max_range=-1.0), dict(max_range=np.inf), dict(max_range=np.nan), dict(max_range=65536.5 * scale)]
    for kw in bad:
        om.params = _params(gi, **kw)[0]
        with pytest.raises(aa.AnetError) as ei:
            om.integrate(pts, sensor)
        assert ei.value.code == _lib.ANET_ERR_INVALID, kw
    om.params = prm
    for o in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [2.0 ** 30 * scale * 1.2, 0, 0], [0, -2.0 ** 30 * scale * 1.2, 0]):
        with pytest.raises(aa.AnetError) as ei:
            om.integrate(pts, o)
        assert ei.value.code == _lib.ANET_ERR_INVALID, o
    # a bad grid, a bad stride, a negative count: through the C entry point
    import torch
    t = torch.from_numpy(pts).to(om.device)
    st = ctypes.c_void_p(torch.cuda.current_stream(om.device).cuda_stream)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    so = np.ascontiguousarray(sensor)

    def call(grid, n, stride, f64):
        return ctx.lib.anet_occupancy_integrate_dev(ctx.handle, ctypes.byref(grid), ctypes.byref(prm), vp(om._logodds),
                                                    so.ctypes.data_as(ctypes.c_void_p), vp(t), n, stride, f64, vp(om._work), st)
    g = _lib.VoxelGrid.from_buffer_copy(om._grid)
    g.scale = 0.0
    assert call(g, len(pts), 24, 1) == _lib.ANET_ERR_INVALID
    g = _lib.VoxelGrid.from_buffer_copy(om._grid)
    g.size[1] = 0
    assert call(g, len(pts), 24, 1) == _lib.ANET_ERR_INVALID
    assert call(om._grid, -1, 24, 1) == _lib.ANET_ERR_INVALID
    assert call(om._grid, len(pts), 20, 1) == _lib.ANET_ERR_INVALID
    assert call(om._grid, len(pts), 8, 0) == _lib.ANET_ERR_INVALID
    assert call(om._grid, len(pts), 24, 2) == _lib.ANET_ERR_INVALID
    assert ctx.lib.anet_occupancy_workspace(ctypes.byref(g)) == -1
    assert np.array_equal(om.getLogOdds(), before) and not om._work.any()
    # the largest range that is allowed is allowed
    om.params = _params(gi, max_range=65536.0 * scale)[0]
    om.integrate(pts[:10], sensor)


def test_cpp_occupancy_program(ctx):
    import allocnet_amd as aa
    src = os.path.join(ROOT, "tests", "cpp", "test_occupancy.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "test_occupancy")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe, td], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
        rd = lambda f, dt: np.fromfile(os.path.join(td, f), dtype=dt)  # noqa: E731
        size, origin, scale = (60, 50, 12), (-3.0, -2.5, 0.0), 0.1
        sensor = np.array([-2.2, -1.9, 0.55])
        prm = aa.occupancy_params(0.7, 0.4, 0.12, 0.97, 0.2, 4.0)
        ref_prm = onp.Params(prm.hit, prm.miss, prm.lo, prm.hi, 0.2, 4.0)
        cloud = rd("cloud.bin", np.float32).reshape(-1, 4)
        om = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
        om.integrateCloud(cloud.tobytes(), 16, sensor)
        L = rd("logodds.bin", np.int16)
        assert np.array_equal(L, om.getLogOdds())
        assert np.array_equal(L, onp.integrate(np.full(L.size, onp.UNKNOWN, dtype=np.int16), size, origin, scale, ref_prm, sensor, cloud))
        assert (L > 0).sum() > 100 and (L == onp.UNKNOWN).sum() > 100
        R = rd("rotation.bin", np.float64).reshape(3, 3)
        od = aa.OccupancyMap(size, origin, scale, prm, ctx=ctx)
        od.integrateDepth(rd("depth.bin", np.float32).reshape(30, 40), (30.0, 30.0, 19.5, 14.5), (R, sensor), 1, 1.0, 0.1, 8.0)
        LD = rd("logodds_depth.bin", np.int16)
        assert np.array_equal(LD, od.getLogOdds()) and (LD > 0).sum() > 50
        vm = om.to_voxel_map(occ=0, unknown="free", dilate=1)
        assert np.array_equal(rd("voxels.bin", np.uint8), vm.getVoxels())
        v, t = vm.raycast(sensor, np.array([2.9, -1.9, 0.55]))
        ray = rd("ray.bin", np.float64)
        assert ray[0] == v and ray[1:].tobytes() == np.float64(t).tobytes()
