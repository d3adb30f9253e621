"""GPU suite of the exploration-goal kernels (csrc/frontier_kernels.h) against the numpy restatement (tests/frontier_np.py, pinned
by test_frontier_cpu.py): the frontier mask, component labels and their table, the view gain, the facades, the C++ header and a
closed exploration loop.  Integers only: every comparison is exact."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import frontier_np as fnp
from tests import occupancy_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZE, ORIGIN, SCALE = (24, 20, 12), (-1.3, 0.7, -0.25), 0.25
PRM = dict(hit=847, miss=-405, lo=-1100, hi=2000, min_range=0.2, max_range=3.0)


@pytest.fixture(scope="module")
def ctx():
    import allocnet_amd as aa
    return aa.default_context()


def _params(**kw):
    import allocnet_amd as aa
    d = dict(PRM); d.update(kw)
    prm = aa.occupancy_params()
    for k, v in d.items():
        setattr(prm, k, v)
    return prm, onp.Params(**d)


def _centre(cell):
    return np.asarray(ORIGIN) + (np.asarray(cell, dtype=np.float64) + 0.5) * SCALE


@pytest.fixture(scope="module")
def scanned():
    """The log-odds of three scans (restatement) on 24 x 20 x 12 at 0.25 m: free, occupied and unknown voxels, computed once."""
    rng = np.random.default_rng(11)
    _, ref_prm = _params()
    L = np.full(int(np.prod(SIZE)), onp.UNKNOWN, dtype=np.int16)
    ext = np.asarray(SIZE) * SCALE
    for frac in ([0.3, 0.35, 0.5], [0.6, 0.6, 0.4], [0.45, 0.2, 0.7]):
        sensor = np.asarray(ORIGIN) + np.asarray(frac) * ext
        d = rng.normal(size=(700, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts = sensor + d * rng.uniform(0.1, 4.5, (700, 1))
        onp.integrate(L, SIZE, ORIGIN, SCALE, ref_prm, sensor, pts)
    assert (L == onp.UNKNOWN).sum() > 500 and (L > 0).sum() > 100 and ((L != onp.UNKNOWN) & (L < 0)).sum() > 500
    L.setflags(write=False)
    return L


def _map_with(ctx, L, prm=None):
    import allocnet_amd as aa
    import torch
    om = aa.OccupancyMap(SIZE, ORIGIN, SCALE, prm or _params()[0], ctx=ctx)
    om.logodds_dev().copy_(torch.from_numpy(np.array(L)))
    return om


# ---- frontier --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [None, ((5, 3, 2), (9, 11, 7)), ((0, 9, 0), (24, 1, 12)), ((23, 19, 11), (1, 1, 1))])
@pytest.mark.parametrize("occ", [0, 900])
def test_frontier_mask_and_count(ctx, scanned, box, occ):
    import torch
    om = _map_with(ctx, scanned)
    want, count = fnp.frontier(scanned, SIZE, occ, box)
    out = torch.full((scanned.size,), 0xFF, dtype=torch.uint8, device=om.device)
    mask, got = om.frontier(occ=occ, box=box, out=out)
    assert mask is out and got == count
    assert np.array_equal(mask.cpu().numpy(), want)                          # every byte written: 0 outside the box
    if box is None or box[1][0] > 1:
        assert count > 20


def test_frontier_refusals_leave_the_mask_untouched(ctx, scanned):
    import allocnet_amd as aa
    import torch
    from allocnet_amd import _lib
    om = _map_with(ctx, scanned)
    out = torch.full((scanned.size,), 0xFF, dtype=torch.uint8, device=om.device)
    for box in [((20, 0, 0), (5, 1, 1)), ((-1, 0, 0), (2, 2, 2)), ((0, 0, 12), (1, 1, 1)), ((0, 0, 0), (1, 0, 1)), ((30, 30, 30), (1, 1, 1))]:
        with pytest.raises(aa.AnetError) as ei:
            om.frontier(box=box, out=out)
        assert ei.value.code == _lib.ANET_ERR_INVALID, box
    assert (out == 0xFF).all().item()


# ---- labels ----------------------------------------------------------------------------------------------------------------------
def _labels(ctx, mask, size, connectivity, rounds=False):
    import allocnet_amd as aa
    import torch
    grid = aa._lib.VoxelGrid()
    for c in range(3):
        grid.size[c] = int(size[c]); grid.origin[c] = 0.0
    grid.scale = 1.0
    dev = torch.device("cuda", ctx.device)
    garbage = torch.randint(-2 ** 31, 2 ** 31 - 1, (mask.size,), dtype=torch.int64, device=dev).to(torch.int32)
    out = aa.label_components_dev(grid, torch.from_numpy(mask).to(dev), connectivity, out=garbage, with_rounds=rounds, ctx=ctx)
    return (out[0].cpu().numpy(), out[1], grid) if rounds else out.cpu().numpy()


@pytest.mark.parametrize("size", [(19, 13, 11), (33, 17, 9), (64, 48, 1), (1, 1, 40)])
def test_labels_of_random_masks(ctx, size):
    """Shapes against the 8 x 8 x 4 tile: below one tile on an axis, odd multiples, flat, a single column; `labels` pre-filled
    with garbage; the empty and the full mask."""
    n = int(np.prod(size))
    rng = np.random.default_rng(n)
    masks = [(rng.uniform(size=n) < d).astype(np.uint8) for d in (0.1, 0.3, 0.6)]
    masks += [np.zeros(n, dtype=np.uint8), np.full(n, 3, dtype=np.uint8)]
    for mask in masks:
        for connectivity in (6, 26):
            want = fnp.label_components(mask, size, connectivity)
            got = _labels(ctx, mask, size, connectivity)
            assert got.dtype == np.int32 and np.array_equal(got, want), (size, connectivity, int(mask.sum()))
    assert (fnp.label_components(masks[-1], size, 6)[0], fnp.label_components(masks[-2], size, 6).max()) == (0, -1)


@pytest.mark.parametrize("touch", ["edge", "corner"])
def test_blobs_touching_across_an_edge_or_a_corner(ctx, touch):
    """One component at 26-connectivity, two at 6; the contact straddles tile borders on every axis it uses."""
    size = (19, 13, 11)
    M = np.zeros((size[2], size[1], size[0]), dtype=np.uint8)
    M[2:4, 5:8, 5:8] = 1                                                    # z 2..3, y 5..7, x 5..7
    if touch == "edge":
        M[2:4, 8:11, 8:11] = 1                                              # shares the edge x = 8, y = 8
    else:
        M[4:6, 8:11, 8:11] = 1                                              # shares the corner x = 8, y = 8, z = 4
    mask = M.reshape(-1)
    for connectivity, k in ((6, 2), (26, 1)):
        want = fnp.label_components(mask, size, connectivity)
        assert len(np.unique(want[want >= 0])) == k
        assert np.array_equal(_labels(ctx, mask, size, connectivity), want)


def test_serpentine_across_every_tile_border(ctx, capsys):
    """A one-voxel-wide serpentine on 64 x 48 x 1: full rows at even y joined at alternating ends, 1559 cells (the longest a
    one-wide path with one-wide gaps can be on this grid), crossing the x tile borders 7 times per row and a y tile border every
    fourth row.  One component at either connectivity.  The rounds are printed, not asserted."""
    size = (64, 48, 1)
    M = np.zeros((48, 64), dtype=np.uint8)
    M[0::2, :] = 1
    for k, y in enumerate(range(1, 47, 2)):
        M[y, 63 if k % 2 == 0 else 0] = 1
    mask = M.reshape(-1)
    assert mask.sum() == 24 * 64 + 23
    for connectivity in (6, 26):
        got, rounds, _ = _labels(ctx, mask, size, connectivity, rounds=True)
        assert np.array_equal(got, fnp.label_components(mask, size, connectivity))
        assert (got[mask != 0] == 0).all()
        with capsys.disabled():
            print(f"\nserpentine, connectivity {connectivity}: {rounds} rounds")


# ---- stats -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_component_table(ctx, connectivity):
    import allocnet_amd as aa
    import torch
    size = (33, 17, 9)
    n = int(np.prod(size))
    # (below the percolation threshold of the connectivity, so that there are many components)
    mask = (np.random.default_rng(3).uniform(size=n) < (0.3 if connectivity == 6 else 0.05)).astype(np.uint8)
    mask[:33 * 17] = 1                                                       # a large component: whole waves of one label
    labels, _, grid = _labels(ctx, mask, size, connectivity, rounds=True)
    root, count, sums, bbox = fnp.component_stats(labels, size)
    assert len(root) > 20 and count.max() > 500 and (np.diff(root) > 0).all()
    dev = torch.device("cuda", ctx.device)
    ld = torch.from_numpy(labels).to(dev)
    for cap in (len(root) + 7, len(root), 5, 0):
        k, r, c, s, b = aa.component_stats_dev(grid, ld, cap, ctx=ctx)
        m = min(cap, len(root))
        assert k == len(root) and len(r) == m                               # the true number, whatever the cap
        assert np.array_equal(r.cpu().numpy(), root[:m]) and np.array_equal(c.cpu().numpy(), count[:m])
        assert s.dtype == torch.int64 and np.array_equal(s.cpu().numpy(), sums[:m])
        assert np.array_equal(b.cpu().numpy(), bbox[:m])


# ---- view gain -------------------------------------------------------------------------------------------------------------------
def _template():
    """8 x 6 frustum points at 2.5 m (inside max_range), the six axis directions beyond it, the eight exact cube diagonals from a
    cell centre (ties), a point inside min_range, a NaN row."""
    K, W, H = (6.0, 6.0, 3.5, 2.5), 8, 6
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = np.full(W * H, 2.5)
    fr = np.stack([(u.reshape(-1) - K[2]) / K[0] * z, (v.reshape(-1) - K[3]) / K[1] * z, z], axis=1)
    axes = np.concatenate([np.eye(3), -np.eye(3)]) * 5.0
    diag = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64) * (6 * SCALE)
    return np.concatenate([fr, axes, diag, [[0.05, 0.0, 0.05]], [[np.nan, 0.0, 1.0]]])


def _rot(rng):
    return np.linalg.qr(rng.normal(size=(3, 3)))[0]


def _views(L):
    """(R (V, 3, 3), t (V, 3)): in free space (axis-aligned at a cell centre: ties), rotated in free space, outside the map looking
    in, in an occupied cell, in an unknown cell, at a map corner, far outside, one with a NaN."""
    rng = np.random.default_rng(2)
    cell = lambda v: (v % SIZE[0], (v // SIZE[0]) % SIZE[1], v // (SIZE[0] * SIZE[1]))  # noqa: E731
    free = np.flatnonzero((L != onp.UNKNOWN) & (L < 0))
    occd = np.flatnonzero((L != onp.UNKNOWN) & (L >= 0))
    occd = occd if len(occd) else free                                          # (a grid without an occupied voxel)
    unk = np.flatnonzero(L == onp.UNKNOWN)
    ext = np.asarray(SIZE) * SCALE
    eye = np.eye(3)
    look_in = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])     # the camera's z along world x
    views = [(eye, _centre(cell(int(free[len(free) // 2])))),
             (_rot(rng), _centre(cell(int(free[len(free) // 3]))) + 0.07 * SCALE),
             (look_in, np.asarray(ORIGIN) + np.array([-0.2, 0.5, 0.5]) * ext),
             (_rot(rng), _centre(cell(int(occd[len(occd) // 2]))) + 0.03),
             (_rot(rng), _centre(cell(int(unk[len(unk) // 2])))),
             (eye, _centre((0, 0, 0))),
             (_rot(rng), _centre((SIZE[0] - 1, SIZE[1] - 1, SIZE[2] - 1)) + 0.1 * SCALE),
             (eye, np.asarray(ORIGIN) + np.array([40.0, -35.0, 50.0])),
             (np.where(np.eye(3) > 0, np.nan, 0.0), _centre((3, 3, 3)))]
    return np.stack([v[0] for v in views]), np.stack([v[1] for v in views])


@pytest.fixture(scope="module")
def gain_case(scanned):
    prm, ref_prm = _params()
    R, t = _views(scanned)
    pts = _template()
    want = fnp.view_gain(scanned, SIZE, ORIGIN, SCALE, ref_prm, 0, R, t, pts)
    return prm, R, t, pts, want


def _gain(ctx, om, prm, R, t, pts, occ=0, work=None):
    import allocnet_amd as aa
    import torch
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(om.device)  # noqa: E731
    return aa.view_gain_dev(om, prm, om.logodds_dev(), d(R), d(t), d(pts), occ, work=work, ctx=ctx).cpu().numpy()


def test_view_gain_against_the_restatement(ctx, scanned, gain_case):
    prm, R, t, pts, want = gain_case
    assert want[3] == 0 and want[7] == 0 and want[8] == -1                  # in an occupied cell, far outside, NaN
    assert (want[[0, 1, 2, 4, 5, 6]] > 0).all(), want
    om = _map_with(ctx, scanned, prm)
    got = _gain(ctx, om, prm, R, t, pts)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    # another threshold: what blocks changes, and so does the count
    _, ref_prm = _params()
    want2 = fnp.view_gain(scanned, SIZE, ORIGIN, SCALE, ref_prm, 2000, R, t, pts)
    assert not np.array_equal(want2, want)
    assert np.array_equal(_gain(ctx, om, prm, R, t, pts, occ=2000), want2)
    # the method on the map
    assert np.array_equal(om.viewGain(R, t, pts), want)
    assert len(om.viewGain(R[:0], t[:0], pts)) == 0 and np.array_equal(om.viewGain(R, t, pts[:0]), np.where(want < 0, -1, 0))


def test_view_gain_does_not_depend_on_the_chunking_and_leaves_zero_marks(ctx, scanned, gain_case):
    import allocnet_amd as aa
    import torch
    from allocnet_amd import frontier as fr
    prm, R, t, pts, want = gain_case
    om = _map_with(ctx, scanned, prm)
    one = fr.view_gain_workspace(om, prm, None, ctx=ctx)
    assert fr.view_gain_workspace(om, prm, 1, ctx=ctx) == one and fr.view_gain_workspace(om, prm, len(t), ctx=ctx) == len(t) * one
    for views in (len(t), 1, 3):
        work = torch.zeros(views * one + (7 if views == 3 else 0), dtype=torch.uint8, device=om.device)
        assert np.array_equal(_gain(ctx, om, prm, R, t, pts, work=work), want), views
        assert not work.any().item(), "marks left behind"
        assert np.array_equal(_gain(ctx, om, prm, R, t, pts, work=work), want), views      # and the workspace is reusable as it is
    short = torch.zeros(one - 1, dtype=torch.uint8, device=om.device)
    with pytest.raises(aa.AnetError) as ei:
        _gain(ctx, om, prm, R, t, pts, work=short)
    assert ei.value.code == aa._lib.ANET_ERR_INVALID


def test_view_gain_is_a_function_of_the_set_of_template_points(ctx, scanned, gain_case):
    prm, R, t, pts, want = gain_case
    om = _map_with(ctx, scanned, prm)
    rng = np.random.default_rng(9)
    for variant in (pts[rng.permutation(len(pts))], np.repeat(pts, 2, axis=0), np.concatenate([pts[::-1], pts[:20]])):
        assert np.array_equal(_gain(ctx, om, prm, R, t, variant), want)


def test_view_gain_is_what_a_scan_reveals(ctx):
    """On a grid with no occupied voxel, gain[v] == the drop of the UNKNOWN count after anet_occupancy_integrate_dev of the same world
    points from the same origin, on a copy: both device paths, no restatement of the walk."""
    import allocnet_amd as aa
    prm, ref_prm = _params()
    rng = np.random.default_rng(21)
    om = aa.OccupancyMap(SIZE, ORIGIN, SCALE, prm, ctx=ctx)
    ext = np.asarray(SIZE) * SCALE
    sensor = np.asarray(ORIGIN) + 0.4 * ext
    d = rng.normal(size=(400, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    om.integrate(sensor + 50.0 * d, sensor)                                 # every ray truncated: misses only, nothing occupied
    L0 = om.getLogOdds()
    assert not ((L0 != onp.UNKNOWN) & (L0 >= 0)).any() and 200 < (L0 != onp.UNKNOWN).sum() < L0.size - 500
    pts = _template()
    R, t = _views(L0)
    R, t = R[:8], t[:8]
    got = _gain(ctx, om, prm, R, t, pts)
    for v in range(len(t)):
        cp = _map_with(ctx, L0, prm)
        cp.integrate(fnp.world_points(R[v], t[v], pts), t[v])
        drop = int((L0 == onp.UNKNOWN).sum() - (cp.getLogOdds() == onp.UNKNOWN).sum())
        assert got[v] == drop, (v, got[v], drop)
    assert (got > 0).sum() >= 5


# ---- facades ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_frontier_clusters_table(ctx, scanned, connectivity):
    import allocnet_amd as aa
    om = _map_with(ctx, scanned)
    root, count, cen, lo, hi = fnp.clusters(scanned, SIZE, ORIGIN, SCALE, 0, 4, connectivity)
    assert len(root) >= 2
    for tab in (om.frontierClusters(0, 4, connectivity), aa.frontier_clusters(om, occ=0, min_size=4, connectivity=connectivity)):
        assert np.array_equal(tab["root"], root) and np.array_equal(tab["count"], count)
        assert tab["centroid"].tobytes() == cen.tobytes()
        assert np.array_equal(tab["cells_lo"], lo) and np.array_equal(tab["cells_hi"], hi)
        assert tab["n_components"] >= len(root)
    box = ((4, 2, 1), (12, 14, 9))
    root, count, cen, lo, hi = fnp.clusters(scanned, SIZE, ORIGIN, SCALE, 0, 1, connectivity, box)
    tab = om.frontierClusters(0, 1, connectivity, box)
    assert np.array_equal(tab["root"], root) and np.array_equal(tab["count"], count) and tab["n_components"] == len(root)


def test_voxel_map_components(ctx, scanned):
    om = _map_with(ctx, scanned)
    vm = om.to_voxel_map(occ=0, unknown="blocked")
    vox = vm.getVoxels()
    for connectivity in (6, 26):
        assert np.array_equal(vm.components(connectivity).cpu().numpy(), fnp.label_components(vox == 0, SIZE, connectivity))
    assert np.array_equal(vm.components(6, free=False).cpu().numpy(), fnp.label_components(vox != 0, SIZE, 6))


def test_cpp_frontier_program(ctx, scanned):
    src = os.path.join(ROOT, "tests", "cpp", "test_frontier.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    prm, ref_prm = _params()
    R, t = _views(scanned)
    R, t, pts = R[:3], t[:3], _template()
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "test_frontier")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        np.array(scanned).tofile(os.path.join(td, "logodds.bin"))
        np.concatenate([R.reshape(-1), t.reshape(-1)]).tofile(os.path.join(td, "views.bin"))
        pts.tofile(os.path.join(td, "pts.bin"))
        res = subprocess.run([exe, td], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
        out = dict(line.split("=") for line in res.stdout.split() if "=" in line)
    mask, count = fnp.frontier(scanned, SIZE, 0)
    root, cnt, _, _, _ = fnp.clusters(scanned, SIZE, ORIGIN, SCALE, 0, 4, 26)
    free = fnp.label_components(onp.to_voxels(scanned, 0, True) == 0, SIZE, 6)
    assert int(out["frontier"]) == count
    assert int(out["clusters"]) == len(root) and int(out["largest"]) == cnt.max()
    assert int(out["free_components"]) == len(np.unique(free[free >= 0]))
    want = fnp.view_gain(scanned, SIZE, ORIGIN, SCALE, ref_prm, 0, R, t, pts)
    assert [int(v) for v in out["gain"].split(",")] == want.tolist()


# ---- a closed loop ---------------------------------------------------------------------------------------------------------------
def test_closed_exploration_loop(ctx):
    """A 40 x 40 x 10 room at 0.25 m with walls and one pillar; the sensor is the truth map's ray query; at most 30 poses.  At the
    end no frontier cluster of min_size is left in the robot's component, more is known than after the first scan, no truly
    occupied voxel is held free, and every goal was in a free cell of the robot's component when it was chosen."""
    import allocnet_amd as aa
    import torch
    size, origin, scale, max_range, min_size = (40, 40, 10), (0.0, 0.0, 0.0), 0.25, 3.0, 6
    T = np.zeros((10, 40, 40), dtype=np.uint8)
    T[:, 0, :] = T[:, -1, :] = T[:, :, 0] = T[:, :, -1] = 1
    T[0] = T[-1] = 1
    T[:, 17:22, 17:22] = 1
    truth = aa.VoxelMap(size, origin, scale, ctx=ctx)
    truth.voxels_dev.copy_(torch.from_numpy(T.reshape(-1)))
    om = aa.OccupancyMap(size, origin, scale, aa.occupancy_params(min_range=0.0, max_range=max_range), ctx=ctx)
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    az = (np.arange(96) + 0.5) * (2 * np.pi / 96)
    el = -0.5 * np.pi + (np.arange(48) + 0.5) * (np.pi / 48)
    a, e = np.meshgrid(az, el, indexing="ij")
    dirs = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1).reshape(-1, 3)
    reach = 1.5 * max_range
    dd = torch.from_numpy(dirs).to(om.device)
    template = reach * dd

    def scan(pose):
        o = torch.from_numpy(pose).to(om.device).expand(len(dirs), 3).contiguous()
        q = o + reach * dd
        voxel, tt = aa.voxel_raycast_dev(truth, truth.voxels_dev, o, q)
        tt = torch.where(voxel >= 0, tt + 1e-6 * scale / reach, torch.ones_like(tt))
        om.integrate(o + tt[:, None] * (q - o), pose)

    def cell_id(p):
        c = np.floor((np.asarray(p) - origin) / scale).astype(int)
        return int(c[0] + 40 * (c[1] + 40 * c[2]))

    pose = np.array([2.1, 2.1, 1.3])
    first = None
    for k in range(30):
        scan(pose)
        first = om.known_fraction() if first is None else first
        om.to_voxel_map(occ=0, unknown="blocked", out=vm)
        nv = aa.next_view(om, vm, pose, template, occ=0, min_size=min_size, connectivity=26, radii=(0.75, 1.5), n_yaw=6)
        if len(nv["order"]) == 0 or nv["utility"][nv["order"][0]] <= 0.0:
            break
        goal = nv["t"][nv["order"][0]]
        free = vm.components(6).cpu().numpy()
        assert vm.getVoxels()[cell_id(goal)] == 0 and free[cell_id(goal)] == free[cell_id(pose)] >= 0, (k, goal)
        pose = goal
    assert k < 29, "the pose budget ran out"
    L = om.getLogOdds()
    # no cluster of min_size with a voxel in the robot's component is left
    free = fnp.label_components(onp.to_voxels(L, 0, True) == 0, size, 6)
    mask, _ = fnp.frontier(L, size, 0)
    labels = fnp.label_components(mask, size, 26)
    root, count, _, _ = fnp.component_stats(labels, size)
    for r in root[count >= min_size]:
        assert not (free[labels == r] == free[cell_id(pose)]).any(), int(r)
    assert om.known_fraction() > first
    assert not ((T.reshape(-1) != 0) & (L != onp.UNKNOWN) & (L < 0)).any()
