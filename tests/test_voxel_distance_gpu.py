"""The distance field of the voxel map on the device (anet_voxel_distance_dev), its query and the obstacle penalty of the MINCO
objective against the restatement of tests/dist_np.py: the transform bit for bit against brute force, the query against the stated
interpolant and the exact tools that exist, the penalty's values and contracts, the composed objective end to end and under the
lockstep L-BFGS."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dist_np as dn

pytestmark = pytest.mark.gpu
DEV = "cuda"
NONE = dn.NONE


def _grid(size, origin=(0.0, 0.0, 0.0), scale=1.0):
    from allocnet_amd._lib import VoxelGrid
    g = VoxelGrid()
    for c in range(3):
        g.size[c], g.origin[c] = int(size[c]), float(origin[c])
    g.scale = float(scale)
    return g


def _transform(anet_ctx, vox, walls, **kw):
    """vox [x, y, z] uint8 -> the device field as a flat CPU int32 tensor (x fastest)."""
    import allocnet_amd as aa
    d_vox = torch.from_numpy(dn.flat(vox.astype(np.uint8))).to(DEV)
    out = aa.distance_transform_dev(_grid(vox.shape, **kw), d_vox, walls, ctx=anet_ctx)
    torch.cuda.synchronize()
    return out


def _expect(sd2_xyz):
    return torch.from_numpy(dn.flat(sd2_xyz).astype(np.int32))


def _random_vox(rng, size, density, twos=False):
    vox = (rng.uniform(size=size) < density).astype(np.uint8)
    if twos:
        vox *= rng.integers(1, 3, size=size).astype(np.uint8)
    return vox


# ---------------------------------------------------------------------------------------------
# the transform
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walls", [0, 1])
def test_smallest_map_and_sentinels(anet_ctx, walls):
    free, blocked = np.zeros((1, 1, 1), np.uint8), np.ones((1, 1, 1), np.uint8)
    assert _transform(anet_ctx, free, walls).cpu().tolist() == [1 if walls else NONE]
    assert _transform(anet_ctx, blocked, walls).cpu().tolist() == [-NONE]


def _two_on_a_line(size):
    """two blocked voxels only, near the two ends of the long axis: parabolas that reach across the whole line"""
    vox = np.zeros(size, np.uint8)
    far = [n - 1 for n in size]
    vox[0, 0, 0] = 1
    vox[far[0] - (size[0] > 100) * 3, far[1] - (size[1] > 100) * 3, far[2] - (size[2] > 100) * 3] = 1
    return vox


CASES = {
    "small": lambda rng: _random_vox(rng, (7, 5, 3), 0.3),
    "sparse": lambda rng: _random_vox(rng, (2, 1, 9), 0.2),
    "long_x": lambda rng: _two_on_a_line((130, 3, 2)),
    "long_y": lambda rng: _two_on_a_line((3, 130, 2)),
    "long_z": lambda rng: _two_on_a_line((2, 3, 130)),
    "tile_edges": lambda rng: _random_vox(rng, (70, 66, 5), 0.01, twos=True),
    "x_tiles": lambda rng: _random_vox(rng, (140, 150, 2), 0.01),       # three x tiles of 64 in the y pass, the last 12 wide
}


@pytest.mark.parametrize("walls", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_transform_equals_brute_force(anet_ctx, name, walls):
    vox = CASES[name](np.random.default_rng(len(name)))
    assert vox.any() and not vox.all()
    if name == "tile_edges":
        assert (vox == 2).any() and (vox == 1).any()
    want = _expect(dn.brute_sd2(vox, walls))
    got = _transform(anet_ctx, vox, walls)
    assert torch.equal(got.cpu(), want), (name, walls, int((got.cpu() != want).sum()))
    assert torch.equal(_transform(anet_ctx, vox, walls), got)            # the same bits on a second run


def test_empty_map_with_walls_is_the_closed_form(anet_ctx):
    size = (9, 70, 4)
    x, y, z = np.meshgrid(*[np.arange(n) for n in size], indexing="ij")
    edge = np.minimum.reduce([x + 1, size[0] - x, y + 1, size[1] - y, z + 1, size[2] - z])
    assert torch.equal(_transform(anet_ctx, np.zeros(size, np.uint8), 1).cpu(), _expect(edge * edge))
    assert (_transform(anet_ctx, np.zeros(size, np.uint8), 0) == NONE).all()


@pytest.mark.parametrize("walls", [0, 1])
def test_full_map_is_the_negative_sentinel(anet_ctx, walls):
    assert (_transform(anet_ctx, np.full((9, 70, 4), 2, np.uint8), walls) == -NONE).all()


@pytest.mark.parametrize("walls", [0, 1])
def test_longest_axis_against_the_closed_form(anet_ctx, walls):
    vox = np.zeros((4096, 1, 1), np.uint8)
    vox[0] = vox[-1] = 1
    x = np.arange(4096)
    want = np.minimum(x, 4095 - x) ** 2
    if walls:
        want = np.minimum(want, 1)                                       # the walls beside the single row and column
    want[0] = want[-1] = -1
    assert torch.equal(_transform(anet_ctx, vox, walls).cpu(), torch.from_numpy(want.astype(np.int32)))
    # along y and z the same line, tiles of four and fewer x
    for size in ((1, 4096, 1), (1, 1, 4096)):
        assert torch.equal(_transform(anet_ctx, vox.reshape(size), walls).cpu(), torch.from_numpy(want.astype(np.int32)))


def test_one_voxel_longer_is_unsupported(anet_ctx):
    import allocnet_amd as aa
    from allocnet_amd._lib import ANET_ERR_UNSUPPORTED, ANET_ERR_INVALID
    for size in ((4097, 1, 1), (1, 4097, 1), (1, 1, 4097)):
        with pytest.raises(aa.AnetError) as e:
            _transform(anet_ctx, np.zeros(size, np.uint8), 1)
        assert e.value.code == ANET_ERR_UNSUPPORTED
    g = _grid((2, 2, 2))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(8, dtype=torch.int32, device=DEV)
    assert anet_ctx.lib.anet_voxel_distance_dev(anet_ctx.handle, ctypes.byref(g), None, 1, ctypes.c_void_p(buf.data_ptr()), st) == ANET_ERR_INVALID
    g.scale = 0.0
    vox = torch.zeros(8, dtype=torch.uint8, device=DEV)
    assert anet_ctx.lib.anet_voxel_distance_dev(anet_ctx.handle, ctypes.byref(g), ctypes.c_void_p(vox.data_ptr()), 1,
                                                ctypes.c_void_p(buf.data_ptr()), st) == ANET_ERR_INVALID


# ---------------------------------------------------------------------------------------------
# the query
# ---------------------------------------------------------------------------------------------
SIZE, ORIGIN, SCALE = (24, 20, 12), (-1.0, -0.5, 0.0), 0.25


class Field:
    """A random map, its field by brute force on the host (the device's is checked against it once) and on the device."""
    _cache = {}

    def __init__(self, anet_ctx, size=SIZE, origin=ORIGIN, scale=SCALE, density=0.08, walls=1, seed=11):
        rng = np.random.default_rng(seed)
        self.size, self.origin, self.scale, self.walls = size, origin, scale, walls
        self.vox = _random_vox(rng, size, density)
        self.sd2 = dn.brute_sd2(self.vox, walls)
        self.grid = _grid(size, origin, scale)
        self.d_sd2 = _transform(anet_ctx, self.vox, walls, origin=origin, scale=scale)
        assert torch.equal(self.d_sd2.cpu(), _expect(self.sd2))
        self.kw = dict(sd2=self.sd2, size=size, origin=origin, scale=scale)
        self.lo, self.hi = np.array(origin), np.array(origin) + scale * np.array(size)

    @classmethod
    def get(cls, anet_ctx, **kw):
        key = tuple(sorted(kw.items()))
        if key not in cls._cache:
            cls._cache[key] = cls(anet_ctx, **kw)
        return cls._cache[key]

    def query(self, anet_ctx, pos, grad=True):
        import allocnet_amd as aa
        d, g = aa.distance_query_dev(self.grid, self.d_sd2, torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64)).to(DEV),
                                     grad=grad, ctx=anet_ctx)
        torch.cuda.synchronize()
        return d.cpu().numpy(), (g.cpu().numpy() if grad else None)


def _points(rng, f, n):
    """uniform points inside, within half a voxel of each face (both sides), and outside"""
    inside = rng.uniform(f.lo, f.hi, (n, 3))
    near = rng.uniform(f.lo, f.hi, (n, 3))
    ax = rng.integers(0, 3, n)
    face = np.where(rng.integers(0, 2, n) == 0, f.lo[ax], f.hi[ax])
    near[np.arange(n), ax] = face + rng.uniform(-0.5, 0.5, n) * f.scale
    outside = rng.uniform(f.lo - 3.0, f.hi + 3.0, (n, 3))
    return np.concatenate([inside, near, outside])


@pytest.mark.parametrize("size", [SIZE, (9, 1, 5)])
@pytest.mark.parametrize("n", [1, 1000])
def test_query_matches_the_restatement(anet_ctx, size, n):
    """dist and grad within 1e-12 max(1, max|D|): about ten roundings of 1.1e-16 on values bounded by max|D|, a thousandfold margin.
    Gradient rows are compared only where the restatement's |u - round(u)| >= 1e-6 (the share left out is <= 1 %)."""
    f = Field.get(anet_ctx, size=size)
    pos = _points(np.random.default_rng(n + size[1]), f, n)
    d, g = f.query(anet_ctx, pos)
    rd, rg = dn.query(pos=pos, **f.kw)
    bar = 1e-12 * max(1.0, np.abs(dn.centre_values(f.sd2, f.scale)).max())
    u = dn.cell_of(pos, f.size, f.origin, f.scale)[0]
    keep = (np.abs(u - np.round(u)) >= 1e-6).all(1)
    print(f"size {size} n {n}: dist error {np.abs(d - rd).max():.3e}, grad error {np.abs(g - rg)[keep].max():.3e} (bar {bar:.3e}); "
          f"{(~keep).sum()} of {len(keep)} gradient rows left out")
    assert np.isfinite(rd).all() and (~keep).mean() <= 0.01
    assert np.abs(d - rd).max() <= bar
    assert np.abs(g - rg)[keep].max() <= bar
    assert (g[:, 1] == 0.0).all() if size[1] == 1 else (n == 1 or np.abs(g[:, 1]).max() > 0.0)
    d_only, none = f.query(anet_ctx, pos, grad=False)
    assert none is None and np.array_equal(d_only, d)


def test_query_at_exact_centres_is_the_centre_value_to_the_bit(anet_ctx):
    """scale is a power of two, so the centres are exact: dist == D(v); <= 0 at every blocked voxel and > 0 at every free one."""
    f = Field.get(anet_ctx)
    ids = np.stack(np.meshgrid(*[np.arange(k) for k in f.size], indexing="ij"), -1).reshape(-1, 3)
    centres = np.array(f.origin) + 0.5 * f.scale + ids * f.scale
    d, _ = f.query(anet_ctx, centres)
    assert np.array_equal(d, dn.centre_values(f.sd2, f.scale).reshape(-1))
    blocked = f.vox.reshape(-1) != 0
    assert (d[blocked] <= 0.0).all() and (d[~blocked] > 0.0).all()


def test_query_nan_row_and_uniform_map(anet_ctx):
    import allocnet_amd as aa
    f = Field.get(anet_ctx)
    pos = np.random.default_rng(2).uniform(f.lo, f.hi, (5, 3))
    good = f.query(anet_ctx, pos)
    bad = pos.copy()
    bad[1, 2], bad[3, 0] = np.nan, np.inf
    d, g = f.query(anet_ctx, bad)
    rest = [0, 2, 4]
    assert np.isnan(d[[1, 3]]).all() and np.isnan(g[[1, 3]]).all()
    assert np.array_equal(d[rest], good[0][rest]) and np.array_equal(g[rest], good[1][rest])
    empty = _transform(anet_ctx, np.zeros(f.size, np.uint8), 0)
    d, g = aa.distance_query_dev(f.grid, empty, torch.from_numpy(pos).to(DEV), ctx=anet_ctx)
    assert (d == float("inf")).all() and (g == 0.0).all()
    d, g = aa.distance_query_dev(f.grid, empty, torch.zeros((0, 3), dtype=torch.float64, device=DEV), ctx=anet_ctx)   # n == 0
    assert d.numel() == 0


def test_get_distance_agrees_with_traj_clearance_on_a_single_voxel(anet_ctx):
    """A map whose blocked set is one voxel: getDistance at the centre of every free voxel is the exact clearance of a constant piece
    there to that voxel's centre, within 1e-12.  The cache: dropped by setOccupied, bypassed by writes through voxels_dev."""
    import allocnet_amd as aa
    size, origin, scale = (5, 4, 3), (0.5, -1.0, 2.0), 0.5
    vm = aa.VoxelMap(size, origin, scale, ctx=anet_ctx)
    assert (vm.distance_field(walls=False) == NONE).all()
    vm.setOccupied(np.array([[2, 1, 1]], dtype=np.int32))
    field = vm.distance_field(walls=False)
    assert field.dtype == torch.int32 and field.is_cuda and field[2 + 5 * (1 + 4 * 1)].item() == -1
    assert vm.distance_field(walls=False) is field and vm.distance_field(walls=True) is not field
    ids = np.stack(np.meshgrid(*[np.arange(k) for k in size], indexing="ij"), -1).reshape(-1, 3)
    ids = ids[(ids != [2, 1, 1]).any(1)]
    centres = vm.posI2D(ids)
    d = vm.getDistance(centres, walls=False)
    co = np.zeros((len(ids), 1, 3, 6))
    co[:, 0, :, -1] = centres
    cl = aa.traj_clearance(co, np.ones((len(ids), 1)), vm.posI2D(np.array([[2, 1, 1]])), ctx=anet_ctx)[0][:, 0]
    print(f"getDistance against traj_clearance: worst {np.abs(d - cl).max():.3e} (bar 1e-12)")
    assert np.abs(d - cl).max() <= 1e-12
    one, g1 = vm.getDistance(centres[0], grad=True, walls=False)
    assert isinstance(one, float) and one == d[0] and g1.shape == (3,)
    assert vm.getDistance(vm.posI2D(np.array([2, 1, 1])), walls=False) == -scale
    vm.voxels_dev[0] = 1                                                   # behind the map's back
    assert vm.distance_field(walls=False)[0].item() > 0
    assert vm.distance_field(walls=False, refresh=True)[0].item() == -1
    vm.dilate(1)
    assert (vm.distance_field(walls=False)[:2] < 0).all()


def test_cpp_members_program(anet_ctx):
    """tests/cpp/test_voxel_distance.cpp: VoxelMap::distanceField with and without walls (computed after a setOccupied that is still
    buffered) and both getDistance overloads print what the restatement gives on the same 6 x 5 x 4 map with one blocked voxel."""
    import json
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, lib = os.path.join(root, "tests", "cpp", "test_voxel_distance.cpp"), os.path.join(root, "allocnet_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "test_voxel_distance")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads(res.stdout)
    size, origin, scale = (6, 5, 4), (-1.0, 0.0, 0.25), 0.5
    vox = np.zeros(size, np.uint8)
    vox[2, 2, 1] = 1
    p = np.array([[0.1, 1.3, 0.9]])
    for walls in (0, 1):
        sd2 = dn.brute_sd2(vox, walls)
        assert out["sd2_%d" % walls] == [int(sd2[0, 0, 0]), int(sd2[2, 2, 1]), int(sd2[5, 4, 3])]
        d, g = dn.query(sd2, size, origin, scale, p)
        if walls:
            assert abs(out["dist"] - d[0]) <= 1e-12 and np.abs(np.array(out["grad"]) - g[0]).max() <= 1e-12
            assert np.abs(g[0]).max() > 0.0
        else:
            assert abs(out["dist_no_walls"] - d[0]) <= 1e-12
    assert out["sd2_1"][1] == -1 and out["dist"] != out["dist_no_walls"]


# ---------------------------------------------------------------------------------------------
# the penalty against the restatement
# ---------------------------------------------------------------------------------------------
def _bm(a, ld, fill=0.0):
    """(n, f) numpy -> batch-minor torch tensor (f, ld) on the device."""
    a = np.asarray(a, dtype=np.float64)
    t = torch.full((a.shape[1], ld), fill, dtype=torch.float64)
    t[:, :a.shape[0]] = torch.from_numpy(a.reshape(a.shape[0], -1)).T
    return t.to(DEV)


def _pieces(rng, f, B, N, s, res):
    """Random polynomial pieces around points inside the map (not continuous at the knots: the formulas hold piece by piece).
    A trajectory is drawn again until none of its samples lies within 1e-4 voxel of a lattice plane, where the interpolant's
    gradient jumps."""
    D = 2 * s
    co, T = np.empty((B, N, 3, D)), np.empty((B, N))
    for b in range(B):
        for _ in range(100):
            c = rng.normal(size=(N, 3, D)) * 0.3 ** (D - 1 - np.arange(D))
            c[..., -1] = rng.uniform(f.lo + 0.4, f.hi - 0.4, (N, 3))
            t = rng.uniform(0.6, 1.4, N)
            if dn.all_d(c[None], t[None], res, **f.kw)[1] >= 1e-4:
                break
        co[b], T[b] = c, t
    return co, T


class Case:
    def __init__(self, anet_ctx, s, N, B, res, seed, f=None, w=40.0):
        self.f = f or Field.get(anet_ctx)
        self.s, self.N, self.B, self.res, self.w = s, N, B, res, w
        self.co, self.T = _pieces(np.random.default_rng(seed), self.f, B, N, s, res)
        d, off = dn.all_d(self.co, self.T, res, **self.f.kw)
        clearance, mu, frac = dn.limits_from(d)
        if len(d) < 2:
            # one sample has no percentiles (the rule would put the clearance AT its d: x = 0, every reference value zero): a fixed
            # mu and the sample in the middle of the blend, x = clearance - d = mu / 2, so that cost and gradients are not zero
            mu = 0.05
            clearance, frac = float(d[0]) + 0.5 * mu, 1.0
        print(f"{len(d)} samples, active on {100 * frac:.1f} %, nearest lattice plane {off:.3e} voxel; clearance {clearance:.4f} m, "
              f"mu {mu:.4f} m")
        assert off >= 1e-4
        if len(d) >= 50:
            assert 0.1 <= frac <= 0.9
        self.n_samples = len(d)
        self.kw = dict(res=res, w=w, mu=mu, clearance=clearance, **self.f.kw)

    def penalty(self):
        import allocnet_amd as aa
        return aa.make_obstacle_penalty(w=self.kw["w"], smooth_mu=self.kw["mu"], clearance=self.kw["clearance"], res=self.res)

    def device(self, ld=None):
        import allocnet_amd as aa
        ld = ld or (aa.recommended_ld(self.B) if self.B > 1 else 1)
        return dict(ld=ld, co=_bm(self.co.reshape(self.B, -1), ld), T=_bm(self.T, ld, fill=1.0))

    def launch(self, anet_ctx, d=None, pen=None, accumulate=False, into=None, fill=float("nan"), field=None):
        """-> the device tensors gdC, gdT, piece_cost (whole rows, padding lanes included)."""
        import allocnet_amd as aa
        d = d or self.device()
        ld = d["ld"]
        if into is None:
            into = tuple(torch.full(shape, fill, dtype=torch.float64, device=DEV)
                         for shape in ((self.N * 3 * 2 * self.s, ld), (self.N, ld), (self.N, ld)))
        aa.minco_obstacle_partial_grads_dev(pen or self.penalty(), self.s, self.N, self.B, d["co"], d["T"],
                                            field or (self.f.grid, self.f.d_sd2), into[0], into[1], into[2], accumulate=accumulate,
                                            ctx=anet_ctx)
        torch.cuda.synchronize()
        return into

    def numpy(self, out):
        B, N, D = self.B, self.N, 2 * self.s
        gC, gT, pc = out
        return pc[:, :B].T.cpu().numpy(), gC[:, :B].T.cpu().numpy().reshape(B, N, 3, D), gT[:, :B].T.cpu().numpy()


SHAPES = {
    "one": dict(s=2, N=1, B=1, res=1),
    "quad": dict(s=2, N=4, B=5, res=9),                                 # order 2 with enough samples for both conditions
    "ragged": dict(s=3, N=5, B=3, res=5),
    "wide": dict(s=4, N=8, B=130, res=20),                              # ld > B
    "rounds": dict(s=3, N=16, B=2, res=64),                             # 1024 samples: more than one round
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_matches_the_restatement(anet_ctx, name):
    """cost 1e-9 relative; gdC and gdT 1e-7 scaled by max(1, max|ref|): the avoidance term's bars.  The reference is not zero at any
    shape.  `one` has a single sample and so no percentiles: its clearance is d + mu / 2 with mu = 0.05 (Case), a deviation from the
    percentile rule; `quad` is order 2 under the rule with both conditions asserted."""
    case = Case(anet_ctx, seed=1000 + len(name), **SHAPES[name])
    d = case.device()
    assert d["ld"] > case.B or name != "wide"
    pc, gC, gT = case.numpy(case.launch(anet_ctx, d=d))
    rpc, rgC, rgT = dn.j_obs_grads(case.co, case.T, **case.kw)
    cost, rcost = pc.sum(1), rpc.sum(1)
    rel = np.abs(cost - rcost) / np.maximum(np.abs(rcost), 1e-300)
    rel[rcost == 0.0] = np.abs(cost[rcost == 0.0])
    errs = {n: np.abs(g - r).max() / max(1.0, np.abs(r).max()) for n, g, r in (("gdC", gC, rgC), ("gdT", gT, rgT))}
    print(f"{name} cost: worst relative {rel.max():.3e} (bar 1e-9); " + ", ".join(f"{n}: {e:.3e}" for n, e in errs.items()) +
          f" (bar 1e-7); max |ref| {np.abs(rgC).max():.3e}, {np.abs(rgT).max():.3e}")
    assert np.abs(rgC).max() > 0.0 and np.abs(rgT).max() > 0.0 and (rcost > 0.0).any()
    assert np.abs(gC).max() > 0.0 and np.abs(gT).max() > 0.0
    assert rel.max() <= 1e-9
    assert all(e <= 1e-7 for e in errs.values()), errs


# ---------------------------------------------------------------------------------------------
# the penalty's contracts
# ---------------------------------------------------------------------------------------------
def test_accumulate_contract(anet_ctx):
    """accumulate = 1 after anet_minco_partial_grads_dev equals the sum of the separate results to the last bit; accumulate = 0
    overwrites a NaN-poisoned buffer; lanes in [B, ld) keep a sentinel."""
    import allocnet_amd as aa
    case = Case(anet_ctx, seed=1004, **SHAPES["wide"])
    s, N, B = case.s, case.N, case.B
    d = case.device()
    ld = d["ld"]
    assert ld > B
    own = case.launch(anet_ctx, d=d)                                     # onto NaN
    for t in own:
        assert torch.isfinite(t[..., :B]).all() and torch.isnan(t[..., B:]).all()
    pen = aa.make_penalty(rho=0.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=case.res)
    acc = tuple(torch.full_like(t, 123.0) for t in own)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    anet_ctx.check(anet_ctx.lib.anet_minco_partial_grads_dev(anet_ctx.handle, s, N, B, ld, q(d["co"]), q(d["T"]), None,
                                                             ctypes.cast(ctypes.pointer(pen), ctypes.c_void_p), 1, q(acc[0]),
                                                             q(acc[1]), q(acc[2]), st))
    torch.cuda.synchronize()
    sums = [e[..., :B] + f[..., :B] for e, f in zip(acc, own)]
    assert float(acc[2][:, :B].sum()) > 0.0 and float(own[2][:, :B].sum()) > 0.0
    case.launch(anet_ctx, d=d, accumulate=True, into=acc)
    for got, ref in zip(acc, sums):
        assert torch.equal(got[..., :B], ref)
        assert (got[..., B:] == 123.0).all()
    # piece_cost may be NULL
    two = tuple(torch.full_like(t, float("nan")) for t in own[:2])
    aa.minco_obstacle_partial_grads_dev(case.penalty(), s, N, B, d["co"], d["T"], (case.f.grid, case.f.d_sd2), two[0], two[1], None,
                                        ctx=anet_ctx)
    torch.cuda.synchronize()
    assert torch.equal(two[0][:, :B], own[0][:, :B]) and torch.equal(two[1][:, :B], own[1][:, :B])


def test_same_bits_alone_and_at_another_stride(anet_ctx):
    """The outputs of three trajectories: the whole batch in one launch, at another ld, and each alone in a launch of its own."""
    import allocnet_amd as aa
    case = Case(anet_ctx, seed=1004, **SHAPES["wide"])
    B = case.B
    whole = case.launch(anet_ctx)
    wide = case.launch(anet_ctx, d=case.device(ld=B + 3))
    for a, b in zip(whole, wide):
        assert torch.equal(a[..., :B], b[..., :B])
    d = case.device()
    for b in (0, 64, 129):
        one = tuple(torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
                    for shape in ((case.N * 3 * 2 * case.s, 1), (case.N, 1), (case.N, 1)))
        aa.minco_obstacle_partial_grads_dev(case.penalty(), case.s, case.N, 1, d["co"][:, b:b + 1].contiguous(),
                                            d["T"][:, b:b + 1].contiguous(), (case.f.grid, case.f.d_sd2), *one, ctx=anet_ctx)
        torch.cuda.synchronize()
        for a, w in zip(one, whole):
            assert torch.equal(a[..., 0], w[..., b]), b


def test_exact_zeros_and_nan_isolation(anet_ctx):
    case = Case(anet_ctx, seed=1006, **SHAPES["ragged"])
    B = case.B
    # 100 m and more inside free space, walls = 0: a 400 m map at 10 m voxels whose only blocked voxel is at the far end
    far = Field.get(anet_ctx, size=(40, 4, 4), origin=(-300.0, -20.0, -20.0), scale=10.0, density=0.0, walls=0)
    vox = np.zeros(far.size, np.uint8)
    vox[0, 0, 0] = 1
    sd2 = _transform(anet_ctx, vox, 0, origin=far.origin, scale=far.scale)
    assert dn.query(dn.unflat(sd2.cpu().numpy(), far.size), far.size, far.origin, far.scale, case.co[:, :, :, -1].reshape(-1, 3))[0].min() > 100.0
    for field in ((far.grid, sd2), (far.grid, far.d_sd2)):               # ... and the +NONE map: d = +inf
        out = case.launch(anet_ctx, field=field)
        for t in out:
            assert (t[..., :B] == 0.0).all() and torch.isnan(t[..., B:]).all()
    assert (far.d_sd2 == NONE).all()
    # a duration of trajectory 1 that is not positive: NaN there, the same bits elsewhere; lanes in [B, ld) keep their sentinel
    good = case.launch(anet_ctx)
    d = case.device()
    d["T"][2, 1] = 0.0
    bad = case.launch(anet_ctx, d=d, fill=5.0)
    for g, t in zip(good, bad):
        assert torch.isnan(t[..., 1]).all() and torch.isfinite(t[..., [0, 2]]).all()
        assert torch.equal(g[..., [0, 2]], t[..., [0, 2]]) and (t[..., B:] == 5.0).all()
    # a non-finite sample position of trajectory 2
    d = case.device()
    d["co"][5, 2] = float("inf")
    out = case.launch(anet_ctx, d=d)
    for g, t in zip(good, out):
        assert torch.isnan(t[..., 2]).all() and torch.equal(g[..., [0, 1]], t[..., [0, 1]])
    # the all-blocked map: d = -inf, NaN everywhere
    full = _transform(anet_ctx, np.ones(case.f.size, np.uint8), 1)
    out = case.launch(anet_ctx, field=(case.f.grid, full))
    assert all(torch.isnan(t[..., :B]).all() for t in out)


# ---------------------------------------------------------------------------------------------
# composed
# ---------------------------------------------------------------------------------------------
def _walks(rng, f, B, N, c):
    """Rest-to-rest random walks of about 0.8 m steps, reflected into the map's interior."""
    lo, hi = f.lo + 0.5, f.hi - 0.5
    pts = np.empty((B, N + 1, 3))
    pts[:, 0] = rng.uniform(lo, hi, (B, 3))
    for i in range(N):
        p = pts[:, i] + rng.normal(size=(B, 3)) * 0.5
        p = lo + np.abs(p - lo)
        pts[:, i + 1] = hi - np.abs(hi - p)
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 1.0 + 0.5
    return head, tail, pts[:, 1:-1].copy(), T


def test_minco_obstacle_cost_grad_finite_differences(anet_ctx):
    """s = 4, N = 6, B = 8: the cost is minco_cost_grad + the restatement within 1e-9 relative; gradP and gradT against central
    differences of the returned cost, h = 1e-6, bar 2e-5.  The seed is the first from 77 for which, on the restatement alone, the term
    is active on 10-90 % of the samples and no sample lies within 1e-4 voxel of a lattice plane."""
    import allocnet_amd as aa
    s, N, B, res = 4, 6, 8, 7
    f = Field.get(anet_ctx)
    for seed in range(77, 177):
        head, tail, wps, T = _walks(np.random.default_rng(seed), f, B, N, 3)
        co, _ = aa.minco_solve(head, tail, wps, T, s, ctx=anet_ctx)
        d, off = dn.all_d(co, T, res, **f.kw)
        clearance, mu, frac = dn.limits_from(d)
        if off >= 1e-4 and 0.1 <= frac <= 0.9 and mu > 0.0:
            break
    else:
        raise AssertionError("no seed meets the two conditions")
    print(f"seed {seed}: active on {100 * frac:.1f} %, nearest lattice plane {off:.3e} voxel; clearance {clearance:.4f} m, mu {mu:.4f} m")
    kw = dict(res=res, w=25.0, mu=mu, clearance=clearance, **f.kw)
    open_ = aa.make_obstacle_penalty(w=25.0, smooth_mu=mu, clearance=clearance, res=res)
    pen = aa.make_penalty(rho=2.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=9)
    field = (f.grid, f.d_sd2)
    fn = lambda w, t: aa.minco_obstacle_cost_grad(head, tail, w, t, s, field, open_, penalty=pen, ctx=anet_ctx)
    cost, gP, gT = fn(wps, T)
    base = aa.minco_cost_grad(head, tail, wps, T, s, penalty=pen, ctx=anet_ctx)[0]
    jo = dn.j_obs(co, T, **kw)
    assert (jo > 0.0).any()
    rel = np.abs(cost - (base + jo)) / np.abs(base + jo)
    print(f"cost against minco_cost_grad + J_obs: worst relative {rel.max():.3e} (bar 1e-9)")
    assert rel.max() <= 1e-9
    h = 1e-6

    def check(what, fd, g):
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        print(f"{what}: {err:.3e} (bar 2e-5)")
        assert err <= 2e-5
    for (k, ax) in [(0, 0), (2, 1), (4, 2)]:
        wp, wm = wps.copy(), wps.copy()
        wp[:, k, ax] += h
        wm[:, k, ax] -= h
        check(f"gradP[{k},{ax}]", (fn(wp, T)[0] - fn(wm, T)[0]) / (2 * h), gP[:, k, ax])
    for i in (0, 3, 5):
        tp, tm = T.copy(), T.copy()
        tp[:, i] += h
        tm[:, i] -= h
        check(f"gradT[{i}]", (fn(wps, tp)[0] - fn(wps, tm)[0]) / (2 * h), gT[:, i])


def test_lockstep_lbfgs_leaves_a_block(anet_ctx):
    """A straight 4-piece jerk trajectory flies through a 3 x 3 x 3-voxel block in the middle of a 40 x 24 x 12 map: lbfgs_optimize_dev
    on obstacle_objective_dev.  Every status is >= 0; the composed cost and its J_obs share end below the start.  The first
    collision before and after is printed, not asserted (the energy may trade against the penalty)."""
    import allocnet_amd as aa
    s, c, N, B, res = 3, 3, 4, 1, 20
    size, origin, scale = (40, 24, 12), (0.0, 0.0, 0.0), 0.25
    vm = aa.VoxelMap(size, origin, scale, ctx=anet_ctx)
    block = np.stack(np.meshgrid(np.arange(19, 22), np.arange(11, 14), np.arange(5, 8), indexing="ij"), -1).reshape(-1, 3)
    vm.setOccupied(block.astype(np.int32))
    assert int((vm.distance_field() < 0).sum()) == 27
    frac = np.linspace(0.0, 1.0, N + 1)[None, :, None]
    ends = np.array([[[1.0, 3.07, 1.55], [9.0, 3.07, 1.55]]])            # a little off the block's axis: the symmetry is broken
    pts = ends[:, :1] * (1.0 - frac) + ends[:, 1:] * frac
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    wps, T = pts[:, 1:-1], np.full((B, N), 1.5)
    open_ = aa.make_obstacle_penalty(w=200.0, smooth_mu=0.05, clearance=0.5, res=res)
    pen = aa.make_penalty(rho=5.0, res=res)
    sd2 = dn.unflat(vm.distance_field().cpu().numpy(), size)
    kw = dict(res=res, w=200.0, mu=0.05, clearance=0.5, sd2=sd2, size=size, origin=origin, scale=scale)

    def state(w, t):
        co, _ = aa.minco_solve(head, tail, w, t, s, ctx=anet_ctx)
        jo = dn.j_obs(co, t, **kw)
        base = aa.minco_cost_grad(head, tail, w, t, s, penalty=pen, ctx=anet_ctx)[0]
        return (base + jo).sum(), jo.sum(), aa.traj_first_collision(co, t, vm, ctx=anet_ctx)
    j0, o0, hit0 = state(wps, T)
    assert o0 > 0.0
    ld = 1
    nw = 3 * (N - 1)
    x = torch.zeros(nw + N, ld, dtype=torch.float64, device=DEV)
    x[:nw, :B] = torch.from_numpy(wps.reshape(B, -1)).T.to(DEV)
    x[nw:, :B] = torch.from_numpy(np.log(T)).T.to(DEV)
    ev = aa.obstacle_objective_dev(_bm(head.reshape(B, -1), ld), _bm(tail.reshape(B, -1), ld), s, c, N, B, vm, open_, penalty=pen,
                                   ctx=anet_ctx)
    res_ = aa.lbfgs_optimize_dev(x, ev, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-4), max_evals=600, ctx=anet_ctx)
    torch.cuda.synchronize()
    status = res_["status"].cpu().numpy()
    print(f"status {status.tolist()}, evals {res_['evals'].cpu().numpy().tolist()}")
    assert (status >= 0).all()
    w = x[:nw, :B].T.cpu().numpy().reshape(B, N - 1, 3)
    t = np.exp(x[nw:, :B].T.cpu().numpy())
    j1, o1, hit1 = state(w, t)
    print(f"J {j0:.6g} -> {j1:.6g}, J_obs {o0:.6g} -> {o1:.6g}; first collision t {hit0[0].tolist()} voxel {hit0[2].tolist()} -> "
          f"t {hit1[0].tolist()} voxel {hit1[2].tolist()}")
    assert j1 < j0 and o1 < o0
