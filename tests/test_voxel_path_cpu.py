"""CPU suite of the path search: the numpy restatement (tests/voxel_path_np.py) on hand-made grids with known answers, the
ctypes table, and sfc_gen::planPath through the C++ headers at the reference's language level."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests.voxel_path_np import PathNP, make_map, EXACT, APPROXIMATE, INVALID_START, INF32, MOVES, weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute_field(p, start):
    """Bellman-Ford on the same graph, written from the definition (slow, tiny grids only)"""
    sv = p.free_voxel(start)
    d = np.full(p.n, np.iinfo(np.int64).max, dtype=np.int64)
    d[sv] = 0
    changed = True
    while changed:
        changed = False
        for i in range(p.n):
            x, y, z = p.xyz(i)
            if not p.is_free(x, y, z):
                continue
            for mv in MOVES:
                nx, ny, nz = x + mv[0], y + mv[1], z + mv[2]
                if p.is_free(nx, ny, nz) and p.edge(x, y, z, mv):
                    j = nx + p.sx * (ny + p.sy * nz)
                    if d[j] != np.iinfo(np.int64).max and d[j] + weight(mv) < d[i]:
                        d[i] = d[j] + weight(mv); changed = True
    return np.where(d == np.iinfo(np.int64).max, INF32, d).astype(np.uint32)


def test_empty_box_is_one_segment():
    m = make_map((12, 9, 5), (-1.0, 2.0, 0.5), 0.25)
    p = PathNP(m)
    s, g = np.array([-0.9, 2.1, 0.6]), np.array([1.8, 4.1, 1.6])
    cost, path, st = p.plan(s, g)
    assert st == EXACT
    assert path.tobytes() == np.array([s, g]).tobytes()
    assert cost == pytest.approx(np.linalg.norm(g - s), rel=1e-15)


def test_field_matches_bellman_ford_on_a_random_grid():
    rng = np.random.default_rng(3)
    m = make_map((7, 6, 4), (0.0, 0.0, 0.0), 1.0)
    m.vox[:] = (rng.uniform(size=m.vox.size) < 0.25).astype(np.uint8)
    m.vox[0] = 0
    p = PathNP(m)
    f = p.fields([[0.5, 0.5, 0.5]])[0]
    assert np.array_equal(f, _brute_field(p, [0.5, 0.5, 0.5]))


def test_wall_with_one_hole_routes_through_the_hole():
    occ = [(5, y, z) for y in range(9) for z in range(3) if (y, z) != (7, 1)]
    m = make_map((11, 9, 3), (0.0, 0.0, 0.0), 1.0, occ)
    p = PathNP(m)
    s, g = np.array([1.5, 1.5, 1.5]), np.array([9.5, 1.5, 1.5])
    cost, path, st = p.plan(s, g)
    assert st == EXACT
    assert path[0].tobytes() == s.tobytes() and path[-1].tobytes() == g.tobytes()
    assert cost > np.linalg.norm(g - s) + 1.0
    # every segment stays in free voxels, and one of them goes through the hole
    through = False
    for a, b in zip(path[:-1], path[1:]):
        q = a + np.linspace(0.0, 1.0, 400)[:, None] * (b - a)
        assert not m.query(q).any()
        through |= bool((np.floor(q).astype(int) == [5, 7, 1]).all(axis=1).any())
    assert through


def test_voxels_touching_along_an_edge_block_the_diagonal():
    # (1, 0) and (0, 1) occupied: the start voxel (0, 0) has no edge to (1, 1), so it is a pocket of one voxel
    m = make_map((3, 3, 1), (0.0, 0.0, 0.0), 1.0, [(1, 0, 0), (0, 1, 0)])
    p = PathNP(m)
    f = p.fields([[0.5, 0.5, 0.5]])[0]
    assert f[0] == 0 and (f[1:] == INF32).all()
    cost, path, st = p.plan([0.5, 0.5, 0.5], [1.5, 1.5, 0.5])
    assert st == APPROXIMATE and cost == 0.0
    assert path.tolist() == [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]
    # with one of them free, the detour is two face moves and then the diagonal shortcut is visible
    m.vox[1] = 0
    cost, path, st = PathNP(m).plan([0.5, 0.5, 0.5], [1.5, 1.5, 0.5])
    assert st == EXACT
    assert path.tolist() == [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [1.5, 1.5, 0.5]]


def test_sealed_pocket_start_ends_at_the_nearest_reached_centre():
    occ = [(x, y, z) for x in range(1, 6) for y in range(1, 6) for z in range(1, 6)
           if max(abs(x - 3), abs(y - 3), abs(z - 3)) == 2]
    m = make_map((9, 7, 7), (0.0, 0.0, 0.0), 1.0, occ)
    p = PathNP(m)
    cost, path, st = p.plan([3.5, 3.5, 3.5], [8.5, 3.5, 3.5])
    assert st == APPROXIMATE
    assert path[-1].tolist() == [4.5, 3.5, 3.5]
    assert cost == 1.0
    # and the other way round: a goal in the sealed room
    cost, path, st = p.plan([8.5, 3.5, 3.5], [3.5, 3.5, 3.5])
    assert st == APPROXIMATE
    assert path[-1].tolist() == [3.5, 3.5, 0.5]   # six centres at squared distance 9: the lowest id wins


def test_invalid_start_and_the_box():
    m = make_map((6, 6, 3), (0.0, 0.0, 0.0), 1.0, [(2, 2, 1)])
    p = PathNP(m)
    assert p.plan([2.5, 2.5, 1.5], [5.5, 5.5, 1.5])[2] == INVALID_START
    assert p.plan([-1.5, 2.5, 1.5], [5.5, 5.5, 1.5])[2] == INVALID_START
    assert p.plan([-0.5, 2.5, 1.5], [5.5, 5.5, 1.5])[2] == EXACT   # truncation toward zero: voxel 0, as query() does
    c, path, st = p.plan([2.5, 2.5, 1.5], [5.5, 5.5, 1.5])
    assert math.isinf(c) and path.shape == (0, 3)
    # a sub-box: voxels whose centre lies outside [lb, hb] are not free, the goal beyond it is approximated
    q = PathNP(m, lb=[0.0, 0.0, 0.0], hb=[3.6, 6.0, 3.0])
    c, path, st = q.plan([0.5, 0.5, 0.5], [5.5, 0.5, 0.5])
    assert st == APPROXIMATE and path[-1].tolist() == [3.5, 0.5, 0.5]


def test_same_voxel_and_same_point():
    m = make_map((4, 4, 4), (0.0, 0.0, 0.0), 1.0)
    p = PathNP(m)
    c, path, st = p.plan([1.2, 1.3, 1.4], [1.7, 1.6, 1.5])
    assert st == EXACT and path.tolist() == [[1.2, 1.3, 1.4], [1.7, 1.6, 1.5]]
    c, path, st = p.plan([1.2, 1.3, 1.4], [1.2, 1.3, 1.4])
    assert st == EXACT and c == 0.0 and len(path) == 2


def test_lib_table_has_the_path_entries():
    from allocnet_amd import _lib
    for n in ("anet_voxel_path_workspace", "anet_voxel_path_field_dev", "anet_voxel_path_field_ptr",
              "anet_voxel_path_extract_dev"):
        assert n in _lib.PROTOTYPES
    import allocnet_amd as aa
    assert (aa.PATH_EXACT, aa.PATH_APPROXIMATE, aa.PATH_INVALID_START) == (0, 1, 2)
    assert callable(aa.plan_path) and callable(aa.plan_paths) and hasattr(aa.VoxelMap, "path_field_dev")


def test_workspace_refuses_grids_past_the_weight_bound():
    import ctypes
    from allocnet_amd import _lib
    lib = _lib.load()
    g = _lib.VoxelGrid()
    for c, v in enumerate((400, 400, 50)):
        g.size[c] = v
    g.scale = 0.1
    assert lib.anet_voxel_path_workspace(ctypes.byref(g), 1) > 4 * 8_000_000
    assert lib.anet_voxel_path_workspace(ctypes.byref(g), 0) == -1
    for c, v in enumerate((1024, 1024, 256)):   # 17 * 2^28 > 2^32
        g.size[c] = v
    assert lib.anet_voxel_path_workspace(ctypes.byref(g), 1) == -1


# learning_planner.hpp's call, with an Eigen-like column for the start and goal and the map's own vectors for the box
PLAN_PATH_CALL = """
#include <vector>
#include "allocnet_amd/sfc_gen_map.hpp"
#include "allocnet_amd/voxel_map.hpp"
struct V3 {
  double v[3] = {0.0, 0.0, 0.0};
  V3() = default;
  V3(double x, double y, double z) : v{x, y, z} {}
  double operator()(int i) const { return v[i]; }
};
struct Col {  // an expression like iniState.col(0)
  const double *p;
  double operator()(int i) const { return p[i]; }
};
struct V3i {
  int v[3];
  int operator()(int i) const { return v[i]; }
};
double plan(voxel_map::VoxelMap &mapPtr, const double *ini, const double *fin, std::vector<V3> &route) {
  if (route.size() <= 0) {
    return sfc_gen::planPath(Col{ini}, Col{fin}, mapPtr.getOrigin(), mapPtr.getCorner(), &mapPtr, 0.01, route);
  }
  const V3 s(0.0, 0.0, 0.0), g(1.0, 1.0, 1.0);
  return sfc_gen::planPath<V3>(s, g, s, g, &mapPtr, 0.01, route);
}
int main() {
  voxel_map::VoxelMap m(V3i{{4, 4, 4}}, V3(0.0, 0.0, 0.0), 1.0);
  std::vector<V3> route;
  const double a[3] = {0.5, 0.5, 0.5}, b[3] = {3.5, 3.5, 3.5};
  return plan(m, a, b, route) > 0.0 ? 0 : 1;
}
"""


def test_plan_path_compiles_as_cxx14(tmp_path):
    src = tmp_path / "plan_path_call.cpp"
    src.write_text(PLAN_PATH_CALL)
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                          "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
