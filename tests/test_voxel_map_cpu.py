"""CPU suite of the voxel map: the numpy restatement (tests/voxel_np.py) against a brute-force Chebyshev-distance layer,
the reference's blocking and no-op behaviours, the truncation of the fill, and the C++ header's language level."""
import os
import subprocess

import numpy as np
import pytest

from tests.voxel_np import VoxelMapNP, chebyshev_layers, DILATED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape,r,density", [((7, 5, 4), 1, 0.05), ((9, 6, 5), 2, 0.03), ((6, 6, 6), 3, 0.01),
                                             ((11, 3, 2), 5, 0.1), ((4, 4, 4), 9, 0.02), ((5, 7, 3), 2, 0.0)])
def test_frontier_rounds_match_chebyshev_on_01_grids(shape, r, density):
    rng = np.random.default_rng(hash((shape, r)) & 0xffff)
    m = VoxelMapNP(shape, (0.0, 0.0, 0.0), 1.0)
    g = (rng.uniform(size=shape[::-1]) < density).astype(np.uint8)
    m.vox[:] = g.reshape(-1)
    m.dilate(r)
    want, surf = chebyshev_layers(g, r)
    assert np.array_equal(m.vox, want.reshape(-1))
    assert np.array_equal(m.surf, surf)


def test_second_dilate_is_blocked_by_the_first():
    m = VoxelMapNP((8, 8, 8), (0.0, 0.0, 0.0), 0.5)
    m.vox[m.step @ np.array([4, 4, 4])] = 1
    m.dilate(1)
    assert len(m.surf) == 26
    before = m.vox.copy()
    m.dilate(1)   # round 1 grows from the 1s only, and their neighbours are all 2 now
    assert len(m.surf) == 0
    assert np.array_equal(m.vox, before)


def test_dilated_voxels_are_not_sources_and_block():
    """Not a distance transform once 2s are present: the 2s of an earlier call neither grow nor let growth through."""
    m = VoxelMapNP((9, 1, 1), (0.0, 0.0, 0.0), 1.0)
    m.vox[:] = [0, 0, 2, 1, 0, 0, 0, 0, 0]
    m.dilate(3)
    assert list(m.vox) == [0, 0, 2, 1, 2, 2, 2, 0, 0]
    assert list(m.surf) == [6]


def test_r0_keeps_the_old_surface():
    m = VoxelMapNP((6, 6, 6), (0.0, 0.0, 0.0), 1.0)
    m.set_occupied([[2.5, 2.5, 2.5]])
    m.dilate(2)
    surf = m.surf.copy()
    m.set_occupied([[0.5, 0.5, 0.5]])
    m.dilate(0)
    m.dilate(-3)
    assert np.array_equal(m.surf, surf)
    assert m.vox[0] == 1


def test_fill_truncates_toward_zero():
    o = np.array([1.0, -2.0, 0.25]); s = 0.1
    m = VoxelMapNP((4, 4, 4), o, s)
    m.set_occupied([o - 0.5 * s])                 # (pos - o) / scale = -0.5: truncates to 0
    assert m.vox[0] == 1 and m.vox.sum() == 1
    m.set_occupied([o - 1.5 * s, o + 4 * s + 1e-9])   # -1.5 -> -1 and exactly past the upper face: dropped
    assert m.vox.sum() == 1
    assert list(m.query([o - 0.5 * s, o - 1.5 * s, o + 1.5 * s])) == [True, True, False]


def test_surface_coordinates_use_two_roundings():
    m = VoxelMapNP((5, 7, 3), (0.1, -0.3, 0.7), 0.1)
    m.surf = np.arange(m.vox.size)
    p = m.surf_points()
    xyz = m.xyz(m.surf)
    off = (xyz * m.step).astype(np.float64)
    prod = off * m.step_scale
    assert np.array_equal(p, prod + m.oc)
    assert np.allclose(p, xyz * m.scale + m.oc, atol=1e-12)


def test_cloud_records_skip_non_finite():
    m = VoxelMapNP((4, 4, 4), (0.0, 0.0, 0.0), 1.0)
    rec = np.array([[0.5, 0.5, 0.5, 7], [np.nan, 1.5, 1.5, 0], [1.5, np.inf, 1.5, 0], [2.5, 2.5, 2.5, 0]], dtype=np.float32)
    m.set_occupied_cloud(rec)
    assert np.flatnonzero(m.vox).tolist() == [0, 42]
    m.dilate(1)
    assert (m.vox == DILATED).sum() == len(m.surf) > 0


def test_cpp_voxel_map_header_compiles_as_cxx14():
    """include/allocnet_amd/voxel_map.hpp builds with the reference's language level, without Eigen or HIP headers."""
    src = os.path.join(ROOT, "tests", "cpp", "test_voxel_map.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                          "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# A translation unit shaped like the reference's learning_planning.cpp after the documented sfc_gen swap: the reference's
# own voxel_map namespace (declared here from its interface) and then allocnet_amd/sfc_gen.hpp, which must not bring a
# second voxel_map with it.
REFERENCE_SHAPED_MAP = """
#include <cstdint>
#include <vector>
namespace voxel_map {
constexpr uint8_t Unoccupied = 0;
constexpr uint8_t Occupied = 1;
constexpr uint8_t Dilated = 2;
class VoxelMap {
 public:
  VoxelMap() = default;
  std::vector<uint8_t> voxels;
};
}  // namespace voxel_map
#include "allocnet_amd/sfc_gen.hpp"
int main() {
  voxel_map::VoxelMap m;
  return (int)m.voxels.size() + voxel_map::Dilated;
}
"""


def test_sfc_gen_builds_next_to_the_reference_voxel_map(tmp_path):
    src = tmp_path / "ref_shaped_map.cpp"
    src.write_text(REFERENCE_SHAPED_MAP)
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                          "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_index_fill_drops_out_of_bounds():
    m = VoxelMapNP((4, 3, 2), (0.0, 0.0, 0.0), 1.0)
    m.set_occupied_id([[0, 0, 0], [3, 2, 1], [4, 0, 0], [-1, 1, 1], [1, 3, 0], [2, 1, 2]])
    assert np.flatnonzero(m.vox).tolist() == [0, 23]
