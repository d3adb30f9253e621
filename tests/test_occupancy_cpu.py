"""CPU suite of the occupancy grid's restatement (tests/occupancy_np.py): the walk against exact rational geometry, the documented
tie cases, degenerate and truncated rays, the update rule, and the C++ header at the reference's language level.  The GPU suite
(tests/test_occupancy_gpu.py) holds the device to this restatement bit for bit, so this file is what pins the rules themselves."""
import itertools
import math
import os
import subprocess
from fractions import Fraction as F

import numpy as np

from tests import occupancy_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, ORIGIN, SCALE = (12, 9, 7), (-1.3, 0.7, -0.25), 0.1


def _exact_cells(o, q, origin, scale):
    """The cells whose OPEN box the segment o -> q crosses, in exact rational arithmetic on the doubles given."""
    o = [F(float(x)) for x in o]; q = [F(float(x)) for x in q]; og = [F(float(x)) for x in origin]; s = F(float(scale))
    lo = [math.floor((min(o[c], q[c]) - og[c]) / s) for c in range(3)]
    hi = [math.floor((max(o[c], q[c]) - og[c]) / s) for c in range(3)]
    out = set()
    for cell in itertools.product(*[range(lo[c], hi[c] + 1) for c in range(3)]):
        t0, t1, ok = F(0), F(1), True
        for c in range(3):
            a = og[c] + cell[c] * s; b = a + s; d = q[c] - o[c]
            if d == 0:
                if not (a < o[c] < b):
                    ok = False
                    break
            else:
                ta, tb = (a - o[c]) / d, (b - o[c]) / d
                if ta > tb:
                    ta, tb = tb, ta
                t0, t1 = max(t0, ta), min(t1, tb)
        if ok and t0 < t1:
            out.add(cell)
    return out


def _near_degenerate(o, q, origin, scale):
    """True when two crossing parameters lie within 1e-9 of each other, or an endpoint within 1e-9 * scale of a cell face."""
    o = [F(float(x)) for x in o]; q = [F(float(x)) for x in q]; og = [F(float(x)) for x in origin]; s = F(float(scale))
    tol = F(1, 10 ** 9)
    for p in (o, q):
        for c in range(3):
            r = (p[c] - og[c]) / s
            if min(r - math.floor(r), math.ceil(r) - r) < tol:      # (in units of scale)
                return True
    ts = []
    for c in range(3):
        d = q[c] - o[c]
        if d == 0:
            continue
        k0, k1 = sorted((math.floor((o[c] - og[c]) / s), math.floor((q[c] - og[c]) / s)))
        ts += [(og[c] + k * s - o[c]) / d for k in range(k0 + 1, k1 + 1)]
    ts.sort()
    return any(b - a < tol for a, b in zip(ts, ts[1:]))


def test_walk_equals_exact_geometry():
    rng = np.random.default_rng(11)
    origin = np.asarray(ORIGIN); ext = np.asarray(SIZE) * SCALE
    left_out = 0
    for _ in range(100):
        o = origin + rng.uniform(-0.2, 1.2, 3) * ext
        q = origin + rng.uniform(-0.2, 1.2, 3) * ext
        if _near_degenerate(o, q, ORIGIN, SCALE):
            left_out += 1
            continue
        cells = onp.walk_cells(o, q, ORIGIN, SCALE)
        assert len(set(cells)) == len(cells), "a cell visited twice"
        assert set(cells) == _exact_cells(o, q, ORIGIN, SCALE)
        first, _ = onp.cells_of(o, origin, SCALE); last, _ = onp.cells_of(q, origin, SCALE)
        assert cells[0] == tuple(first[0]) and cells[-1] == tuple(last[0])
    assert left_out <= 1, left_out


def test_ties_step_together():
    # centre to centre along (1, 1, 1): exactly the diagonal cells
    cells = onp.walk_cells((2.5, 3.5, 1.5), (7.5, 8.5, 6.5), (0.0, 0.0, 0.0), 1.0)
    assert cells == [(2 + k, 3 + k, 1 + k) for k in range(6)]
    cells = onp.walk_cells(np.asarray(ORIGIN) + np.array([2.5, 3.5, 1.5]) * SCALE, np.asarray(ORIGIN) + np.array([6.5, 7.5, 5.5]) * SCALE,
                           ORIGIN, SCALE)
    assert cells == [(2 + k, 3 + k, 1 + k) for k in range(5)]
    # centre to centre along (3, 1, 0): x at t = 1/6; x and y together at t = 1/2 (only the diagonal cell (2, 1, 0), neither
    # (2, 0, 0) nor (1, 1, 0)); x at t = 5/6
    cells = onp.walk_cells((0.5, 0.5, 0.5), (3.5, 1.5, 0.5), (0.0, 0.0, 0.0), 1.0)
    assert cells == [(0, 0, 0), (1, 0, 0), (2, 1, 0), (3, 1, 0)]
    # and backwards
    cells = onp.walk_cells((3.5, 1.5, 0.5), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0)
    assert cells == [(3, 1, 0), (2, 1, 0), (1, 0, 0), (0, 0, 0)]
    # axis-parallel, through cells outside the map (negative indices: floor, not truncation)
    cells = onp.walk_cells((-1.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0)
    assert cells == [(-2, 0, 0), (-1, 0, 0), (0, 0, 0), (1, 0, 0)]


def _idx(cell, size=SIZE):
    return cell[0] + size[0] * (cell[1] + size[1] * cell[2])


def test_zero_length_rays():
    o = np.asarray(ORIGIN) + np.array([4.5, 3.5, 2.5]) * SCALE
    hit, miss = onp.scan_marks(SIZE, ORIGIN, SCALE, onp.Params(min_range=0.0), o, o[None, :])
    assert hit.sum() == 1 and hit[_idx((4, 3, 2))] and not miss.any()
    hit, miss = onp.scan_marks(SIZE, ORIGIN, SCALE, onp.Params(min_range=0.05), o, o[None, :])
    assert not hit.any() and not miss.any()


def test_truncated_ray_only_carves():
    prm = onp.Params(max_range=0.3)
    o = np.asarray(ORIGIN) + np.array([1.5, 1.5, 1.5]) * SCALE
    d = np.array([0.6, 0.0, 0.0]) * 1.0                              # twice max_range along x
    p = o + d
    ln = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    assert ln > prm.max_range
    r = prm.max_range / ln
    end, _ = onp.cells_of((o + d * r)[None, :], np.asarray(ORIGIN), SCALE)
    hit, miss = onp.scan_marks(SIZE, ORIGIN, SCALE, prm, o, p[None, :])
    assert not hit.any()
    assert miss[_idx(tuple(end[0]))]
    want = {_idx(c) for c in onp.walk_cells(o, o + d * r, ORIGIN, SCALE)}
    assert set(np.flatnonzero(miss)) == want and tuple(end[0]) == (4, 1, 1)
    # the same return inside the range is a hit at its own cell
    hit, miss = onp.scan_marks(SIZE, ORIGIN, SCALE, onp.Params(max_range=1.0), o, p[None, :])
    assert list(np.flatnonzero(hit)) == [_idx((7, 1, 1))] and miss.sum() == 6


def test_update_rule():
    prm = onp.Params(hit=800, miss=-300, lo=-700, hi=1500, max_range=5.0)
    n = int(np.prod(SIZE))
    o = np.asarray(ORIGIN) + np.array([0.5, 0.5, 0.5]) * SCALE
    a = np.asarray(ORIGIN) + np.array([5.5, 0.5, 0.5]) * SCALE       # a return in cell (5, 0, 0)
    b = np.asarray(ORIGIN) + np.array([9.5, 0.5, 0.5]) * SCALE       # a return behind it: its ray passes through (5, 0, 0)
    L = np.full(n, onp.UNKNOWN, dtype=np.int16)
    # hit wins over misses within a scan, duplicates change nothing, UNKNOWN counts as 0 before the first increment
    onp.integrate(L, SIZE, ORIGIN, SCALE, prm, o, np.stack([b, a, b, a, a, b, b]))
    assert L[_idx((5, 0, 0))] == 800 and L[_idx((9, 0, 0))] == 800
    assert all(L[_idx((x, 0, 0))] == -300 for x in (0, 1, 2, 3, 4, 6, 7, 8))
    assert (L != onp.UNKNOWN).sum() == 10
    # both clamps, and revision: (5, 0, 0) seen through until it is free again
    onp.integrate(L, SIZE, ORIGIN, SCALE, prm, o, a[None, :])
    assert L[_idx((5, 0, 0))] == 1500 and L[_idx((4, 0, 0))] == -600
    onp.integrate(L, SIZE, ORIGIN, SCALE, prm, o, a[None, :])
    assert L[_idx((5, 0, 0))] == 1500 and L[_idx((4, 0, 0))] == -700
    for k in range(8):
        onp.integrate(L, SIZE, ORIGIN, SCALE, prm, o, b[None, :])
    assert L[_idx((5, 0, 0))] == -700 and L[_idx((9, 0, 0))] == 1500
    # UNKNOWN is never produced by an update, whatever the clamps
    ext = onp.Params(hit=32767, miss=-32767, lo=-32767, hi=32767, max_range=5.0)
    L2 = np.full(n, onp.UNKNOWN, dtype=np.int16)
    for _ in range(3):
        onp.integrate(L2, SIZE, ORIGIN, SCALE, ext, o, b[None, :])
    touched = [_idx((x, 0, 0)) for x in range(10)]
    assert (L2[touched] != onp.UNKNOWN).all() and L2[_idx((0, 0, 0))] == -32767 and L2[_idx((9, 0, 0))] == 32767
    assert (np.delete(L2, touched) == onp.UNKNOWN).all()
    # the hand-over
    v = onp.to_voxels(L, 0, True)
    assert v[_idx((9, 0, 0))] == 1 and v[_idx((5, 0, 0))] == 0 and v[_idx((0, 1, 0))] == 1
    assert onp.to_voxels(L, 0, False)[_idx((0, 1, 0))] == 0 and onp.to_voxels(L, -700, False)[_idx((5, 0, 0))] == 1


def test_first_hit_restatement():
    vox = np.zeros(int(np.prod(SIZE)), dtype=np.uint8)
    vox[_idx((5, 0, 0))] = 1
    og = np.asarray(ORIGIN)
    o = og + np.array([[0.5, 0.5, 0.5], [5.5, 0.5, 0.5], [0.5, 1.5, 0.5], [-3.5, 0.5, 0.5], [np.nan, 0, 0]]) * SCALE
    q = og + np.array([[9.5, 0.5, 0.5], [9.5, 0.5, 0.5], [9.5, 1.5, 0.5], [-1.5, 0.5, 0.5], [1, 1, 1]]) * SCALE
    voxel, t = onp.raycast(vox, SIZE, ORIGIN, SCALE, o, q)
    assert list(voxel) == [_idx((5, 0, 0)), _idx((5, 0, 0)), onp.HIT_FREE, onp.HIT_FREE, onp.HIT_INVALID]
    assert abs(t[0] - 0.5) < 1e-12 and t[1] == 0.0 and t[2] == 1.0 and t[3] == 1.0 and np.isnan(t[4])


def test_cpp_occupancy_header_compiles_as_cxx14():
    src = os.path.join(ROOT, "tests", "cpp", "test_occupancy.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                          "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
