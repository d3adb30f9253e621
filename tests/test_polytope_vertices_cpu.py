"""Vertex enumeration without a GPU: the restatement the GPU tests compare against (tests/polytope_np.py) is checked against facts
that do not depend on it; the new entry points are declared, exported and bound; the C++ program compiles as C++14; the kernel uses
no scratch memory; and without a device the entry point fails loudly."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
from scipy.optimize import linprog

from tests import polytope_np as pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["anet_polytope_vertices", "anet_polytope_vertices_dev"]


@pytest.mark.parametrize("name, count", [("cube", 8), ("tetrahedron", 4), ("octahedron", 6), ("dressed_cube", 8), ("cone", 41)])
def test_restatement_known_solids(name, count):
    h = getattr(pnp, name)()
    vq = pnp.vertices_qhull(h)
    ve, min_det = pnp.enumerate_triples(h)
    assert len(vq) == count and len(ve) == count
    assert pnp.hausdorff(vq, ve) <= 1e-12
    assert min_det >= 1e-3


def test_restatement_vertices_are_feasible_and_tight_on_three_rows():
    polys = [pnp.cube(), pnp.octahedron(), pnp.cone((37.0, -41.0, 3.0)), pnp.sphere_tangents(50, 5)] + list(pnp.corridor_polytopes()[:16])
    for h in polys:
        n, d, _ = pnp.unit_rows(h)
        for verts in (pnp.vertices_qhull(h), pnp.enumerate_triples(h)[0]):
            r = verts @ n.T + d
            assert r.max() <= 1e-9
            assert ((np.abs(r) <= 1e-9).sum(1) >= 3).all()


def test_restatement_support_function_is_the_linear_programme():
    """max u.v over the vertices equals max u.x over the polytope (HiGHS) for 20 random directions."""
    rng = np.random.default_rng(3)
    for h in [pnp.cone(), pnp.sphere_tangents(64, 6)] + list(pnp.corridor_polytopes()[:8]):
        n, d, _ = pnp.unit_rows(h)
        for verts in (pnp.vertices_qhull(h), pnp.enumerate_triples(h)[0]):
            for u in rng.normal(size=(20, 3)):
                res = linprog(-u, A_ub=n, b_ub=-d, bounds=[(None, None)] * 3, method="highs")
                assert res.status == 0
                assert abs((verts @ u).max() + res.fun) <= 1e-9 * max(1.0, abs(res.fun))


def test_restatement_statuses():
    assert pnp.vertices_qhull(np.array([[1.0, 0.0, 0.0, 1.0], [-1.0, 0.0, 0.0, 1.0]])) is None          # x <= -1, x >= 1
    assert pnp.vertices_qhull(np.zeros((4, 4))) is None
    slab = np.array([[1.0, 0.0, 0.0, -1.0], [-1.0, 0.0, 0.0, -1.0]])
    assert pnp.interior(slab)[0] == 1.0 and not pnp.bounded(slab) and pnp.vertices_qhull(slab) is None
    assert len(pnp.enumerate_triples(slab)[0]) == 0                                                     # it has no vertex
    assert pnp.interior(slab[:1])[0] == np.inf                                                          # a half-space
    flat = np.vstack([pnp.box([-1.0] * 3, [1.0] * 3), [[1.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0]]])
    assert pnp.vertices_qhull(flat) is None


def _declared():
    txt = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(anet_[A-Za-z0-9_]+)\s*\(", txt))


def test_entry_points_are_declared_exported_and_bound():
    import allocnet_amd as aa
    from allocnet_amd import _lib, build
    declared = _declared()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared in the header"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.PROTOTYPES, f"{n} is not in the ctypes table"
    assert "api_polytope.hip" in build.SOURCES
    for n in ("polytope_vertices", "polytope_vertices_dev", "enumerate_vs", "polytope_faces", "polytope_volume", "corridor_vertices"):
        assert callable(getattr(aa, n))


def test_no_cpu_result_without_a_device():
    import allocnet_amd as aa
    from allocnet_amd import _lib
    if _lib.load().anet_device_count() != 0:
        ok, v = aa.enumerate_vs(pnp.cube())
        assert ok and len(v) == 8                                            # (a GPU box: the product path answers)
        return
    with pytest.raises(aa.AnetError) as ei:
        aa.enumerate_vs(pnp.cube())
    assert ei.value.code == _lib.ANET_ERR_NODEVICE


def test_faces_and_volume_from_the_restatements_masks():
    """polytope_faces / polytope_volume are host code over (vertices, masks): fed with the restatement's they give the cube's
    six quadrilaterals, Euler's formula and ConvexHull's volume."""
    import allocnet_amd as aa
    from scipy.spatial import ConvexHull
    h = pnp.dressed_cube()
    v = pnp.enumerate_triples(h)[0]
    act = pnp.active_rows(h, v)
    faces = aa.polytope_faces(h, v, act)
    assert sorted(faces) == [0, 1, 2, 3, 4, 5, 6, 7] and all(len(f) == 4 for f in faces.values())
    assert abs(aa.polytope_volume(h, v, act) - 8.0) <= 1e-14
    for r, f in faces.items():                                               # counter-clockwise about the outward normal
        p = v[f]
        assert np.cross(p[1] - p[0], p[2] - p[1]) @ h[r, :3] > 0.0
    for h in pnp.corridor_polytopes()[:32]:
        v = pnp.enumerate_triples(h)[0]
        act = pnp.active_rows(h, v)
        faces = aa.polytope_faces(h, v, act)
        edges = {frozenset((f[i], f[(i + 1) % len(f)])) for f in faces.values() for i in range(len(f))}
        assert len(v) - len(edges) + len(faces) == 2
        vol = ConvexHull(v).volume
        assert abs(aa.polytope_volume(h, v, act) - vol) <= 1e-9 * vol


def test_cpp_vertices_program_compiles_as_cxx14():
    src = os.path.join(ROOT, "tests", "cpp", "test_geo_vertices.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_vertex_kernel_uses_no_scratch_memory():
    """The new unit compiled for gfx950 with the product's flags: both launch shapes of k_polytope_vertices keep their state in
    registers and LDS (the figures are recorded in DESIGN.md 8h and printed here)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_polytope.hip"), "-o", os.path.join(td, "u.o")],
                             capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    usage, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    kernels = {fn: u for fn, u in usage.items() if "k_polytope_vertices" in fn}
    assert len(kernels) == 2, list(usage)
    for fn, u in kernels.items():
        print(fn, u)
        assert u["ScratchSize"] == 0, (fn, u)
