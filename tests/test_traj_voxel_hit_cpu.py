"""Exact first collision with the voxel map, without a GPU: the multiprecision reference (tests/traj_voxel_hit_mp.py) against a
dense sampling of itself; a float64 restatement of the kernel's procedure against the reference on every golden case at the
a-priori bound; the node budget's conservative answer; the new unit's resources; the entry points declared, exported and bound;
the C++ header as C++14."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import traj_voxel_hit_mp as hm
from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["anet_traj_voxel_hit", "anet_traj_voxel_hit_dev"]
SIZE, ORIGIN, SCALE = (16, 12, 8), (-2.0, -1.5, 0.0), 0.25


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "traj_voxel_hit_cases.npz"))


def grids_of(fx):
    g = hm.Grid(SIZE, ORIGIN, SCALE)
    n = SIZE[0] * SIZE[1] * SIZE[2]
    return [(g, fx["vox0"]), (g, np.zeros(n, dtype=np.uint8)), (g, fx["vox2"]),
            (hm.Grid((1, 1, 1), (0.0, 0.0, 0.0), 1.0), np.zeros(1, dtype=np.uint8))]


hit_float64 = hm.hit_float64


# ---- the reference against facts that do not depend on it ---------------------------------------------------
def test_reference_straight_line_in_closed_form():
    """p(t) = p0 + v t along +x from the middle of cell (2, 3, 4) of an empty map with the voxel (5, 3, 4) set: q_x = 2.5 + 4 t
    enters it at t = 5/8; without it the map is left at q_x = 16, t = 27/8; along -x at q_x = -1 (not 0), t = 7/8."""
    g = hm.Grid(SIZE, ORIGIN, SCALE)
    vox = np.zeros(16 * 12 * 8, dtype=np.uint8)
    for s in (2, 3, 4):
        cm = np.zeros((3, 2 * s))
        cm[:, -1] = [-2.0 + 2.5 * 0.25, -1.5 + 3.5 * 0.25, 4.5 * 0.25]
        cm[0, -2] = 1.0
        r = hm.piece_hit_mp(cm, 4.0, g, vox)
        assert r["voxel"] == hm.HIT_OUTSIDE and r["axis"] == 0 and r["plane"] == 16 and abs(r["tau"] * 4 - hm.mpmath.mpf(27) / 8) < 1e-50
        assert hm.piece_hit_mp(cm, 3.0, g, vox)["voxel"] == hm.HIT_FREE
        v2 = vox.copy(); v2[5 + 16 * (3 + 12 * 4)] = 2
        r = hm.piece_hit_mp(cm, 4.0, g, v2)
        assert r["voxel"] == 5 + 16 * (3 + 12 * 4) and r["plane"] == 5 and abs(r["tau"] * 4 - hm.mpmath.mpf(5) / 8) < 1e-50
        assert abs(r["dq"] - 16) < 1e-50
        cm[0, -2] = -1.0
        r = hm.piece_hit_mp(cm, 4.0, g, v2)
        assert r["voxel"] == hm.HIT_OUTSIDE and r["plane"] == -1 and abs(r["tau"] * 4 - hm.mpmath.mpf(7) / 8) < 1e-50
        v2[2 + 16 * (3 + 12 * 4)] = 1
        r = hm.piece_hit_mp(cm, 4.0, g, v2)
        assert r["tau"] == 0 and r["voxel"] == 2 + 16 * (3 + 12 * 4) and r["axis"] == -1


def test_reference_against_dense_sampling_of_itself(fx):
    """Every 5th case at 2001 rational times, exact arithmetic: no sample before t* is blocked, and a free case has no blocked
    sample at all.  Hit cases (every 3rd): the exact point just behind t* (by 1e-9 in normalised time, well inside the 1e-6 the
    generator keeps clear) is in the reference's voxel, or outside the map when it says so."""
    from fractions import Fraction as Fr
    G = grids_of(fx)
    cell_at = lambda q, x, grid: tuple(hm.cell_of(hm._pval(q[ax], x), grid.size[ax]) for ax in range(3))
    for i in range(0, len(fx["T"]), 5):
        s = int(fx["s"][i])
        grid, vox = G[int(fx["grid"][i])]
        q = hm.q_exact(fx["cm"][i][:, :2 * s], fx["T"][i], grid)
        tau = fx["tau"][i]
        for j in range(2001):
            if j / 2000.0 < tau:
                assert hm.probe(cell_at(q, Fr(j, 2000), grid), grid, vox) == hm.HIT_FREE, (i, str(fx["family"][i]), j)
        if math.isinf(tau):
            assert fx["voxel"][i] == hm.HIT_FREE
    for i in np.flatnonzero(fx["voxel"] != hm.HIT_FREE)[::3]:
        s = int(fx["s"][i])
        grid, vox = G[int(fx["grid"][i])]
        q = hm.q_exact(fx["cm"][i][:, :2 * s], fx["T"][i], grid)
        x = Fr(float(fx["tau"][i])) + Fr(1, 10 ** 9)
        assert hm.probe(cell_at(q, x, grid), grid, vox) == fx["voxel"][i], (i, str(fx["family"][i]))


def test_golden_file_is_what_the_generator_writes(fx):
    """Spot check: the stored reference of every 9th case is recomputed (the whole file: make_traj_voxel_hit_golden --check)."""
    G = grids_of(fx)
    for i in range(0, len(fx["T"]), 9):
        s = int(fx["s"][i])
        grid, vox = G[int(fx["grid"][i])]
        r = hm.piece_hit_mp(fx["cm"][i][:, :2 * s], fx["T"][i], grid, vox)
        assert r["voxel"] == fx["voxel"][i] and r["axis"] == fx["axis"][i]
        assert (float(r["tau"]) if r["tau"] is not None else math.inf) == fx["tau"][i]
    rej, drawn = fx["rejected"]
    assert rej < 0.05 * drawn


def test_fixture_holds_every_family(fx):
    fams = ["free", "hit_low", "hit_high"] + ["exit_%s%d" % (a, h) for a in "xyz" for h in (0, 1)] + \
        ["start_blocked", "cell0", "cheb", "long", "unit", "graze_in", "graze_out"]
    for s in (2, 3, 4):
        assert set(fx["family"][fx["s"] == s]) == set(fams)
    assert (fx["n_cross"][fx["family"] == "long"] > 30).all()
    assert (fx["voxel"][fx["family"] == "graze_in"] >= 0).all() and (fx["voxel"][fx["family"] == "graze_out"] == hm.HIT_FREE).all()
    assert 0.02 < np.mean(fx["vox0"] != 0) < 0.04 and fx["vox0"][8 + 16 * (6 + 12 * 4)] == 0
    c0 = fx["family"] == "cell0"
    assert (fx["voxel"][c0] == hm.HIT_OUTSIDE).any() and (fx["voxel"][c0] == hm.HIT_FREE).any()
    assert (fx["plane"][c0 & (fx["voxel"] == hm.HIT_OUTSIDE)] == -1).all()


# ---- the kernel's procedure in float64 ------------------------------------------------------------------------
def test_float64_restatement_meets_the_bound_on_every_case(fx):
    G = grids_of(fx)
    worst, stats = {}, {}
    free_nodes, free_lookups = [], []
    for i in range(len(fx["T"])):
        s, fam = int(fx["s"][i]), str(fx["family"][i])
        grid, vox = G[int(fx["grid"][i])]
        st = {}
        t, v = hit_float64(fx["cm"][i][:, :2 * s], float(fx["T"][i]), grid, vox, stats=st)
        for k, x in st.items():
            stats[k] = stats.get(k, 0) + x
        assert v == fx["voxel"][i], (i, fam, s, v, fx["voxel"][i], t, fx["t"][i])
        if v == hm.HIT_FREE:
            assert t == math.inf
            free_nodes.append(st["nodes"]); free_lookups.append(st.get("lookups", 0))
            continue
        bound = float(hm.hit_bound(fx["T"][i], fx["scale"][i], fx["dq"][i]))
        ratio = abs(t - fx["t"][i]) / bound
        worst[fam] = max(worst.get(fam, 0.0), ratio)
        assert ratio <= 1.0, (i, fam, s, t, fx["t"][i], ratio)
        if math.isfinite(fx["dq"][i]):       # against the rounding term alone (the depth term is T 2^-32 on every case)
            worst["rounding term alone"] = max(worst.get("rounding term alone", 0.0),
                                               abs(t - fx["t"][i]) / (bound - fx["T"][i] * 2.0 ** -hm.HIT_DEPTH))
    print("worst |err| / bound per family:", {k: "%.3g" % v for k, v in worst.items()}, stats)
    print("free pieces: median nodes %g, median lookups %g" % (np.median(free_nodes), np.median(free_lookups)))
    assert stats["bisect"] > 50           # crossings are located by bisection, not left to the depth bound


def test_node_budget_gives_the_conservative_answer():
    """hm.corner_case: every corner costs the procedure a descent to the depth bound.  With the kernel's budget the visits run
    out: a finite t_hit with HIT_INVALID, before which every sample is free; with a budget large enough the curve is found free,
    which it is."""
    grid, vox, cm, T = hm.corner_case(4)
    q = np.array([[float(c) for c in qa] for qa in hm.q_exact(cm, T, grid)])
    assert np.array_equal(q[0], q[1]) and np.array_equal(q[0], q[2])      # the diagonal, exactly
    t, v = hit_float64(cm, T, grid, vox)
    assert v == hm.HIT_INVALID and 0.0 < t < T
    for j in range(400):
        tt = j * t / 400.0
        assert hm.probe(hm.cells_float64(cm, T, grid, tt), grid, vox) == hm.HIT_FREE
    st = {}
    assert hit_float64(cm, T, grid, vox, max_nodes=10 ** 6, stats=st) == (math.inf, hm.HIT_FREE)
    assert st["nodes"] > hm.HIT_MAX_NODES and st["depth"] > 20


def test_planar_trajectory_on_a_cell_plane_is_cheap():
    """z = 1.0 m exactly is the plane q_z = 4 of the grid; the layer below it is full.  The constant component keeps its exact
    value through every de Casteljau step, the curve is in layer 4 as query says, and the piece is free after a few visits."""
    grid = hm.Grid(SIZE, ORIGIN, SCALE)
    vox = np.zeros(16 * 12 * 8, dtype=np.uint8).reshape(8, 12, 16)
    vox[3] = 1
    cm = np.zeros((3, 6))
    cm[2, -1] = 1.0
    cm[0, -1], cm[0, -2], cm[0, -3] = -1.3, 0.9, -0.11
    cm[1, -1], cm[1, -2], cm[1, -4] = -0.7, 0.5, 0.03
    st = {}
    assert hit_float64(cm, 2.5, grid, vox.ravel(), stats=st) == (math.inf, hm.HIT_FREE)
    assert st["nodes"] < 100
    cm[2, -1] = 1.0 - 1e-9
    t, v = hit_float64(cm, 2.5, grid, vox.ravel())
    assert t == 0.0 and v >= 0


# ---- the unit and its bindings ------------------------------------------------------------------------------------
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
    assert "api_voxel_hit.hip" in build.SOURCES
    for n in ("traj_voxel_hit", "traj_voxel_hit_dev", "traj_first_collision"):
        assert callable(getattr(aa, n))
    for n in ("getFirstCollision", "checkCollisionFree"):
        assert callable(getattr(aa.Trajectory, n))
    assert callable(aa.Piece.getFirstCollision)
    assert (aa.HIT_FREE, aa.HIT_OUTSIDE, aa.HIT_INVALID) == (hm.HIT_FREE, hm.HIT_OUTSIDE, hm.HIT_INVALID)
    hdr = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    for name, val in (("ANET_HIT_FREE", -1), ("ANET_HIT_OUTSIDE", -2), ("ANET_HIT_INVALID", -3)):
        assert re.search(r"#define %s \(%d\)" % (name, val), hdr), name
    assert lib.anet_abi_version() == 2


def test_kernel_constants_match_the_restatement():
    txt = open(os.path.join(ROOT, "allocnet_amd", "csrc", "voxel_hit_kernels.h")).read()
    for name, val in (("kHitDepth", hm.HIT_DEPTH), ("kHitMaxNodes", hm.HIT_MAX_NODES), ("kHitBisect", hm.HIT_BISECT),
                      ("kHitBoxCells", hm.HIT_BOX_CELLS), ("kHitC", hm.HIT_C)):
        m = re.search(name + r" = ([0-9.]+);", txt)
        assert m and float(m.group(1)) == float(val), name
    m = re.search(r"kHitFree = (-\d+), kHitOutside = (-\d+), kHitInvalid = (-\d+);", txt)
    assert m and [int(x) for x in m.groups()] == [hm.HIT_FREE, hm.HIT_OUTSIDE, hm.HIT_INVALID]


def test_voxel_hit_unit_resources():
    """The unit compiles for gfx950 with the product's flags; the three instantiations use no scratch, no LDS and no AGPRs, and
    the registers and occupancy DESIGN.md 8l quotes (its resource table is read here)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_voxel_hit.hip"), "-o", os.path.join(td, "u.o")],
                             capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    usage, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    kernels = {fn: u for fn, u in usage.items() if "k_traj_voxel_hit" in fn}
    assert len(kernels) == 3, list(usage)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 8l."):design.index("## 9.")]
    for fn, u in sorted(kernels.items()):
        print(fn, u)
        assert u["ScratchSize"] == 0 and u["LDS"] == 0 and u["AGPRs"] == 0, (fn, u)
        assert u["VGPRs"] <= 256 and u["Occupancy"] >= 2, (fn, u)
        assert "| %d | %d |" % (u["VGPRs"], u["Occupancy"]) in sec, (fn, u, "DESIGN.md 8l quotes other figures")


def test_cpp_header_compiles_as_cxx14():
    src = os.path.join(ROOT, "tests", "cpp", "test_traj_voxel_hit.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
