"""CPU suite of the shortest route through a corridor and the setup on top of it: the numpy restatement (tests/sfc_path_np.py)
against facts -- central differences, exact zeros in padded slots, the fixed-order sum, the convex optimum --, the enumeration of
a polytope stacked with itself, the allotment of pieces and first durations against hand-computed cases, and the compile checks
of the new kernel, layout and exports."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import polytope_np as pnp
from tests import sfc_np
from tests import sfc_path_np as spn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_problem(rng, Nm1, K, spread=3.0):
    count = rng.integers(2, K - 2, size=Nm1)
    verts = np.zeros((Nm1, K, 3)); xi = np.zeros((Nm1, K))
    for w in range(Nm1):
        verts[w, :count[w]] = rng.normal(size=(count[w], 3)) * spread + np.array([4.0 * w, 0.0, 0.0])
        xi[w, :count[w]] = rng.normal(size=count[w]) * rng.choice([0.3, 1.0])
    return xi, verts, count, rng.normal(size=3) - np.array([4.0, 0.0, 0.0]), rng.normal(size=3) + np.array([4.0 * Nm1, 0.0, 0.0])


# ---- 1. gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nm1,K", [(1, 16), (2, 24), (7, 32)])
def test_gradient_matches_central_differences_and_padded_slots_are_zero(Nm1, K):
    """h = 1e-6 on a cost of order 10 m: rounding 1e-15 * 10 / 2e-6 = 5e-9, truncation h^2 |L'''| of the same order: 1e-7 max(1, |g|)
    as tests/test_sfc_opt_cpu.py holds the transform to."""
    rng = np.random.default_rng(31 + Nm1)
    xi, verts, count, start, goal = _random_problem(rng, Nm1, K)
    for eps, w_norm in [(1e-2, 1.0), (0.5, 0.3)]:
        L, g, P = spn.route_cost(xi, verts, start, goal, eps, w_norm)
        assert any(np.square(xi[w]).sum() > 1.0 for w in range(Nm1))                 # the norm term is live
        h = 1e-6
        for w in range(Nm1):
            for j in range(count[w]):
                e = np.zeros_like(xi); e[w, j] = h
                fd = (spn.route_cost(xi + e, verts, start, goal, eps, w_norm)[0] - spn.route_cost(xi - e, verts, start, goal, eps, w_norm)[0]) / (2 * h)
                assert abs(fd - g[w, j]) <= 1e-7 * max(1.0, np.abs(g).max()), (w, j, fd, g[w, j])
            assert (g[w, count[w]:] == 0.0).all()


def test_gradient_in_P_is_the_difference_of_unit_legs():
    """dL/dP_w = (P_w - P_{w-1}) / l_{w-1} - (P_{w+1} - P_w) / l_w against central differences in P itself (one vertex per waypoint
    carrying all the weight makes P that vertex)."""
    rng = np.random.default_rng(37)
    pts = rng.normal(size=(6, 3)) * 2.0
    eps = 1e-2
    f = lambda p: spn.fixed_order_sum(spn.legs(p, eps))
    l = spn.legs(pts, eps)
    u = np.diff(pts, axis=0) / l[:, None]
    for w in range(1, 5):
        for a in range(3):
            e = np.zeros_like(pts); e[w, a] = 1e-6
            assert abs((f(pts + e) - f(pts - e)) / 2e-6 - (u[w - 1] - u[w])[a]) <= 1e-8


# ---- 2. fixed-order sum ---------------------------------------------------------------------------------------------------------------
def test_cost_is_the_fixed_order_sum_of_legs_then_norm_terms():
    rng = np.random.default_rng(41)
    for Nm1, K in [(1, 8), (7, 16), (15, 12)]:
        xi, verts, count, start, goal = _random_problem(rng, Nm1, K)
        L, _, P = spn.route_cost(xi, verts, start, goal, 1e-2, 0.7)
        pts = [start] + list(P) + [goal]
        want = 0.0
        for i in range(Nm1 + 1):
            d = pts[i + 1] - pts[i]
            want = want + math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] + 1e-2 * 1e-2)
        norms = 0.0
        for w in range(Nm1):
            S = float(np.square(xi[w]).sum())
            norms = norms + 0.7 * max(S - 1.0, 0.0) ** 3
        assert norms > 0.0 and L == want + norms
        # one problem changed elsewhere changes nothing here: the function takes one problem at a time
        assert spn.route_cost(xi.copy(), verts.copy(), start.copy(), goal.copy(), 1e-2, 0.7)[0] == L


# ---- 3. gap to the convex optimum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [9, 7, 1])
def test_route_is_within_gap_of_the_convex_optimum(seed):
    R = spn.reference(seed)
    g = spn.gaps(seed)
    ev = np.array([r["evals"] for r in R["route"]])
    print("seed %d: %d problems, worst gap %.3g, evaluations median %g max %d" % (seed, len(g), g.max(), np.median(ev), ev.max()))
    assert len(g) == spn.SUBSET[seed][0]
    assert g.max() <= spn.GAP
    assert g.min() >= -1e-9                       # the optimum is no longer than a feasible route (SLSQP's own convergence)
    assert spn.GAP == 2.0 * max(spn.WORST_GAP.values())
    for b in range(len(g)):
        # facts about the reference itself: at least the straight line, at most the route it started from, its points inside
        straight = spn.smoothed_length(R["start"][b], np.zeros((0, 3)), R["goal"][b])
        assert R["optimum"][b] >= straight - 1e-12
        for w in range(R["N"] - 1):
            assert sfc_np.row_violation(R["pairs"][b, w], R["route"][b]["wps"][w]) <= spn.ENUM_EPS, (b, w)
            assert sfc_np.row_violation(R["pairs"][b, w], R["opt_wps"][b, w]) <= 1e-9, (b, w)
        assert R["route"][b]["ret"] in (0, 1) and R["route"][b]["evals"] < spn.MAX_EVALS


def test_vertex_mean_start_is_far_from_the_shortest_route():
    """Why the route is computed at all: the median excess of the vertex-mean start over the optimum (the issue's table)."""
    for seed, least in [(9, 0.15), (7, 0.2), (1, 0.5)]:
        R = spn.reference(seed)
        mean = np.array([spn.smoothed_length(R["start"][b], sfc_np.forward(spn.mean_start(R["count"][b], R["K"]), R["verts"][b])[0],
                                             R["goal"][b]) for b in range(len(R["optimum"]))])
        assert np.median(mean / R["optimum"] - 1.0) >= least


# ---- 4. repeated polytopes ------------------------------------------------------------------------------------------------------------
def test_overlap_of_a_polytope_with_itself_enumerates_its_own_vertices():
    """sfc_expand_corridor repeats a polytope; the stacked pair (polytope, itself) has, among its duplicated rows, only singular
    triples and repeats of the polytope's own vertices, which the merge removes: pnp.enumerate_triples of the pair gives the
    polytope's vertex set -- Qhull's, and that of the triples of the single polytope, in the same order."""
    import allocnet_amd as aa
    from scipy.spatial import HalfspaceIntersection
    checked = 0
    for seed, B, N, M in sfc_np.INPUTS:
        hp = sfc_np.corridor(seed, B, N, M)[4]
        for b in range(0, 24, 3):
            pieces = np.ones(N, dtype=np.int64); pieces[b % N] = 2
            ex = aa.sfc_expand_corridor(hp[b], pieces)
            assert ex.shape == (N + 1, M, 4)
            i = b % N
            assert np.array_equal(ex[i], hp[b, i]) and np.array_equal(ex[i + 1], hp[b, i]) and np.array_equal(ex[i + 2:], hp[b, i + 1:])
            pair = sfc_np.stacked_raw(ex[None])[0, i]
            single = pair[:M]
            assert np.array_equal(pair[:M], pair[M:])
            v_pair, det_pair = pnp.enumerate_triples(pair)
            v_one, det_one = pnp.enumerate_triples(single)
            depth, x = pnp.interior(single)
            n, d, _ = pnp.unit_rows(single)
            vq = pnp.merge(HalfspaceIntersection(np.c_[n, d], x).intersections)
            assert len(v_pair) == len(v_one) == len(vq), (seed, b)
            assert np.array_equal(v_pair, v_one) and det_pair == det_one
            assert pnp.hausdorff(v_pair, vq) <= 1e-8 * max(1.0, np.abs(vq).max())
            checked += 1
    assert checked == 24


# ---- 5. allotment and durations -------------------------------------------------------------------------------------------------------
def test_allotment_spacing_and_durations_of_hand_computed_cases():
    import allocnet_amd as aa
    # legs: 0 (start on the first junction), exactly 3 x 2.0, 5 (3-4-0 triangle side): ceil(0 / 2) -> 1, 3, ceil(2.5) = 3
    route = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [7.0, 1.0, 0.0], [10.0, 5.0, 0.0]])
    pieces = aa.sfc_allot_pieces(route, 2.0)
    assert pieces.tolist() == [1, 3, 3] and pieces.dtype == np.int64
    assert aa.sfc_allot_pieces(route, 6.0).tolist() == [1, 1, 1] and aa.sfc_allot_pieces(route, 5.0).tolist() == [1, 2, 1]
    assert aa.sfc_allot_pieces(np.stack([route, route[::-1]]), 2.0).tolist() == [[1, 3, 3], [3, 3, 1]]      # batched
    wps, lens = aa.sfc_route_waypoints(route, pieces)
    want = np.array([[1.0, 1.0, 0.0], [3.0, 1.0, 0.0], [5.0, 1.0, 0.0], [7.0, 1.0, 0.0], [8.0, 7.0 / 3.0, 0.0], [9.0, 11.0 / 3.0, 0.0]])
    assert wps.shape == want.shape and np.abs(wps - want).max() <= 4e-15             # a few roundings at 10 m
    assert np.array_equal(wps[0], route[1]) and np.array_equal(wps[3], route[2])         # the junctions themselves, bit for bit
    assert np.abs(lens - np.array([0.0, 2.0, 2.0, 2.0, 5.0 / 3.0, 5.0 / 3.0, 5.0 / 3.0])).max() <= 4e-16
    # speed 4 m/s: 0, 0.5, 0.5, 0.5, 5/12 x 3; min_duration 0.45 binds on the zero leg and on the last three
    T = aa.sfc_first_durations(lens, 4.0, 0.45)
    assert np.abs(T - np.array([0.45, 0.5, 0.5, 0.5, 0.45, 0.45, 0.45])).max() <= 1e-16
    assert np.abs(aa.sfc_first_durations(lens, 4.0, 0.0) - np.array([0.0, 0.5, 0.5, 0.5, 5.0 / 12.0, 5.0 / 12.0, 5.0 / 12.0])).max() <= 1e-16
    hp = np.arange(3 * 2 * 4, dtype=np.float64).reshape(3, 2, 4)
    ex = aa.sfc_expand_corridor(hp, pieces)
    assert ex.shape == (7, 2, 4) and [int(e[0, 0]) // 8 for e in ex] == [0, 1, 1, 1, 2, 2, 2]
    assert len(wps) == len(ex) - 1 and len(T) == len(ex)
    with pytest.raises(ValueError):
        aa.sfc_allot_pieces(route, 0.0)
    with pytest.raises(ValueError):
        aa.sfc_expand_corridor(hp, [1, 0, 1])


# ---- 6. workspace carve ---------------------------------------------------------------------------------------------------------------
def test_route_workspace_carves_without_overlap_under_sanitizers(tmp_path):
    """tests/cpp/test_sfc_path_workspace_layout.cpp, a stand-alone program over csrc/workspace.h alone, built with the host compiler
    under AddressSanitizer and UBSan and run as an ordinary executable, against the sizes anet_sfc_shortest_path_workspace()
    returns -- with the caller's parameters and with NULL (the defaults: mem_size 8, past 3)."""
    from allocnet_amd import _lib
    lib = _lib.load()
    exe = str(tmp_path / "test_sfc_path_workspace_layout")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                          os.path.join(ROOT, "tests", "cpp", "test_sfc_path_workspace_layout.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = []
    for N, K, ld, m, past in [(2, 16, 1, 8, 3), (2, 16, 65, 8, 3), (3, 24, 72, 8, 0), (8, 32, 264, 6, 5), (16, 8, 7, 20, 1), (5, 3, 3, 1, 2)]:
        prm = _lib.LbfgsParams()
        lib.anet_lbfgs_default_params(ctypes.byref(prm))
        prm.mem_size, prm.past = m, past
        want = lib.anet_sfc_shortest_path_workspace(N, K, ld, ctypes.cast(ctypes.pointer(prm), ctypes.c_void_p))
        assert want > 0
        lines.append("sfc_path %d %d %d %d %d %d" % (N, K, ld, m, past, want))
    for N, K, ld in [(2, 16, 1), (8, 32, 264)]:
        lines.append("sfc_path %d %d %d 8 3 %d" % (N, K, ld, lib.anet_sfc_shortest_path_workspace(N, K, ld, None)))
    assert lib.anet_sfc_shortest_path_workspace(1, 16, 8, None) == -1 and lib.anet_sfc_shortest_path_workspace(2, 0, 8, None) == -1
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "8 layouts carved, 0 failures" in res.stdout


# ---- 7. kernel resources --------------------------------------------------------------------------------------------------------------
def test_route_kernels_use_no_scratch_memory_and_no_lds():
    """The unit compiled for gfx950 with the product's flags: k_sfc_path_eval and its helpers keep everything in registers and
    use no LDS (the figures are recorded in DESIGN.md 8s and printed here)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_sfc.hip"), "-o", os.path.join(td, "u.o")],
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
    for want in ("k_sfc_path_eval", "k_sfc_path_mean_start", "k_sfc_path_map", "k_sfc_path_length"):
        hit = {fn: u for fn, u in usage.items() if want in fn}
        assert len(hit) == 1, (want, list(usage))
        for fn, u in hit.items():
            print(fn, u)
            assert u["ScratchSize"] == 0 and u["LDS"] == 0, (fn, u)


# ---- 8. ABI -----------------------------------------------------------------------------------------------------------------------------
def test_route_exports_are_in_the_ctypes_table_with_the_headers_arity():
    from allocnet_amd import _lib
    txt = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret in [("anet_sfc_shortest_path_workspace", ctypes.c_int64), ("anet_sfc_shortest_path_dev", ctypes.c_int),
                      ("anet_sfc_shortest_path", ctypes.c_int), ("anet_sfc_path_cost_grad_dev", ctypes.c_int)]:
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        args = [a.strip() for a in m.group(2).split(",")]
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ret and (m.group(1) == "int64_t") == (ret is ctypes.c_int64)
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        for a, t in zip(args, argtypes):
            want = ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[a.split()[0]]
            assert t is want, (name, a, t)
    assert re.search(r"#define\s+ANET_SFC_PATH_MAX_EVALS\s+400\b", txt)
    import allocnet_amd as aa
    assert aa.sfc_opt.SFC_PATH_MAX_EVALS == 400 == spn.MAX_EVALS
    for fn in ("sfc_shortest_path", "sfc_shortest_path_dev", "sfc_allot_pieces", "sfc_expand_corridor", "sfc_setup"):
        assert callable(getattr(aa, fn))


def test_cpp_route_program_compiles_as_cxx14():
    src = os.path.join(ROOT, "tests", "cpp", "test_sfc_path.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
