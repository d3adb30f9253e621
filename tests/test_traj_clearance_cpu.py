"""k_traj_clearance without a GPU: the multiprecision reference against closed forms and against itself, the fixture, a float64
restatement of the kernel's procedure against the a-priori bound, the budgets, the ABI plumbing, the unit's resources and the
facade logic."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import traj_clearance_mp as cl
from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("anet_traj_clearance_dev", "anet_traj_clearance")
FAMILIES = ["solver", "min_t0", "min_tT", "interior", "on_curve", "near_touch", "stationary", "straight", "cheb", "symmetric",
            "duplicates", "nonfinite", "empty", "T0", "spread"]

needs_mp = pytest.mark.skipif(cl.mpmath is None, reason="mpmath / sympy not installed")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "traj_clearance_cases.npz"))


def case(fx, i):
    """(cm (3, 2s), T, the points the kernel may use)"""
    s = int(fx["s"][i])
    off = int(fx["npts"][:i].sum())
    pts = fx["pts"][off:off + int(fx["npts"][i])]
    if fx["count"][i] >= 0:
        pts = pts[:int(fx["count"][i])]
    return fx["cm"][i][:, :2 * s], float(fx["T"][i]), pts


def bounds(fx):
    """clearance_bound of every case; the two coefficient sums are formed here, exactly, from the case's doubles"""
    sc = np.array([cl.scales(*case(fx, i)) for i in range(len(fx["T"]))])
    return cl.clearance_bound(sc[:, 0], sc[:, 1], fx["speed"], fx["kappa"], fx["d"], fx["interior"])


@needs_mp
def test_reference_straight_line_in_closed_form():
    """p(t) = (t, 0, 0) on [0, 2]: a point above the middle, one behind the start, one past the end"""
    cm = np.zeros((3, 6))
    cm[0, -2] = 1.0
    pts = np.array([[1.0, 3.0, 4.0], [-3.0, 4.0, 0.0], [2.5, 0.0, 1.0]])
    for j, (want, tau) in enumerate([(5.0, 0.5), (5.0, 0.0), (np.sqrt(1.25), 1.0)]):
        r = cl.piece_clearance_mp(cm, 2.0, pts[j:j + 1])
        assert abs(float(r["d"]) - want) < 1e-15 and float(r["tau"]) == tau and r["interior"] == (j == 0)
    r = cl.piece_clearance_mp(cm, 2.0, pts)
    assert r["point"] == 2 and abs(float(r["runner"]) - 5.0) < 1e-15
    assert cl.piece_clearance_mp(cm, 2.0, np.array([[np.nan, 0.0, 0.0]]))["point"] == -1
    c, p, t = cl.clearance_float64(cm, 2.0, pts)
    assert p == 2 and t == 2.0 and abs(c - np.sqrt(1.25)) < 1e-15


@needs_mp
def test_reference_against_dense_sampling_of_itself(fx):
    """Every 6th case at 401 times in 60 digits: no sample is nearer than the reference, and the nearest is within L / 800."""
    for i in range(0, len(fx["T"]), 6):
        cm, T, pts = case(fx, i)
        fin = cl.finite_points(pts)
        if not fin:
            continue
        best = min(float(cl.dist_mp(cm, T, T * k / 400.0, pts[j])) for j in fin[:6] for k in range(401))
        per6 = cl.piece_clearance_mp(cm, T, pts[fin[:6]])
        assert best >= float(per6["d"]) - 1e-15
        speed = max(np.linalg.norm([np.polyval(np.polyder(cm[ax]), T * k / 50.0) for ax in range(3)]) for k in range(51))
        assert best <= float(per6["d"]) + 1.5 * speed * T / 800.0 + 1e-12


@needs_mp
def test_golden_file_is_what_the_generator_writes(fx):
    """Spot check: the stored reference of every 9th case is recomputed (the whole file: make_traj_clearance_golden --check)."""
    for i in range(0, len(fx["T"]), 9):
        cm, T, pts = case(fx, i)
        r = cl.piece_clearance_mp(cm, T, pts)
        assert float(r["d"]) == fx["d"][i] and r["point"] == fx["point"][i] and float(r["tau"]) == fx["tau"][i]
        assert float(r["runner"]) == fx["runner"][i] and r["interior"] == fx["interior"][i]
        assert float(r["kappa"]) == fx["kappa"][i] and float(r["speed"]) == fx["speed"][i]
        if r["point"] >= 0:      # the exact-rational distance of the GPU tests against the 60-digit one
            t = float(r["tau"]) * T
            assert abs(cl.dist_exact(cm, T, t, pts[r["point"]]) - float(cl.dist_mp(cm, T, t, pts[r["point"]]))) <= 4e-16 * max(fx["d"][i], 1e-300)


def test_fixture_holds_every_family(fx):
    assert list(fx["families"]) == FAMILIES
    n = len(fx["T"])
    assert 100 <= n <= 400 and fx["npts"].max() <= 48
    for s in (2, 3, 4):
        for f in range(len(FAMILIES)):
            assert ((fx["s"] == s) & (fx["family"] == f)).sum() >= 3, (s, FAMILIES[f])
    fam = lambda name: fx["family"] == FAMILIES.index(name)
    assert (fx["tau"][fam("min_t0")] == 0.0).all() and (fx["tau"][fam("min_tT")] == 1.0).all()
    assert fx["interior"][fam("interior") | fam("near_touch") | fam("symmetric")].all()
    assert ((fx["d"][fam("near_touch")] > 1e-13) & (fx["d"][fam("near_touch")] < 2e-6)).all()
    assert (fx["d"][fam("on_curve")] < 1e-13).all()
    assert (fx["d"][fam("empty")] == np.inf).all() and (fx["point"][fam("empty")] == -1).all()
    assert (fx["T"][fam("T0")] == 0.0).all() and np.isin(fx["T"][fam("spread")], [1e-3, 30.0]).all()
    assert (fx["runner"][fam("duplicates")] == fx["d"][fam("duplicates")]).all()
    usual = ~(fam("T0") | fam("spread"))
    assert ((fx["T"][usual] >= 0.3) & (fx["T"][usual] <= 3.0)).all()
    fin = fx["pts"][np.isfinite(fx["pts"])]
    assert np.abs(fin).max() <= 20.0
    assert os.path.getsize(os.path.join(GOLDEN, "traj_clearance_cases.npz")) < 32 * 1024


def test_bound_is_not_vacuous(fx):
    """The cap of the issue: at most 1e-9 m on every fixture case, near-touching and on-curve ones included; the Chebyshev-like
    family of order 4 has the cap traj_clearance_mp.cap_of derives for it.  No case was selected by its bound."""
    b = bounds(fx)
    cap = np.array([cl.cap_of(FAMILIES[f], int(s)) for f, s in zip(fx["family"], fx["s"])])
    assert (cap[~((fx["family"] == FAMILIES.index("cheb")) & (fx["s"] == 4))] == cl.CAP).all() and cl.CAP == 1e-9
    for s in (2, 3, 4):
        print("s=%d largest bound per family:" % s,
              {f: "%.3g" % b[(fx["family"] == k) & (fx["s"] == s)].max() for k, f in enumerate(FAMILIES)})
    assert np.isfinite(b).all() and (b <= cap).all(), [(i, FAMILIES[fx["family"][i]], int(fx["s"][i]), b[i]) for i in np.flatnonzero(~(b <= cap))]


def test_float64_restatement_meets_the_bound_on_every_case(fx):
    """The kernel's procedure in plain float64: |clearance - ref| <= bound, never below ref - bound, inf cases exact, the point
    where the runner-up is farther than twice the bound, 0 <= t <= T; no budget runs out on any case."""
    b = bounds(fx)
    worst, out_of_budget, surv = {}, 0, []
    for i in range(len(fx["T"])):
        cm, T, pts = case(fx, i)
        st = {}
        c, p, t = cl.clearance_float64(cm, T, pts, stats=st)
        out_of_budget += st["nodes_out"] + st["depth_out"]
        surv.append(st["survivors"])
        f = FAMILIES[int(fx["family"][i])]
        if fx["point"][i] < 0:
            assert c == np.inf and p == -1 and t == 0.0, i
            continue
        err = abs(c - fx["d"][i])
        worst[f] = max(worst.get(f, 0.0), err / b[i])
        assert err <= b[i] and c >= fx["d"][i] - b[i], (i, f, c, fx["d"][i], b[i])
        assert 0.0 <= t <= T and 0 <= p < len(pts)
        if fx["runner"][i] - fx["d"][i] > 2.0 * b[i]:
            assert p == fx["point"][i], (i, f)
    print("worst err / bound per family:", {k: "%.3g" % v for k, v in worst.items()})
    print("survivors per case: mean %.2f, max %d" % (np.mean(surv), max(surv)))
    assert out_of_budget == 0


def test_restatement_edge_inputs():
    cm = np.zeros((3, 6))
    cm[0, -2] = 1.0
    pts = np.array([[0.5, 1.0, 0.0]])
    for badcm, T in ((np.where(np.arange(6) == 2, np.nan, cm), 1.0), (cm, -1.0), (cm, np.inf), (cm, np.nan)):
        c, p, t = cl.clearance_float64(badcm, T, pts)
        assert np.isnan(c) and p == -1 and t == 0.0
    assert cl.clearance_float64(cm, 1.0, np.zeros((0, 3))) == (np.inf, -1, 0.0)
    assert cl.clearance_float64(cm, 1.0, pts, count=0) == (np.inf, -1, 0.0)
    assert cl.clearance_float64(cm, 1.0, pts, count=5)[0] == 1.0
    assert cl.clearance_float64(cm, 0.0, pts)[0] == np.sqrt(1.25)


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
    assert "api_clearance.hip" in build.SOURCES
    for n in ("traj_clearance", "traj_clearance_dev"):
        assert callable(getattr(aa, n))
    for n in ("getClearance", "checkClearance"):
        assert callable(getattr(aa.Trajectory, n)) and callable(getattr(aa.Piece, n))
    assert lib.anet_abi_version() == 2


def test_kernel_constants_match_the_restatement():
    txt = open(os.path.join(ROOT, "allocnet_amd", "csrc", "clearance_kernels.h")).read()
    for name, val in (("kClrK", cl.CLR_K), ("kClrMaxDepth", cl.CLR_DEPTH), ("kClrMaxNodes", cl.CLR_MAX_NODES),
                      ("kClrBisect", cl.CLR_BISECT), ("kClrSlack", cl.CLR_SLACK)):
        m = re.search(name + r" = ([0-9.]+);", txt)
        assert m and float(m.group(1)) == float(val), name


def test_clearance_unit_resources():
    """The unit compiles alone for gfx950 with the product's flags; the three instantiations use no scratch and the one LDS tile,
    and the registers and occupancy DESIGN.md 8m quotes (its resource table is read here)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_clearance.hip"), "-o", os.path.join(td, "u.o")],
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
    kernels = {fn: u for fn, u in usage.items() if "k_traj_clearance" in fn}
    assert len(kernels) == 3, list(usage)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 8m."):design.index("## 9.")]
    for fn, u in sorted(kernels.items()):
        print(fn, u)
        assert u["ScratchSize"] == 0 and u["LDS"] == 1536, (fn, u)
        assert "| %d | %d | %d |" % (u["VGPRs"], u["AGPRs"], u["Occupancy"]) in sec, (fn, u, "DESIGN.md 8m quotes other figures")


def test_cpp_header_compiles_as_cxx14():
    src = os.path.join(ROOT, "tests", "cpp", "test_traj_clearance.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_facade_logic_on_stubbed_results(monkeypatch):
    """Trajectory / Piece getClearance and checkClearance on stubbed per-piece results: the smallest piece wins, global time, NaN
    is never clear, no point is always clear."""
    import allocnet_amd as aa
    from allocnet_amd import trajectory as tr
    seen = {}

    def stub(coeffs, T, points, counts=None, ctx=None):
        seen["shape"] = (np.asarray(coeffs).shape, np.asarray(T).shape)
        n = np.asarray(T).shape[1]
        return (np.asarray(seen["c"][:n], dtype=np.float64)[None], np.asarray(seen["p"][:n], dtype=np.int32)[None],
                np.asarray(seen["t"][:n], dtype=np.float64)[None])
    monkeypatch.setattr(tr, "traj_clearance", stub)
    cm = np.zeros((3, 6))
    traj = aa.Trajectory([0.5, 2.0, 1.0], [cm, cm, cm])
    pts = np.zeros((4, 3))
    seen.update(c=[0.8, 0.25, 0.6], p=[3, 1, 0], t=[0.1, 1.5, 0.0])
    assert traj.getClearance(pts) == (0.25, 0.5 + 1.5, 1, 1)
    assert seen["shape"] == ((1, 3, 3, 6), (1, 3))
    c, p, t = traj.getClearance(pts, per_piece=True)
    assert list(c) == [0.8, 0.25, 0.6] and list(p) == [3, 1, 0] and p.dtype == np.int32 and list(t) == [0.1, 1.5, 0.0]
    assert traj.checkClearance(pts, 0.25) and traj.checkClearance(pts, 0.2) and not traj.checkClearance(pts, 0.2500001)
    assert traj[1].getClearance(pts) == (0.8, 0.1, 3) and traj[1].checkClearance(pts, 0.8) and not traj[1].checkClearance(pts, 0.9)
    seen.update(c=[0.8, np.nan, 0.1], p=[3, -1, 0], t=[0.1, 0.0, 0.0])
    d, tt, piece, point = traj.getClearance(pts)
    assert np.isnan(d) and piece == 1 and point == -1 and tt == 0.0
    assert not traj.checkClearance(pts, 0.0) and not traj.checkClearance(pts, -1.0)
    seen.update(c=[np.inf, np.inf, np.inf], p=[-1, -1, -1], t=[0.0, 0.0, 0.0])
    assert traj.getClearance(pts) == (np.inf, 0.0, -1, -1) and traj.checkClearance(pts, 1e9)
    seen.update(c=[np.inf, 0.4, np.inf], p=[-1, 2, -1], t=[0.0, 2.0, 0.0])
    assert traj.getClearance(pts) == (0.4, 2.5, 1, 2)
