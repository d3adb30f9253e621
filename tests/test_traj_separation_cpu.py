"""k_traj_separation without a GPU: the multiprecision reference against closed forms, the fixture, a float64 restatement of the
kernel's procedure against the a-priori bound, the budgets, the ABI plumbing, the unit's resources and the facade logic."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import traj_separation_mp as sp
from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("anet_traj_separation_dev", "anet_traj_separation")
FAMILIES = ["equal", "stagger", "short", "disjoint", "cross", "translated", "self", "knot_min", "end_min", "near_tie", "zero_T",
            "spread", "discont", "cheb"]

needs_mp = pytest.mark.skipif(sp.mpmath is None, reason="mpmath / sympy not installed")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "traj_separation_cases.npz"))


@pytest.fixture(scope="module")
def bounds(fx):
    return np.array([sp.fixture_bound(fx, i) for i in range(len(fx["d"]))])


def test_fixture_holds_every_family(fx):
    assert list(fx["families"]) == FAMILIES
    n = len(fx["d"])
    assert 100 <= n <= 300
    for s in (2, 3, 4):
        for f in range(len(FAMILIES)):
            assert ((fx["s"] == s) & (fx["family"] == f)).sum() >= 1, (s, FAMILIES[f])
    fam = lambda name: fx["family"] == FAMILIES.index(name)
    assert (fx["d"][fam("disjoint")] == np.inf).all() and (fx["pa"][fam("disjoint")] == -1).all() and (fx["n_int"][fam("disjoint")] == 0).all()
    assert (fx["d"][fam("self")] == 0.0).all() and (fx["pair"][fam("self")] == 0).all()
    assert (fx["d"][fam("cross")] == 0.0).all() and fx["interior"][fam("cross")].all()
    assert (fx["d"][fam("translated")] > 0.0).all()
    assert (~fx["interior"][fam("end_min")]).all() and (~fx["interior"][fam("knot_min")]).all()
    assert (fx["runner"][fam("knot_min")] - fx["d"][fam("knot_min")] <= 1e-14).all()      # the junction, seen from both sides
    assert (fx["n_int"][fam("stagger")] >= 1).all() and fx["n_int"].max() <= 5
    T = fx["T"]
    assert ((T == 0.0) | ((T >= 0.05) & (T <= 20.0))).all()
    assert (T[fam("zero_T")] == 0.0).sum() >= 2 * fam("zero_T").sum()
    worst_t = 0.0
    for i in range(n):
        co, Tc, t0, _ = sp.fixture_case(fx, i)
        for r in range(2):
            K = sp.knots(Tc[r], t0[r])
            worst_t = max(worst_t, abs(K[0]), abs(K[-1]))
            for j in range(Tc.shape[1]):       # the curve within +-12 m: its Bernstein control values bound it
                if Tc[r, j] > 0.0:
                    z = sp._load(co[r, j], Tc[r, j])[1]
                    pos = np.array([[np.polyval(co[r, j, ax], x) for x in np.linspace(0.0, Tc[r, j], 33)] for ax in range(3)])
                    assert np.abs(pos).max() <= 12.0 and z is not None
    assert worst_t <= 60.0
    assert os.path.getsize(os.path.join(GOLDEN, "traj_separation_cases.npz")) < 56 * 1024


def test_reference_alone_settles_the_pieces_on_nine_cases_in_ten(fx, bounds):
    """The index-tie rule: the reference's pieces are required where the runner-up interval lies farther than twice the bound; at
    most 10 % of the cases may be excused by it."""
    live = fx["pa"] >= 0
    gap = np.where(live, fx["runner"], 1.0) - np.where(live, fx["d"], 0.0)
    excused = live & ~(gap > 2.0 * bounds[:, 0])
    print("excused by the tie rule: %d of %d" % (excused.sum(), len(live)))
    assert excused.sum() <= 0.10 * len(live)


def test_bound_is_not_vacuous(fx, bounds):
    """At most 1e-9 m on every fixture case.  No case was selected by its bound."""
    b = bounds[:, 0]
    cap = np.array([sp.cap_of(FAMILIES[f], int(s)) for f, s in zip(fx["family"], fx["s"])])
    assert (cap == sp.CAP).all() and sp.CAP == 1e-9
    for s in (2, 3, 4):
        print("s=%d largest bound per family:" % s,
              {f: "%.3g" % b[(fx["family"] == k) & (fx["s"] == s)].max() for k, f in enumerate(FAMILIES)})
    assert np.isfinite(b).all() and (b <= cap).all(), [(i, FAMILIES[fx["family"][i]], int(fx["s"][i]), b[i]) for i in np.flatnonzero(~(b <= cap))]


def test_float64_restatement_meets_the_bound_on_every_case(fx, bounds):
    """(1) The kernel's procedure in plain float64 meets separation_bound on every case, with no budget event."""
    worst, events, surv = {}, 0, []
    for i in range(len(fx["d"])):
        co, T, t0, (a, b) = sp.fixture_case(fx, i)
        st = {}
        res = sp.separation_float64(co, T, t0, a, b, stats=st)
        events += st["steps_out"] + st["nodes_out"] + st["depth_out"]
        surv.append(st["survivors"])
        assert st["intervals"] == fx["n_int"][i], i
        f = FAMILIES[int(fx["family"][i])]
        worst[f] = max(worst.get(f, 0.0), sp.check_result(fx, i, bounds[i], res))
    print("worst err / bound per family:", {k: "%.3g" % v for k, v in worst.items()})
    print("intervals refined per case: mean %.2f, max %d" % (np.mean(surv), max(surv)))
    assert events == 0


def test_restatement_cutoff(fx, bounds):
    """A cutoff above every minimum changes nothing that is asserted; a cutoff of 0 still yields actual distances."""
    for i in range(0, len(fx["d"]), 3):
        co, T, t0, (a, b) = sp.fixture_case(fx, i)
        sp.check_result(fx, i, bounds[i], sp.separation_float64(co, T, t0, a, b, cutoff=100.0))
        sep, t, pa, pb = sp.separation_float64(co, T, t0, a, b, cutoff=0.0)
        if fx["pa"][i] >= 0:
            Ka, Kb = sp.knots(T[a], t0[a]), sp.knots(T[b], t0[b])
            assert sep >= fx["d"][i] - bounds[i][1]
            assert abs(sp.dist_exact(co[a, pa], Ka[pa], co[b, pb], Kb[pb], t) - sep) <= bounds[i][1]


def test_restatement_edge_inputs():
    co = np.zeros((3, 2, 3, 6))
    co[0, :, 0, -2] = 1.0
    co[1, :, 1, -1] = 2.0
    co[2] = np.nan
    T = np.array([[1.0, 1.0], [1.5, 0.0], [1.0, 1.0]])
    assert sp.separation_float64(co, T, None, 0, 1)[0] == 2.0
    assert np.isnan(sp.separation_float64(co, T, None, 0, 2)[0]) and sp.separation_float64(co, T, None, 0, 3) [2] == -1
    assert sp.separation_float64(co, T, np.array([0.0, 2.0, 0.0]), 0, 1) == (np.inf, 0.0, -1, -1)       # touching
    assert sp.separation_float64(co, T, np.array([0.0, 2.5, 0.0]), 0, 1) == (np.inf, 0.0, -1, -1)
    assert sp.separation_float64(co, T, None, 1, 1)[0] == 0.0
    for bad in (np.nan, np.inf, -1.0):
        Tb = T.copy()
        Tb[1, 0] = bad
        assert np.isnan(sp.separation_float64(co, Tb, None, 0, 1)[0]) and sp.separation_float64(co, Tb, None, 0, 0)[0] == 0.0
    assert np.isnan(sp.separation_float64(co, T, np.array([0.0, np.inf, 0.0]), 0, 1)[0])
    co2 = co.copy()
    co2[1, 1] = np.nan      # poison in a piece of zero duration is never read
    assert sp.separation_float64(co2, T, None, 0, 1)[0] == 2.0


@needs_mp
def test_reference_in_closed_form_and_dist_exact_against_60_digits(fx):
    """(2) two straight lines; then dist_exact against dist_mp at the reference's minimum of every 5th case"""
    s = 2
    coa = np.zeros((1, 3, 4))
    coa[0, 0, -2] = 1.0                                  # (t, 0, 0)
    cob = np.zeros((1, 3, 4))
    cob[0, 1, -2], cob[0, 1, -1], cob[0, 2, -1] = 1.0, -1.5, 2.0       # (0, t' - 1.5, 2), t' = t - 0.5
    r = sp.pair_separation_mp(coa, [4.0], 0.0, cob, [4.0], 0.5)
    # d(t) = (t, 2 - t, -2): |d|^2 = 2 t^2 - 4 t + 8, minimal at t = 1: sqrt(6)
    assert abs(float(r["d"]) - np.sqrt(6.0)) < 1e-15 and float(r["t"]) == 1.0 and r["interior"] and (r["pa"], r["pb"]) == (0, 0)
    for i in range(0, len(fx["d"]), 5):
        if fx["pa"][i] < 0:
            continue
        co, T, t0, (a, b) = sp.fixture_case(fx, i)
        pa, pb, t = int(fx["pa"][i]), int(fx["pb"][i]), float(fx["t"][i])
        Ka, Kb = sp.knots(T[a], t0[a]), sp.knots(T[b], t0[b])
        ex, mp_ = sp.dist_exact(co[a, pa], Ka[pa], co[b, pb], Kb[pb], t), float(sp.dist_mp(co[a, pa], Ka[pa], co[b, pb], Kb[pb], t))
        assert abs(ex - mp_) <= 4e-16 * max(mp_, 1e-300)
        rr = sp.pair_separation_mp(co[a], T[a], t0[a], co[b], T[b], t0[b])          # the file is what the generator writes
        assert float(rr["d"]) == fx["d"][i] and (rr["pa"], rr["pb"]) == (pa, pb) and float(rr["runner"]) == fx["runner"][i]


def test_kernel_constants_match_the_restatement():
    """(3)"""
    txt = open(os.path.join(ROOT, "allocnet_amd", "csrc", "separation_kernels.h")).read()
    for name, val in (("kSepK", sp.SEP_K), ("kSepMaxSteps", sp.SEP_STEPS), ("kSepMaxDepth", sp.SEP_DEPTH),
                      ("kSepMaxNodes", sp.SEP_MAX_NODES), ("kSepBisect", sp.SEP_BISECT), ("kSepSlack", sp.SEP_SLACK)):
        m = re.search(name + r" = ([0-9.]+);", txt)
        assert m and float(m.group(1)) == float(val), name


def _declared():
    txt = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(anet_[A-Za-z0-9_]+)\s*\(", txt))


def test_entry_points_are_declared_exported_and_bound():
    """(4)"""
    import allocnet_amd as aa
    from allocnet_amd import _lib, build
    declared = _declared()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared in the header"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.PROTOTYPES, f"{n} is not in the ctypes table"
    assert "api_separation.hip" in build.SOURCES
    for n in ("traj_separation", "traj_separation_dev"):
        assert callable(getattr(aa, n))
    for n in ("getSeparation", "checkSeparation"):
        assert callable(getattr(aa.Trajectory, n))
    assert not any("separation_workspace" in n for n in declared)
    assert lib.anet_abi_version() == 2


def test_separation_unit_resources():
    """(5) The unit compiles alone for gfx950 with the product's flags; the three instantiations use no scratch, and the registers
    and occupancy DESIGN.md 8n quotes (its resource table is read here)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_separation.hip"), "-o", os.path.join(td, "u.o")],
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
    kernels = {fn: u for fn, u in usage.items() if "k_traj_separation" in fn}
    assert len(kernels) == 3, list(usage)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 8n."):design.index("## 9.")]
    for fn, u in sorted(kernels.items()):
        print(fn, u)
        assert u["ScratchSize"] == 0 and u["LDS"] == 0, (fn, u)
        assert "| %d | %d | %d |" % (u["VGPRs"], u["AGPRs"], u["Occupancy"]) in sec, (fn, u, "DESIGN.md 8n quotes other figures")


def test_cpp_header_compiles_as_cxx14():
    """(6)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_traj_separation.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_facade_logic_on_stubbed_results(monkeypatch):
    """(7) Trajectory.getSeparation / checkSeparation on stubbed results: padding with zero-duration pieces, the cutoff just above
    min_dist, NaN never clear, no common time always clear, different orders refused."""
    import allocnet_amd as aa
    from allocnet_amd import trajectory as tr
    seen = {}

    def stub(coeffs, T, pairs=None, t0=None, cutoff=np.inf, ctx=None):
        seen.update(co=np.array(coeffs), T=np.array(T), pairs=np.array(pairs), t0=np.array(t0), cutoff=cutoff)
        return (np.array([seen["sep"]]), np.array([seen["t"]]), np.array([seen["pieces"]], dtype=np.int32), np.array(pairs))
    monkeypatch.setattr(tr, "traj_separation", stub)
    cm = np.arange(18.0).reshape(3, 6)
    a = aa.Trajectory([0.5, 2.0, 1.0], [cm, cm + 1, cm + 2])
    b = aa.Trajectory([1.5], [cm + 3])
    seen.update(sep=0.75, t=1.25, pieces=[1, 0])
    assert a.getSeparation(b, t0=0.25, other_t0=-1.0) == (0.75, 1.25, 1, 0)
    assert seen["co"].shape == (2, 3, 3, 6) and seen["T"].tolist() == [[0.5, 2.0, 1.0], [1.5, 0.0, 0.0]]
    assert (seen["co"][1, 0] == cm + 3).all() and (seen["co"][1, 1:] == 0.0).all() and (seen["co"][0, 2] == cm + 2).all()
    assert seen["pairs"].tolist() == [[0, 1]] and seen["t0"].tolist() == [0.25, -1.0] and seen["cutoff"] == np.inf
    assert b.getSeparation(a)[2:] == (1, 0) and seen["T"].tolist() == [[1.5, 0.0, 0.0], [0.5, 2.0, 1.0]]
    assert a.checkSeparation(b, 0.75) and a.checkSeparation(b, 0.5) and not a.checkSeparation(b, 0.7500001)
    assert seen["cutoff"] == np.nextafter(0.7500001, np.inf)
    seen.update(sep=np.nan, t=0.0, pieces=[-1, -1])
    assert not a.checkSeparation(b, 0.0) and not a.checkSeparation(b, -1.0) and np.isnan(a.getSeparation(b)[0])
    seen.update(sep=np.inf, t=0.0, pieces=[-1, -1])
    assert a.checkSeparation(b, 1e9) and a.getSeparation(b) == (np.inf, 0.0, -1, -1)
    with pytest.raises(ValueError):
        a.getSeparation(aa.Trajectory([1.0], [np.zeros((3, 8))]))
    assert tr.all_pairs(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and tr.all_pairs(4).dtype == np.int32
    assert tr.all_pairs(1).shape == (0, 2)
