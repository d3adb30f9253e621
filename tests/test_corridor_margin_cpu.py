"""Exact corridor / box-limit margins without a GPU: the multiprecision reference (tests/corridor_margin_mp.py) against facts that
do not depend on it; a float64 restatement of the kernel's procedure, pruning included, against the reference on every golden
case at the a-priori bound; conditions on the golden generator that the GPU test relies on; the new unit's resources; the
new entry points declared, exported and bound."""
import ctypes
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction as Fr

import numpy as np
import pytest

from tests import corridor_margin_mp as cmm
from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["anet_traj_row_margin", "anet_traj_row_margin_dev"]
EPS = cmm.EPS
SLACK, MAX_DEPTH, MAX_NODES, BISECT = cmm.MARGIN_SLACK, cmm.MARGIN_DEPTH, cmm.MARGIN_MAX_NODES, cmm.MARGIN_BISECT
margin_float64 = cmm.margin_float64


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "corridor_margin_cases.npz"))


# ---- the reference against facts that do not depend on it ---------------------------------------------------
def test_reference_constant_velocity_against_a_plane():
    """p(t) = p0 + v t: a . p - b is linear, its maximum is at the end the velocity points to, in closed form."""
    for s in (2, 3, 4):
        cm = np.zeros((3, 2 * s))
        cm[:, -1] = [0.5, -1.0, 2.0]
        cm[:, -2] = [1.0, 0.25, -0.5]
        T = 1.5
        for a, want_tau in (([1.0, 0.0, 0.0], 1), ([0.0, 0.0, 1.0], 0)):
            m, r, tau, _ = cmm.piece_margin_mp(cm, T, 0, [a + [0.75]])
            end = cm[:, -1] + cm[:, -2] * (T if want_tau else 0.0)
            assert r == 0 and tau == want_tau and m == Fr(float(np.dot(a, end))) - Fr(0.75)
        # its velocity is constant: the margin of v_x <= 0.75 is 0.25 everywhere, of the acceleration rows -b
        assert cmm.piece_margin_mp(cm, T, 1, [[1.0, 0.0, 0.0, 0.75]])[0] == Fr(1, 4)
        assert cmm.piece_margin_mp(cm, T, 2, [[1.0, 0.0, 0.0, 0.75]])[0] == Fr(-3, 4)


def test_reference_parabola_apex():
    """z(t) = 3 t - 2 t^2 on [0, 1.5]: apex 9/8 at t = 3/4; against z <= 1 the margin is 1/8 at tau = 1/2."""
    cm = np.zeros((3, 4))
    cm[2, 1], cm[2, 2] = -2.0, 3.0
    m, r, tau, _ = cmm.piece_margin_mp(cm, 1.5, 0, [[0, 0, 0, 0], [0.0, 0.0, 1.0, 1.0]])
    assert r == 1 and abs(m - Fr(1, 8)) < 1e-50 and abs(tau - Fr(1, 2)) < 1e-50
    assert cmm.piece_margin_mp(cm, 1.5, 0, np.zeros((3, 4)))[:2] == (-cmm.mpmath.inf, -1)


def test_reference_is_never_below_exact_samples(fx):
    """At 400 rational times the exact g of every row is at most the reference margin (every 7th case: exact arithmetic)."""
    for i in range(0, len(fx["T"]), 7):
        s, d = int(fx["s"][i]), int(fx["d"][i])
        cm, T, rows = fx["cm"][i][:, :2 * s], fx["T"][i], fx["rows"][i]
        u = cmm.deriv_exact(cm, T, d)
        ref = cmm.piece_margin_mp(cm, T, d, rows)[0]
        for row in rows:
            if cmm.is_padding(row):
                continue
            g = cmm.row_poly_exact(u, row)
            top = max(cmm._pval(g, Fr(j, 399)) for j in range(400))
            assert cmm._mpf(top) <= ref + cmm.mpmath.mpf(10) ** -50 * (1 + abs(ref)), (i, float(top), float(ref))


def test_golden_file_is_what_the_generator_writes(fx):
    """Spot check: the stored reference of every 11th case is recomputed (the whole file: make_corridor_margin_golden --check)."""
    for i in range(0, len(fx["T"]), 11):
        s, d = int(fx["s"][i]), int(fx["d"][i])
        m, r, tau, _ = cmm.piece_margin_mp(fx["cm"][i][:, :2 * s], fx["T"][i], d, fx["rows"][i])
        assert float(m) == fx["ref"][i] and r == fx["ref_row"][i]
        sc = cmm.row_scales(fx["cm"][i][:, :2 * s], fx["T"][i], d, fx["rows"][i])
        assert (sc.max() if len(sc) else 0.0) == fx["scale"][i]


# ---- the kernel's procedure in float64 ------------------------------------------------------------------------
def test_float64_restatement_meets_the_bound_on_every_case(fx):
    worst = {}
    stats = {}
    for i in range(len(fx["T"])):
        s, d = int(fx["s"][i]), int(fx["d"][i])
        cm, T, rows = fx["cm"][i][:, :2 * s], float(fx["T"][i]), fx["rows"][i]
        got, row, t = margin_float64(cm, T, d, rows, stats=stats)
        ref, bound = fx["ref"][i], float(cmm.margin_bound(fx["scale"][i]))
        fam = str(fx["family"][i])
        if fam == "empty":
            assert got == -math.inf and row == -1 and t == 0.0 and ref == -math.inf
            continue
        ratio = abs(got - ref) / bound
        worst[fam] = max(worst.get(fam, 0.0), ratio)
        assert ratio <= 1.0, (i, fam, s, d, got, ref, ratio)
        # pruning never changes the result by more than the tolerance (here: compare with the unpruned procedure)
        assert abs(margin_float64(cm, T, d, rows, prune=False)[0] - ref) <= bound
        assert 0.0 <= t <= T and abs(cmm.g_float64(cm, T, d, rows[row], t) - got) <= bound
        if fx["gap"][i] > 4.0 * bound:
            assert row == fx["ref_row"][i], (i, fam, row, fx["ref_row"][i])
    print("worst |err| / bound per family:", {k: round(v, 4) for k, v in worst.items()}, stats)
    assert stats["pruned"] > 50      # the pruning rule is exercised, not bypassed


def test_between_cases_are_invisible_to_the_samples(fx):
    sel = np.flatnonzero(fx["family"] == "between")
    assert len(sel) >= 20
    for i in sel:
        s, d = int(fx["s"][i]), int(fx["d"][i])
        cm, T = fx["cm"][i][:, :2 * s], float(fx["T"][i])
        top = max(cmm.g_float64(cm, T, d, row, j * T / 20.0) for j in range(21) for row in fx["rows"][i]
                  if not cmm.is_padding(row))
        assert top <= 0.0 < fx["ref"][i], (i, top, fx["ref"][i])
        frac = fx["ref_tau"][i] * 20.0
        assert 0.05 < frac - math.floor(frac) < 0.95


def test_generator_keeps_the_row_assertion_meaningful(fx):
    """Outside multi and flat at least 90 % of the cases have a gap above four bounds; every (s, d) has every family it can."""
    sel = ~np.isin(fx["family"], ["multi", "flat", "empty"])
    frac = np.mean(fx["gap"][sel] > 4.0 * cmm.margin_bound(fx["scale"][sel]))
    assert frac >= 0.9, frac
    multi = fx["family"] == "multi"
    assert (np.abs(fx["gap"][multi]) <= cmm.margin_bound(fx["scale"][multi])).all()
    for s in (2, 3, 4):
        for d in (0, 1, 2):
            fams = set(fx["family"][(fx["s"] == s) & (fx["d"] == d)])
            want = {"inside", "endpoint", "flat", "cheb", "multi", "pad", "empty"}
            if 2 * s - 1 - d >= 2:
                want |= {"interior", "graze", "between"}
            assert fams == want, (s, d, fams ^ want)
    inside = fx["family"] == "inside"
    assert (fx["ref"][inside] < -0.5).all()


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
    assert "api_margin.hip" in build.SOURCES
    for n in ("traj_row_margin", "traj_qp_margins"):
        assert callable(getattr(aa, n))
    for n in ("getCorridorMargin", "checkCorridor", "checkBoxLimits"):
        assert callable(getattr(aa.Trajectory, n))
    assert callable(aa.Piece.getCorridorMargin)


def test_kernel_constants_match_the_restatement():
    txt = open(os.path.join(ROOT, "allocnet_amd", "csrc", "corridor_margin_kernels.h")).read()
    for name, val in (("kMarginMaxDepth", MAX_DEPTH), ("kMarginMaxNodes", MAX_NODES), ("kMarginBisect", BISECT),
                      ("kMarginSlack", SLACK)):
        m = re.search(name + r" = ([0-9.]+);", txt)
        assert m and float(m.group(1)) == float(val), name


def test_margin_unit_resources():
    """The unit compiles for gfx950 with the product's flags; the three instantiations use no scratch and no LDS and the
    registers DESIGN.md 8k quotes (its resource table is read here; 4 / 3 / 2 waves per SIMD for S = 2 / 3 / 4)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_margin.hip"), "-o", os.path.join(td, "u.o")],
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
    kernels = {fn: u for fn, u in usage.items() if "k_traj_row_margin" in fn}
    assert len(kernels) == 3, list(usage)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for fn, u in sorted(kernels.items()):
        print(fn, u)
        assert u["ScratchSize"] == 0 and u["LDS"] == 0 and u["AGPRs"] == 0, (fn, u)
        assert u["VGPRs"] <= 192 and u["Occupancy"] >= 2, (fn, u)
        assert "| %d | %d |" % (u["VGPRs"], u["Occupancy"]) in design, (fn, u, "DESIGN.md 8k quotes other figures")
