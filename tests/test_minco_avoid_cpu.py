"""The trajectory-avoidance penalty without a GPU: the float64 restatement against central differences of its own cost, the location
rule, the neighbour-list helpers, the ABI plumbing and the unit's resources."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import avoid_np as av

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAME = "anet_minco_avoid_partial_grads_dev"


def _random_set(rng, B, N, s, box=2.0):
    """Random polynomial pieces (not continuous at the knots: the formulas hold piece by piece) that stay near a common box."""
    D = 2 * s
    co = rng.normal(size=(B, N, 3, D)) * 0.3 ** (D - 1 - np.arange(D))
    co[..., -1] = rng.uniform(-box, box, (B, N, 3))
    return co, rng.uniform(0.6, 1.4, (B, N))


def _problem(s, seed=3):
    """The issue's shape: N = 3, No = 4, res = 7, three others with staggered starts (one starts inside the ego's window, one ends
    inside it); limits from the percentiles of q."""
    rng = np.random.default_rng(seed + s)
    N, No, res, B, Bo = 3, 4, 7, 2, 3
    co, T = _random_set(rng, B, N, s)
    oco, oT = _random_set(rng, Bo, No, s)
    t0, ot0 = np.array([0.4, 0.9]), np.array([0.0, 1.3, -2.1])
    start, nbr = np.array([0, 3, 5], dtype=np.int32), np.array([0, 1, 2, 2, 0], dtype=np.int32)
    z_scale = 1.5
    q = av.all_q(co, T, t0, oco, oT, ot0, start, nbr, res, z_scale)
    min_dist, mu, frac = av.limits_from(q)
    assert len(q) >= 50 and 0.1 <= frac <= 0.9 and mu > 0.0
    kw = dict(res=res, w=40.0, mu=mu, min_dist=min_dist, z_scale=z_scale)
    return co, T, t0, oco, oT, ot0, start, nbr, kw


@pytest.mark.parametrize("s", [2, 3, 4])
def test_restatement_gradients_match_central_differences(s):
    """h = 1e-6, bar 2e-5 scaled by max(1, max|g|) (the bar of the flatness finite-difference test): every T_i, t0 and a coefficient
    of every axis."""
    co, T, t0, oco, oT, ot0, start, nbr, kw = _problem(s)
    J = lambda c, t, z: av.j_avoid(c, t, z, oco, oT, ot0, start, nbr, **kw)
    pc, gC, gT, g0 = av.j_avoid_grads(co, T, t0, oco, oT, ot0, start, nbr, **kw)
    assert np.abs(gT).max() > 0.0 and np.abs(gC).max() > 0.0 and np.abs(g0).max() > 0.0 and (pc.sum(1) > 0.0).all()
    h = 1e-6

    def check(what, fd, g):
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        print(f"s={s} {what}: fd error {err:.3e} (bar 2e-5), |g| max {np.abs(g).max():.3e}")
        assert err <= 2e-5, (what, err)
    for i in range(T.shape[1]):
        tp, tm = T.copy(), T.copy()
        tp[:, i] += h
        tm[:, i] -= h
        check(f"gdT[{i}]", (J(co, tp, t0) - J(co, tm, t0)) / (2 * h), gT[:, i])
    check("gd_t0", (J(co, T, t0 + h) - J(co, T, t0 - h)) / (2 * h), g0)
    for (i, ax, col) in [(0, 0, 0), (1, 1, 2 * s - 1), (2, 2, s), (1, 0, 1)]:
        cp, cm = co.copy(), co.copy()
        cp[:, i, ax, col] += h
        cm[:, i, ax, col] -= h
        check(f"gdC[{i},{ax},{col}]", (J(cp, T, t0) - J(cm, T, t0)) / (2 * h), gC[:, i, ax, col])


def test_location_rule_at_a_shared_knot():
    co, T, t0, oco, oT, ot0, start, nbr, kw = av.discontinuous_case()
    K = av.knots(T[0], t0[0])
    _, _, t = av.sample_times(T[0], t0[0], kw["res"])
    assert (t[:, 0] == K[:-1]).all()                                   # j = 0 sits on the knot
    m_at, u = av.locate(t, av.knots(oT[0], ot0[0]))
    assert (m_at == np.arange(3)[:, None]).all() and (u[:, 0] == 0.0).all()
    pc, gC, gT, g0 = av.j_avoid_grads(co, T, t0, oco, oT, ot0, start, nbr, **kw)
    x = 1.2 ** 2 - 0.5 ** 2                                            # > mu: the linear branch
    want = 10.0 * (x - 0.5 * 0.05)
    assert np.allclose(pc[0], [T[0, 0] * want, 0.0, T[0, 2] * want], rtol=1e-14) and pc[0, 1] == 0.0
    # the end of the other is open: an ego sample exactly at L_No sees nothing; a zero-duration piece is never located
    assert av.locate(np.array([K[-1]]), K)[0][0] == -1 and av.locate(np.array([K[0]]), K)[0][0] == 0
    assert av.locate(np.array([1.0]), np.array([0.0, 1.0, 1.0, 2.0]))[0][0] == 2


def test_neighbour_helpers():
    import allocnet_amd as aa
    start, nbr = aa.neighbours_all(3, 4)
    assert start.dtype == np.int32 and nbr.dtype == np.int32
    assert start.tolist() == [0, 4, 8, 12] and nbr.tolist() == [0, 1, 2, 3] * 3
    start, nbr = aa.neighbours_all(4, 4, exclude_self=True)
    assert start.tolist() == [0, 3, 6, 9, 12]
    for b in range(4):
        assert nbr[start[b]:start[b + 1]].tolist() == [o for o in range(4) if o != b]
    start, nbr = aa.neighbours_all(1, 1, exclude_self=True)
    assert start.tolist() == [0, 0] and nbr.size == 0
    pairs = np.array([[0, 1], [0, 2], [1, 2], [3, 4], [2, 2], [1, 0]])
    keep = np.array([True, False, True, True, True, True])
    start, nbr = aa.neighbours_from_pairs(pairs, 6, keep=keep)
    assert start.dtype == np.int32 and nbr.dtype == np.int32 and (np.diff(start) >= 0).all() and start[0] == 0 and start[-1] == len(nbr)
    rows = [nbr[start[b]:start[b + 1]].tolist() for b in range(6)]
    assert rows == [[1], [0, 2], [1], [4], [3], []]                      # symmetric, no self, no repeats, empty rows
    for b, row in enumerate(rows):
        assert all(b in rows[o] for o in row)
    start, nbr = aa.neighbours_from_pairs(np.zeros((0, 2), dtype=np.int32), 3)
    assert start.tolist() == [0, 0, 0, 0] and nbr.size == 0
    every = aa.neighbours_from_pairs(aa.trajectory.all_pairs(5), 5)
    assert all(np.array_equal(a, b) for a, b in zip(every, aa.neighbours_all(5, 5, exclude_self=True)))
    with pytest.raises(ValueError):
        aa.neighbours_from_pairs(np.array([[0, 7]]), 3)


def _declared():
    txt = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return txt, set(re.findall(r"\b(anet_[A-Za-z0-9_]+)\s*\(", txt))


def test_entry_point_is_declared_exported_and_bound():
    import allocnet_amd as aa
    from allocnet_amd import _lib, build
    txt, declared = _declared()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert NEW_NAME in declared, f"{NEW_NAME} is not declared in the header"
    assert hasattr(lib, NEW_NAME), f"{NEW_NAME} is not exported"
    assert NEW_NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NEW_NAME][1]) == 23
    assert "api_avoid.hip" in build.SOURCES
    assert "api_avoid.hip" in open(os.path.join(build.SRC_DIR, "api_internal.h")).read()
    for n in ("make_avoid_penalty", "minco_avoid_partial_grads_dev", "minco_avoid_cost_grad_dev", "minco_avoid_cost_grad",
              "neighbours_all", "neighbours_from_pairs"):
        assert callable(getattr(aa, n)), n
    m = re.search(r"typedef struct anet_avoid_penalty \{(.*?)\} anet_avoid_penalty;", txt, re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+);", m.group(1))
    ctype = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.AvoidPenalty._fields_)
    p = aa.make_avoid_penalty(w=3.0, smooth_mu=0.02, min_dist=0.8, z_scale=1.5, res=9)
    assert (p.w, p.smooth_mu, p.min_dist, p.z_scale, p.res) == (3.0, 0.02, 0.8, 1.5, 9)
    assert not any("avoid" in n and "workspace" in n for n in declared)
    assert lib.anet_abi_version() == 2


def test_avoid_unit_resources():
    """The unit compiles alone for gfx950 with the product's flags; the three instantiations use no scratch, and the registers, LDS
    and occupancy DESIGN.md 8o quotes (its resource table is read here)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_avoid.hip"), "-o", os.path.join(td, "u.o")],
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
    kernels = {fn: u for fn, u in usage.items() if "k_minco_avoid" in fn}
    assert len(kernels) == 3, list(usage)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 8o."):design.index("## 9.")]
    for fn, u in sorted(kernels.items()):
        print(fn, u)
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (fn, u)
        assert u["LDS"] <= 32 * 1024, (fn, u)
        assert "| %d | %d | %d |" % (u["VGPRs"], u["LDS"], u["Occupancy"]) in sec, (fn, u, "DESIGN.md 8o quotes other figures")
