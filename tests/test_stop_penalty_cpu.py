"""Stop within known space without a GPU: the ABI plumbing, the restatement of tests/stop_np.py against central differences of its own
cost and against the obstacle term it degenerates to, the new unit's resources and the C++ members."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import dist_np as dn
from tests import stop_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("anet_minco_stop_partial_grads_dev", "anet_traj_stop_margin_dev", "anet_traj_stop_margin")


# ---------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    import allocnet_amd as aa
    from allocnet_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(anet_[A-Za-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NEW_NAMES, (15, 15, 13)):
        assert name in declared, f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
        proto = re.search(r"\bint %s\s*\((.*?)\);" % name, txt, re.S).group(1)
        assert len(proto.split(",")) == nargs, (name, proto)
    assert "api_stop.hip" in build.SOURCES
    assert "api_stop.hip" in open(os.path.join(build.SRC_DIR, "api_internal.h")).read()
    for n in ("make_stop_penalty", "minco_stop_partial_grads_dev", "minco_stop_cost_grad_dev", "minco_stop_cost_grad",
              "stop_objective_dev", "traj_stop_margin_dev", "traj_stop_margin", "traj_stop_check"):
        assert callable(getattr(aa, n)), n
    assert callable(aa.Trajectory.getStopMargin) and callable(aa.Trajectory.checkStoppable)
    m = re.search(r"typedef struct anet_stop_penalty \{(.*?)\} anet_stop_penalty;", txt, re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+);", m.group(1))
    ctype = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.StopPenalty._fields_)
    assert [n for _, n in fields] == ["w", "smooth_mu", "clearance", "a_brake", "t_react", "speed_eps", "res"]
    p = aa.make_stop_penalty(w=3.0, smooth_mu=0.02, clearance=0.8, a_brake=4.0, t_react=0.2, speed_eps=0.01, res=9)
    assert (p.w, p.smooth_mu, p.clearance, p.a_brake, p.t_react, p.speed_eps, p.res) == (3.0, 0.02, 0.8, 4.0, 0.2, 0.01, 9)
    assert not any("stop" in n and "workspace" in n for n in declared)
    assert lib.anet_abi_version() == 2


# ---------------------------------------------------------------------------------------------
# the restatement against itself
# ---------------------------------------------------------------------------------------------
SIZE, ORIGIN, SCALE = (9, 7, 5), (-1.0, -0.5, 0.0), 0.25


def _problem(t_react, seed=3):
    """N = 2, s = 3, res = 5 on a 9 x 7 x 5 field at scale 0.25 with 8 % blocked and walls; the trajectories are drawn again until no
    sample lies within 1e-4 voxel of a lattice plane; clearance and mu by the percentile rule of dist_np.limits_from on
    d - t_react s_eps - v.v / (2 a_brake)."""
    rng = np.random.default_rng(seed)
    vox = (rng.uniform(size=SIZE) < 0.08).astype(np.uint8)
    sd2 = dn.brute_sd2(vox, 1)
    B, N, s, res = 2, 2, 3, 5
    D = 2 * s
    a_brake, speed_eps = 2.0, 1e-2
    lo, hi = np.array(ORIGIN), np.array(ORIGIN) + SCALE * np.array(SIZE)
    f = dict(sd2=sd2, size=SIZE, origin=ORIGIN, scale=SCALE)
    for _ in range(200):
        co = rng.normal(size=(B, N, 3, D)) * 0.25 ** (D - 1 - np.arange(D))
        co[..., -1] = rng.uniform(lo + 0.3, hi - 0.3, (B, N, 3))
        T = rng.uniform(0.6, 1.4, (B, N))
        d, off = dn.all_d(co, T, res, **f)
        if off >= 1e-4:
            break
    vv = np.concatenate([(dn.sample_points(co[b], T[b], res)[3] ** 2).sum(-1).reshape(-1) for b in range(B)])
    eff = d - sn.stop_distance(vv, a_brake, t_react, np.sqrt(vv + speed_eps ** 2))
    clearance, mu, frac = dn.limits_from(eff)
    kw = dict(res=res, w=40.0, mu=mu, clearance=clearance, a_brake=a_brake, t_react=t_react, speed_eps=speed_eps, **f)
    return co, T, kw, frac, off


@pytest.mark.parametrize("t_react", [0.0, 0.15])
def test_restatement_gradients_match_central_differences(t_react):
    """h = 1e-6, bar 2e-5 scaled by max(1, max|g|) (the bar of the obstacle term's restatement): every T_i and a coefficient of every
    axis, the velocity's own coefficient (k = 1) among them.  On the restatement alone: active on 10-90 % of the samples, no sample
    within 1e-4 voxel of a lattice plane, a G share that is not zero."""
    co, T, kw, frac, off = _problem(t_react)
    print(f"t_react={t_react}: active on {100 * frac:.1f} % of the samples, nearest lattice plane {off:.3e} voxel away, clearance "
          f"{kw['clearance']:.4f} m, mu {kw['mu']:.4f} m")
    assert 0.1 <= frac <= 0.9 and kw["mu"] > 0.0 and off >= 1e-4
    J = lambda c, t: sn.j_stop(c, t, **kw)
    pc, gC, gT, gC_G, _ = sn.j_stop_grads(co, T, parts=True, **kw)
    assert np.abs(gT).max() > 0.0 and np.abs(gC).max() > 0.0 and (pc.sum(1) > 0.0).all() and np.abs(gC_G).max() > 0.0
    assert (gC_G[..., -1] == 0.0).all()                                   # the constant coefficient has no velocity share
    h = 1e-6

    def check(what, fd, g):
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        print(f"{what}: fd error {err:.3e} (bar 2e-5), |g| max {np.abs(g).max():.3e}")
        assert err <= 2e-5, (what, err)
    for i in range(T.shape[1]):
        tp, tm = T.copy(), T.copy()
        tp[:, i] += h
        tm[:, i] -= h
        check(f"gdT[{i}]", (J(co, tp) - J(co, tm)) / (2 * h), gT[:, i])
    for (i, ax, col) in [(0, 0, 0), (1, 1, 5), (1, 2, 3), (0, 1, 4), (1, 0, 1), (0, 2, 4)]:
        cp, cm = co.copy(), co.copy()
        cp[:, i, ax, col] += h
        cm[:, i, ax, col] -= h
        check(f"gdC[{i},{ax},{col}]", (J(cp, T) - J(cm, T)) / (2 * h), gC[:, i, ax, col])


def test_restatement_degenerates_to_the_obstacle_term():
    """a_brake = inf, t_react = 0: the same numbers as dist_np.j_obs_grads, exactly."""
    co, T, kw, _, _ = _problem(0.0)
    kw = dict(kw, a_brake=np.inf, t_react=0.0)
    obs = {k: v for k, v in kw.items() if k not in ("a_brake", "t_react", "speed_eps")}
    for got, ref in zip(sn.j_stop_grads(co, T, **kw), dn.j_obs_grads(co, T, **obs)):
        assert np.abs(ref).max() > 0.0 and np.array_equal(got, ref)
    # ... and it dominates it otherwise
    kw = dict(kw, a_brake=2.0)
    assert (sn.j_stop(co, T, **kw) > dn.j_obs(co, T, **obs)).all()


def test_restatement_margin_agrees_with_the_penalty_samples():
    """Where the penalty's g <= 0 the sampled margin at that sample is >= 0 (s_eps >= |v|), and the margin's diagnostics reproduce it."""
    co, T, kw, _, _ = _problem(0.15)
    g = sn.j_stop_grads(co, T, parts=True, **kw)[4]
    f = {k: kw[k] for k in ("sd2", "size", "origin", "scale")}
    arg = dict(res=kw["res"], clearance=kw["clearance"], a_brake=kw["a_brake"], t_react=kw["t_react"], **f)
    m = sn.stop_margin(co, T, per_sample=True, **arg)
    assert (g <= 0.0).any() and (g > 0.0).any()
    assert (m[..., :-1][g <= 0.0] >= 0.0).all()
    margin, t, speed, dist = sn.stop_margin(co, T, **arg)
    assert np.array_equal(margin, m.min(2))
    assert np.allclose(margin, dist - kw["clearance"] - kw["t_react"] * speed - speed ** 2 / (2 * kw["a_brake"]), rtol=0, atol=1e-14)
    assert ((t >= 0.0) & (t <= T)).all()


# ---------------------------------------------------------------------------------------------
# the unit's resources
# ---------------------------------------------------------------------------------------------
def test_stop_unit_resources():
    """api_stop.hip compiles alone for gfx950 with the product's flags; no kernel uses scratch or AGPRs, LDS stays within 64 KiB, and
    the registers, LDS and occupancy are the ones DESIGN.md 8v quotes (its resource tables are read here)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_stop.hip"), "-o", os.path.join(td, "u.o")],
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
    count = lambda key: sum(key in fn for fn in usage)
    assert (count("k_minco_stop"), count("k_traj_stop_margin")) == (3, 3) and len(usage) == 6, list(usage)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 8v."):design.index("## 9.")]
    for kernel in ("k_minco_stop", "k_traj_stop_margin"):
        # the table of this kernel: its header row names it with <S>, its rows begin with the order
        tab = re.search(r"^\| `%s<S>` \|.*\n\|[-| ]+\|\n((?:\|.*\|\n)+)" % kernel, sec, re.M)
        assert tab, f"DESIGN.md 8v has no resource table for {kernel}"
        rows = {int(m.group(1)): m.group(2) for m in re.finditer(r"^\| S = (\d) (\|.*\|)$", tab.group(1), re.M)}
        assert sorted(rows) == [2, 3, 4], (kernel, rows)
        for fn, u in sorted(usage.items()):
            order = re.search(r"%sILi(\d)E" % kernel, fn)
            if not order:
                continue
            print(fn, u)
            assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (fn, u)
            assert u["LDS"] <= 64 * 1024, (fn, u)
            assert rows[int(order.group(1))].startswith("| %d | %d | %d |" % (u["VGPRs"], u["LDS"], u["Occupancy"])), \
                (fn, u, rows[int(order.group(1))], "DESIGN.md 8v quotes other figures for this kernel")


def test_cpp_members_compile_as_cxx14():
    """getStopMargin / checkStoppable of include/allocnet_amd/trajectory_map.hpp build with the reference's language level, without
    Eigen or HIP headers."""
    src = os.path.join(ROOT, "tests", "cpp", "test_stop_margin.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
