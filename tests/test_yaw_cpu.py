"""Yaw trajectories without a GPU: the ABI plumbing, the restatement of tests/yaw_np.py against central differences of its own cost,
the conditions its test cases must meet, the new unit's resources and the C++ facade."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import yaw_np as yn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = {"anet_minco_solve_scalar_dev": 13, "anet_minco_solve_scalar": 11, "anet_minco_propagate_grad_scalar_dev": 13,
             "anet_minco_yaw_partial_grads_dev": 16, "anet_traj_yaw_margin_dev": 15, "anet_traj_yaw_margin": 13,
             "anet_traj_states_yaw_dev": 14, "anet_traj_states_yaw": 12}
SPEED_EPS = 1e-2

# the shapes of tests/test_yaw_gpu.py (s, sy, N, B, res), and the two of the difference check here
GPU_SHAPES = {"one": (2, 2, 1, 1, 1), "quad": (2, 3, 4, 5, 9), "ragged": (3, 2, 5, 3, 5), "wide": (4, 2, 8, 130, 20),
              "rounds": (3, 4, 16, 2, 64), "top": (4, 4, 2, 2, 3)}
FD_SHAPES = {"case1": (3, 2, 2, 2, 5), "case2": (4, 4, 1, 1, 1)}


def make_case(s, sy, N, B, res, seed):
    """Random position coefficients (the power k scaled by 0.5^k), durations in [0.6, 1.4], the yaw as the heading fit plus noise,
    limits by the percentile rule, w_energy so that the effort is half of the two sampled terms."""
    rng = np.random.default_rng(seed)
    D = 2 * s
    co = rng.normal(size=(B, N, 3, D)) * 0.5 ** (D - 1 - np.arange(D))
    T = rng.uniform(0.6, 1.4, (B, N))
    cy = yn.heading_fit(co, T, sy, rng)
    lim, frac_look, frac_rate = yn.limits_for(co, cy, T, res, SPEED_EPS)
    kw = dict(res=res, w_look=30.0, w_rate=20.0, w_energy=0.0, speed_eps=SPEED_EPS, **lim)
    kw["w_energy"] = yn.energy_weight(co, cy, T, kw)
    return co, cy, T, kw, frac_look, frac_rate


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
    for name, nargs in NEW_NAMES.items():
        assert name in declared, f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
        proto = re.search(r"\bint %s\s*\((.*?)\);" % name, txt, re.S).group(1)
        assert len(proto.split(",")) == nargs, (name, proto)
    assert "api_yaw.hip" in build.SOURCES
    assert "api_yaw.hip" in open(os.path.join(build.SRC_DIR, "api_internal.h")).read()
    for n in ("make_yaw_penalty", "minco_solve_scalar", "minco_solve_scalar_dev", "minco_propagate_grad_scalar_dev",
              "minco_yaw_partial_grads_dev", "minco_yaw_cost_grad", "minco_yaw_cost_grad_dev", "yaw_objective_dev", "traj_yaw_margin",
              "traj_yaw_margin_dev", "traj_flat_states_yaw", "heading_waypoints", "YawTrajectory"):
        assert callable(getattr(aa, n)), n
    assert callable(aa.Trajectory.getYawMargin) and callable(aa.Trajectory.checkYaw)
    m = re.search(r"typedef struct anet_yaw_penalty \{(.*?)\} anet_yaw_penalty;", txt, re.S)
    ctype = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    fields = []
    for t, names in re.findall(r"(double|int32_t)\s+([\w, ]+);", m.group(1)):
        fields += [(n.strip(), ctype[t]) for n in names.split(",")]
    assert fields == list(_lib.YawPenalty._fields_)
    assert [n for n, _ in fields] == ["w_look", "mu_look", "half_fov", "speed_eps", "w_rate", "mu_rate", "max_rate", "w_energy", "res"]
    p = aa.make_yaw_penalty(w_look=3.0, mu_look=0.02, half_fov=0.6, speed_eps=0.01, w_rate=4.0, mu_rate=0.03, max_rate=1.5,
                            w_energy=0.1, res=9)
    assert (p.w_look, p.mu_look, p.half_fov, p.speed_eps, p.w_rate, p.mu_rate, p.max_rate, p.w_energy, p.res) == \
        (3.0, 0.02, 0.6, 0.01, 4.0, 0.03, 1.5, 0.1, 9)
    assert lib.anet_abi_version() == 2


def test_python_helpers():
    """heading_waypoints unwraps along the route; YawTrajectory locates times as Trajectory does."""
    import allocnet_amd as aa
    # a route that turns left through more than pi: the headings keep growing instead of jumping by 2 pi
    ang = np.linspace(0.0, 1.5 * np.pi, 9)
    nodes = np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], 1)
    h0, hw, h1 = aa.heading_waypoints(nodes[1:-1], nodes[0], nodes[-1])
    seq = np.concatenate([[h0], hw, [h1]])
    assert (np.diff(seq) > 0.0).all() and seq[-1] - seq[0] > np.pi
    assert np.allclose(hw, ang[1:-1] + 0.5 * np.pi, atol=1e-12)
    hb = aa.heading_waypoints(np.stack([nodes[1:-1]] * 2), nodes[0], nodes[-1])[1]
    assert hb.shape == (2, 7) and np.array_equal(hb[0], hw)
    cy = np.array([[0.0, 0.0, 2.0, 1.0], [0.0, 0.0, -1.0, 3.0]])
    y = aa.YawTrajectory(cy, [1.0, 2.0])
    assert y.getYaw(0.5) == 2.0 and y.getYaw(1.0) == 3.0 and y.getYaw(1.5) == 2.5 and y.getYaw(4.0) == 0.0
    assert y.getYawRate(0.25) == 2.0 and y.getYawRate(2.0) == -1.0 and np.array_equal(y.getDurations(), [1.0, 2.0])
    psi, dpsi = yn.yaw_eval(cy[None], np.array([[1.0, 2.0]]), np.array([[0.5, 1.0, 1.5, 4.0]]))
    assert np.array_equal(psi[0], [2.0, 3.0, 2.5, 0.0]) and np.array_equal(dpsi[0], [2.0, 2.0, -1.0, -1.0])


# ---------------------------------------------------------------------------------------------
# the restatement against itself
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FD_SHAPES))
def test_restatement_gradients_match_central_differences(name):
    """h = 1e-6, bar 2e-5 scaled by max(1, max|g|), the project's bar for this check: every T_i, every yaw coefficient and every
    position coefficient of piece 0 (the z rows among them: their gradient is exactly zero)."""
    s, sy, N, B, res = FD_SHAPES[name]
    co, cy, T, kw, _, _ = make_case(s, sy, N, B, res, seed=1)
    J = lambda c, y, t: yn.j_yaw(c, y, t, **kw)
    pc, gC, gCy, gT = yn.j_yaw_grads(co, cy, T, **kw)
    assert all(np.abs(x).max() > 0.0 for x in (pc, gC, gCy, gT)) and (gC[:, :, 2] == 0.0).all() and (gC[..., -1] == 0.0).all()
    h, worst = 1e-6, 0.0

    def check(what, fd, g):
        nonlocal worst
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        worst = max(worst, err)
        assert err <= 2e-5, (what, err)
    for i in range(N):
        tp, tm = T.copy(), T.copy()
        tp[:, i] += h
        tm[:, i] -= h
        check(f"gdT[{i}]", (J(co, cy, tp) - J(co, cy, tm)) / (2 * h), gT[:, i])
    for i in range(N):
        for col in range(2 * sy):
            yp, ym = cy.copy(), cy.copy()
            yp[:, i, col] += h
            ym[:, i, col] -= h
            check(f"gdCy[{i},{col}]", (J(co, yp, T) - J(co, ym, T)) / (2 * h), gCy[:, i, col])
    for ax in range(3):
        for col in range(2 * s):
            cp, cm = co.copy(), co.copy()
            cp[:, 0, ax, col] += h
            cm[:, 0, ax, col] -= h
            check(f"gdC[0,{ax},{col}]", (J(cp, cy, T) - J(cm, cy, T)) / (2 * h), gC[:, 0, ax, col])
    print(f"{name}: largest scaled difference {worst:.3e} (bar 2e-5); |gdT| {np.abs(gT).max():.3e}, |gdCy| {np.abs(gCy).max():.3e}, "
          f"|gdC| {np.abs(gC).max():.3e}")


@pytest.mark.parametrize("name", list(GPU_SHAPES) + list(FD_SHAPES))
def test_cases_are_partly_active(name):
    """A condition on the restatement alone: with the yaw a heading fit plus noise and the limits by the percentile rule, each of the
    two sampled terms is active on 10 % to 90 % of the samples of every case the tests use.  A case of ONE sample has no such
    fraction: there both terms hold their sample in the middle of the blend, 0 < g < mu."""
    s, sy, N, B, res = dict(GPU_SHAPES, **FD_SHAPES)[name]
    co, cy, T, kw, frac_look, frac_rate = make_case(s, sy, N, B, res, seed=1)
    print(f"{name}: look active on {100 * frac_look:.1f} %, rate on {100 * frac_rate:.1f} % of {B * N * res} samples; half_fov "
          f"{kw['half_fov']:.4f} rad, mu_look {kw['mu_look']:.4f} m/s, max_rate {kw['max_rate']:.4f} rad/s, mu_rate {kw['mu_rate']:.4f}")
    assert 0.0 < kw["half_fov"] <= 0.5 * np.pi and kw["mu_look"] > 0.0 and kw["mu_rate"] > 0.0 and kw["max_rate"] > 0.0
    if B * N * res >= 2:
        assert 0.1 <= frac_look <= 0.9 and 0.1 <= frac_rate <= 0.9
    else:
        gl, gr = yn.look_rate_g(co[0], cy[0], T[0], res, kw["half_fov"], SPEED_EPS, kw["max_rate"])
        assert 0.0 < gl[0, 0] < kw["mu_look"] and 0.0 < gr[0, 0] < kw["mu_rate"]


def test_inactive_look_samples_are_inside_the_field_of_view():
    """Inactive look samples have h.u >= ca |h|, and the margin is >= 0 on the pieces whose samples j < res with |h| >= v_min are
    all inactive (for those samples: the piece's end is a sample of the margin only)."""
    s, sy, N, B, res = GPU_SHAPES["quad"]
    co, cy, T, kw, _, _ = make_case(s, sy, N, B, res, seed=1)
    g = yn.j_yaw_grads(co, cy, T, parts=True, **kw)[4]
    ca = np.cos(kw["half_fov"])
    for b in range(B):
        _, _, h, _, psi, _, _ = yn.samples(co[b], cy[b], T[b], res)
        hu, hn = h[..., 0] * np.cos(psi) + h[..., 1] * np.sin(psi), np.sqrt((h * h).sum(-1))
        assert (hu[g[b] <= 0.0] >= (ca * hn)[g[b] <= 0.0]).all()
    assert (g <= 0.0).any() and (g > 0.0).any()
    v_min = 0.2
    m, hn = yn.yaw_margin(co, cy, T, res, kw["half_fov"], v_min, per_sample=True)
    counted = hn[..., :-1] >= v_min
    assert (m[..., :-1][counted & (g <= 0.0)] >= 0.0).all()
    margin, t, rate = yn.yaw_margin(co, cy, T, res, kw["half_fov"], v_min)
    # ... so on a piece whose counted samples j < res are all inactive, the margin over those samples is >= 0; the reported margin
    # also looks at the piece's end, j = res, which is no sample of the penalty
    quiet = ((g <= 0.0) | ~counted).all(2) & counted.any(2)
    over_penalty_samples = np.where(counted, m[..., :-1], np.inf).min(2)
    assert (over_penalty_samples[quiet] >= 0.0).all()
    assert (margin <= over_penalty_samples).all()
    assert ((t >= 0.0) & (t <= T)).all() and (rate >= 0.0).all()


def test_restatement_one_axis_minco_is_the_first_axis_of_three():
    """minco_scalar (the dense collocation solve with the yaw in axis 0) meets its conditions: end states, waypoints, continuity."""
    rng = np.random.default_rng(2)
    s, N = 3, 4
    head, tail, wps, T = rng.normal(size=3), rng.normal(size=3), rng.normal(size=N - 1), rng.uniform(0.5, 1.5, N)
    co, energy = yn.minco_scalar(s, head, tail, wps, T)
    assert co.shape == (N, 2 * s) and energy > 0.0
    d0 = lambda c, k: np.polyval(np.polyder(c, k) if k else c, 0.0)
    d1 = lambda c, T_, k: np.polyval(np.polyder(c, k) if k else c, T_)
    for k in range(3):
        assert abs(d0(co[0], k) - head[k]) < 1e-10 and abs(d1(co[-1], T[-1], k) - tail[k]) < 1e-9
    for i in range(N - 1):
        assert abs(d0(co[i + 1], 0) - wps[i]) < 1e-10
        for k in range(2 * s - 1):
            assert abs(d1(co[i], T[i], k) - d0(co[i + 1], k)) < 1e-7 * max(1.0, abs(d0(co[i + 1], k)))


# ---------------------------------------------------------------------------------------------
# the unit's resources
# ---------------------------------------------------------------------------------------------
KERNELS = {"k_minco_yaw": 9, "k_traj_yaw_margin": 9, "k_traj_flat_states_yaw": 9, "k_minco_solve_scalar": 3,
           "k_minco_propagate_scalar": 3}
_usage = {}


def unit_usage():
    """api_yaw.hip compiled alone for gfx950 with the product's flags: {mangled kernel name: figures}."""
    if not _usage:
        from allocnet_amd import build as b
        cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
        with tempfile.TemporaryDirectory() as td:
            res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                       os.path.join(b.SRC_DIR, "api_yaw.hip"), "-o", os.path.join(td, "u.o")],
                                 capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        name = None
        for line in res.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                _usage[name] = {}
            m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and name:
                _usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return _usage


def orders_of(kernel, fn):
    """(S,) or (S, SY) of an instantiation of `kernel`, None for another kernel."""
    m = re.search(r"\d+%sILi(\d)E(?:Li(\d)E)?E" % kernel, fn)
    return tuple(int(x) for x in m.groups() if x is not None) if m else None


def design_rows(kernel):
    """The resource table of `kernel` in DESIGN.md 8w: {orders: the rest of the row}."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 8w."):design.index("## 9.")]
    tab = re.search(r"^\| `%s<[A-Z, ]+>` \|.*\n\|[-| ]+\|\n((?:\|.*\|\n)+)" % kernel, sec, re.M)
    assert tab, f"DESIGN.md 8w has no resource table for {kernel}"
    rows = {}
    for m in re.finditer(r"^\| S = (\d)(?:, SY = (\d))? (\|.*\|)$", tab.group(1), re.M):
        rows[tuple(int(x) for x in m.groups()[:2] if x is not None)] = m.group(3)
    return rows


def test_yaw_unit_resources():
    """api_yaw.hip compiles alone for gfx950 with the product's flags; no kernel uses scratch or AGPRs, LDS stays within 64 KiB, and
    the registers, LDS and occupancy of every kernel are the ones DESIGN.md 8w quotes (its resource tables are read here)."""
    usage = unit_usage()
    count = lambda key: sum(orders_of(key, fn) is not None for fn in usage)
    assert {k: count(k) for k in KERNELS} == KERNELS and len(usage) == sum(KERNELS.values()), list(usage)
    for kernel in KERNELS:
        rows = design_rows(kernel)
        assert len(rows) == KERNELS[kernel], (kernel, rows)
        for fn, u in sorted(usage.items()):
            o = orders_of(kernel, fn)
            if o is None:
                continue
            print(fn, u)
            assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (fn, u)
            assert u["LDS"] <= 64 * 1024, (fn, u)
            assert rows[o].startswith("| %d | %d | %d | %d | %d |" % (u["VGPRs"], u["LDS"], u["Occupancy"], u["AGPRs"], u["ScratchSize"])), \
                (fn, u, rows[o], "DESIGN.md 8w quotes other figures for this kernel")


def test_cpp_facade_compiles_as_cxx14():
    """include/allocnet_amd/yaw.hpp and tests/cpp/test_yaw.cpp build with the reference's language level, without Eigen or HIP
    headers."""
    src = os.path.join(ROOT, "tests", "cpp", "test_yaw.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
