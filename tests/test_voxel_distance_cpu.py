"""The distance field of the voxel map, its query and the obstacle penalty without a GPU: the restatement of tests/dist_np.py against a
separable numpy transform and scipy, its gradients against central differences of its own cost, the ABI plumbing, the unit's
resources and the C++ members."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import dist_np as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("anet_voxel_distance_dev", "anet_voxel_distance_query_dev", "anet_minco_obstacle_partial_grads_dev")


# ---------------------------------------------------------------------------------------------
# the transform
# ---------------------------------------------------------------------------------------------
def _scipy_sd2(vox, walls):
    """scipy's Euclidean transform, both polarities, the squares rounded to integers; walls as a padded layer of blocked voxels."""
    from scipy import ndimage
    blocked = vox != 0
    out = np.empty(vox.shape, dtype=np.int64)
    padded = np.pad(blocked, 1, constant_values=True) if walls else blocked
    if padded.any():
        d = ndimage.distance_transform_edt(~padded)
        d = d[1:-1, 1:-1, 1:-1] if walls else d
        out[~blocked] = np.rint(d * d).astype(np.int64)[~blocked]
    else:
        out[~blocked] = dn.NONE
    if (~blocked).any():
        d = ndimage.distance_transform_edt(blocked)
        out[blocked] = -np.rint(d * d).astype(np.int64)[blocked]
    else:
        out[blocked] = -dn.NONE
    return out


@pytest.mark.parametrize("walls", [0, 1])
@pytest.mark.parametrize("size", [(1, 1, 1), (3, 5, 7), (2, 1, 9), (6, 6, 6)])
def test_restatement_transform_equals_separable_and_scipy(size, walls):
    rng = np.random.default_rng(sum(size) + walls)
    for density in (0.0, 0.05, 0.3, 0.9, 1.0):
        vox = (rng.uniform(size=size) < density).astype(np.uint8) * rng.integers(1, 3, size=size).astype(np.uint8)
        if density == 1.0:
            vox[:] = 1
        brute = dn.brute_sd2(vox, walls)
        assert ((brute > 0) == (vox == 0)).all() and ((brute < 0) == (vox != 0)).all()
        assert np.array_equal(brute, dn.separable_sd2(vox, walls)), (size, density, walls)
        assert np.array_equal(brute, _scipy_sd2(vox, walls)), (size, density, walls)
        if not vox.any():
            assert (brute == dn.NONE).all() if not walls else (brute < dn.NONE).all()
        if vox.all():
            assert (brute == -dn.NONE).all()


def test_layout_helpers_round_trip():
    a = np.arange(2 * 3 * 4).reshape(2, 3, 4)
    f = dn.flat(a)
    assert f[1 + 2 * (2 + 3 * 3)] == a[1, 2, 3] and np.array_equal(dn.unflat(f, (2, 3, 4)), a)


# ---------------------------------------------------------------------------------------------
# the penalty's restatement against central differences
# ---------------------------------------------------------------------------------------------
SIZE, ORIGIN, SCALE = (10, 8, 6), (-1.0, -0.5, 0.0), 0.25


def _map(seed):
    rng = np.random.default_rng(seed)
    vox = (rng.uniform(size=SIZE) < 0.08).astype(np.uint8)
    return vox, dn.brute_sd2(vox, 1)


def _problem(s, seed=5):
    """The issue's shape: N = 3, res = 7 on a 10 x 8 x 6 map at scale 0.25 with 8 % blocked; clearance at the 60th percentile of the
    restatement's d over the samples, mu 0.3 of the spread to the 30th."""
    vox, sd2 = _map(seed)
    rng = np.random.default_rng(100 * seed + s)
    N, res, B, D = 3, 7, 2, 2 * s
    lo, hi = np.array(ORIGIN), np.array(ORIGIN) + SCALE * np.array(SIZE)
    co = rng.normal(size=(B, N, 3, D)) * 0.25 ** (D - 1 - np.arange(D))
    co[..., -1] = rng.uniform(lo + 0.3, hi - 0.3, (B, N, 3))
    T = rng.uniform(0.6, 1.4, (B, N))
    d, off = dn.all_d(co, T, res, sd2, SIZE, ORIGIN, SCALE)
    clearance, mu, frac = dn.limits_from(d)
    return co, T, dict(res=res, w=40.0, mu=mu, clearance=clearance, sd2=sd2, size=SIZE, origin=ORIGIN, scale=SCALE), frac, off


@pytest.mark.parametrize("s", [2, 3, 4])
def test_restatement_gradients_match_central_differences(s):
    """h = 1e-6, bar 2e-5 scaled by max(1, max|g|) (the bar of the avoidance and flatness tests): every T_i and a coefficient of every
    axis.  On the restatement alone: the term is active on 10-90 % of the samples and no sample lies within 1e-4 voxel of a lattice
    plane (the interpolant's gradient jumps there)."""
    co, T, kw, frac, off = _problem(s)
    print(f"s={s}: active on {100 * frac:.1f} % of the samples, nearest lattice plane {off:.3e} voxel away, clearance "
          f"{kw['clearance']:.4f} m, mu {kw['mu']:.4f} m")
    assert 0.1 <= frac <= 0.9 and kw["mu"] > 0.0
    assert off >= 1e-4
    J = lambda c, t: dn.j_obs(c, t, **kw)
    pc, gC, gT = dn.j_obs_grads(co, T, **kw)
    assert np.abs(gT).max() > 0.0 and np.abs(gC).max() > 0.0 and (pc.sum(1) > 0.0).all()
    h = 1e-6

    def check(what, fd, g):
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        print(f"s={s} {what}: fd error {err:.3e} (bar 2e-5), |g| max {np.abs(g).max():.3e}")
        assert err <= 2e-5, (what, err)
    for i in range(T.shape[1]):
        tp, tm = T.copy(), T.copy()
        tp[:, i] += h
        tm[:, i] -= h
        check(f"gdT[{i}]", (J(co, tp) - J(co, tm)) / (2 * h), gT[:, i])
    for (i, ax, col) in [(0, 0, 0), (1, 1, 2 * s - 1), (2, 2, s), (1, 0, 1), (0, 2, 2 * s - 2)]:
        cp, cm = co.copy(), co.copy()
        cp[:, i, ax, col] += h
        cm[:, i, ax, col] -= h
        check(f"gdC[{i},{ax},{col}]", (J(cp, T) - J(cm, T)) / (2 * h), gC[:, i, ax, col])


def test_restatement_query_at_centres_and_beyond():
    """At a centre the interpolant is D(v); beyond the outermost centres it continues as a constant with a zero gradient there; a
    NaN row poisons only itself; a uniform +NONE map gives +inf and a zero gradient."""
    vox, sd2 = _map(5)
    D = dn.centre_values(sd2, SCALE)
    ids = np.stack(np.meshgrid(*[np.arange(n) for n in SIZE], indexing="ij"), -1).reshape(-1, 3)
    centres = np.array(ORIGIN) + 0.5 * SCALE + ids * SCALE               # exact: scale is a power of two
    dist, _ = dn.query(sd2, SIZE, ORIGIN, SCALE, centres)
    assert np.array_equal(dist, D.reshape(-1))
    assert ((dist <= 0.0) == (vox.reshape(-1) != 0)).all()
    out = np.array([[-5.0, 0.3, 0.4], [0.1, 0.3, 9.0], [np.nan, 0.3, 0.4]])
    dist, grad = dn.query(sd2, SIZE, ORIGIN, SCALE, out)
    assert grad[0, 0] == 0.0 and grad[1, 2] == 0.0 and np.isfinite(dist[:2]).all() and grad[0, 1] != 0.0
    assert np.isnan(dist[2]) and np.isnan(grad[2]).all()
    dist, grad = dn.query(np.full(SIZE, dn.NONE), SIZE, ORIGIN, SCALE, out[:2])
    assert (dist == np.inf).all() and (grad == 0.0).all()


# ---------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------
def _declared():
    txt = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return txt, set(re.findall(r"\b(anet_[A-Za-z0-9_]+)\s*\(", txt))


def test_entry_points_are_declared_exported_and_bound():
    import allocnet_amd as aa
    from allocnet_amd import _lib, build
    txt, declared = _declared()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NEW_NAMES, (6, 8, 15)):
        assert name in declared, f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
    assert "api_distance.hip" in build.SOURCES
    assert "api_distance.hip" in open(os.path.join(build.SRC_DIR, "api_internal.h")).read()
    for n in ("make_obstacle_penalty", "minco_obstacle_partial_grads_dev", "minco_obstacle_cost_grad_dev", "minco_obstacle_cost_grad",
              "obstacle_objective_dev", "distance_transform_dev", "distance_query_dev"):
        assert callable(getattr(aa, n)), n
    assert callable(aa.VoxelMap.distance_field) and callable(aa.VoxelMap.getDistance)
    m = re.search(r"typedef struct anet_obstacle_penalty \{(.*?)\} anet_obstacle_penalty;", txt, re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+);", m.group(1))
    ctype = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.ObstaclePenalty._fields_)
    p = aa.make_obstacle_penalty(w=3.0, smooth_mu=0.02, clearance=0.8, res=9)
    assert (p.w, p.smooth_mu, p.clearance, p.res) == (3.0, 0.02, 0.8, 9)
    assert re.search(r"#define ANET_DIST_NONE INT32_MAX", txt) and aa.DIST_NONE == dn.NONE == 2 ** 31 - 1
    assert not any(("distance" in n or "obstacle" in n) and "workspace" in n for n in declared)
    assert lib.anet_abi_version() == 2


# ---------------------------------------------------------------------------------------------
# the unit's resources
# ---------------------------------------------------------------------------------------------
def test_distance_unit_resources():
    """The unit compiles alone for gfx950 with the product's flags; no kernel uses scratch, and the registers, LDS and occupancy are
    the ones DESIGN.md 8p quotes (its resource table is read here).  The axis pass keeps two workgroups per CU: 64 KiB of 160."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_distance.hip"), "-o", os.path.join(td, "u.o")],
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
    assert (count("k_vox_dist_x"), count("k_vox_dist_axis"), count("k_vox_dist_query"), count("k_minco_obstacle")) == (1, 1, 1, 3), \
        list(usage)
    assert len(usage) == 6, list(usage)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 8p."):design.index("## 9.")]
    rows = {m.group(1): m.group(2) for m in re.finditer(r"^\| `(k_[a-z_]+(?:<\d>)?)` (\|.*\|)$", sec, re.M)}
    assert len(rows) == 6, list(rows)
    for fn, u in sorted(usage.items()):
        print(fn, u)
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (fn, u)
        assert u["LDS"] <= 64 * 1024, (fn, u)
        order = re.search(r"k_minco_obstacleILi(\d)E", fn)          # the row of THIS kernel: its name, its template argument
        label = "k_minco_obstacle<%s>" % order.group(1) if order else re.search(r"\d+(k_vox_dist_[a-z]+)E", fn).group(1)
        assert rows[label].startswith("| %d | %d | %d |" % (u["VGPRs"], u["LDS"], u["Occupancy"])), \
            (fn, u, rows[label], "DESIGN.md 8p quotes other figures for this kernel")


def test_cpp_members_compile_as_cxx14():
    """distanceField / getDistance of include/allocnet_amd/voxel_map.hpp build with the reference's language level, without Eigen or
    HIP headers."""
    src = os.path.join(ROOT, "tests", "cpp", "test_voxel_distance.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
