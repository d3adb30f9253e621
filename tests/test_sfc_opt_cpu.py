"""CPU suite of the vertex parametrisation of corridor waypoints: the numpy restatement (tests/sfc_np.py) against facts -- hull
membership, convex weights, central differences, exact zeros in padded slots, the norm term --, the composed CPU objective
against central differences, the inputs of the GPU tests (depths and vertex counts of every overlap, so a changed generator cannot
silently empty them), and the compile checks of the new unit and of the C++ header."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
from scipy.spatial import HalfspaceIntersection

from tests import polytope_np as pnp
from tests import sfc_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEN = dict(rho=50.0, w_corridor=1e3, w_vel=10.0, w_acc=10.0, smooth_mu=1e-2, max_vel=3.0, max_acc=4.0, res=8)


def _qhull(pair):
    depth, x = pnp.interior(pair)
    n, d, _ = pnp.unit_rows(pair)
    return depth, pnp.merge(HalfspaceIntersection(np.c_[n, d], x).intersections)


@pytest.fixture(scope="module")
def overlaps():
    """Per input: (head, tail, wps, T, hp), the stacked raw pairs, and per (b, w) the Chebyshev depth and the Qhull vertices."""
    out = {}
    for seed, B, N, M in sfc_np.INPUTS:
        prob = sfc_np.corridor(seed, B, N, M)
        st = sfc_np.stacked_raw(prob[4])
        out[seed] = (prob, st, [[_qhull(st[b, w]) for w in range(N - 1)] for b in range(B)])
    return out


def test_inputs_keep_their_depths_and_counts(overlaps):
    for seed, B, N, M in sfc_np.INPUTS:
        prob, st, dv = overlaps[seed]
        depth = np.array([[dv[b][w][0] for w in range(N - 1)] for b in range(B)])
        count = np.array([[len(dv[b][w][1]) for w in range(N - 1)] for b in range(B)])
        outside = np.array([[sfc_np.row_violation(st[b, w], prob[2][b, w]) > 0.0 for w in range(N - 1)] for b in range(B)])
        print(seed, depth.min(), count.max(), outside.mean())
        assert depth.min() >= sfc_np.MIN_DEPTH
        assert count.max() == sfc_np.MAX_COUNT[seed] and count.max() <= sfc_np.K_OF[seed] and count.min() >= 4
        assert 0.015 <= outside.mean() <= 0.04          # the generator's waypoints that exercise backward_p's residual


def test_forward_lies_in_the_hull_of_qhull_vertices(overlaps):
    rng = np.random.default_rng(3)
    for seed, B, N, M in sfc_np.INPUTS:
        _, st, dv = overlaps[seed]
        K = sfc_np.K_OF[seed]
        for b in range(0, B, 4):
            for w in range(N - 1):
                v = dv[b][w][1]
                verts, count = sfc_np.pack_vertices([v], K)
                xi = np.zeros(K)
                xi[:count[0]] = rng.normal(size=count[0]) * rng.choice([1e-3, 1.0, 30.0])
                P, S = sfc_np.forward(xi, verts[0])
                assert sfc_np.row_violation(st[b, w], P) <= 1e-12, (seed, b, w)


def test_sqrt_of_convex_weights_reproduces_the_combination():
    rng = np.random.default_rng(4)
    for k in range(2, 33):
        v = rng.normal(size=(k, 3)) * 5.0
        lam = rng.uniform(size=k); lam /= lam.sum()
        P, S = sfc_np.forward(np.sqrt(lam) * rng.choice([-1.0, 1.0], size=k), v)
        assert np.abs(P - lam @ v).max() <= 1e-15 * 16 and abs(S - 1.0) <= 1e-15


def test_gradient_matches_central_differences_and_padded_slots_are_zero():
    rng = np.random.default_rng(5)
    h = 1e-6
    for k in range(2, 33):
        K = k + 5
        v = np.zeros((K, 3)); v[:k] = rng.normal(size=(k, 3)) * 3.0
        xi = np.zeros(K); xi[:k] = rng.normal(size=k)
        a = rng.normal(size=3); c = rng.normal(size=3)
        J = lambda x: float(np.sin(sfc_np.forward(x, v)[0] @ a) + ((sfc_np.forward(x, v)[0] - c) ** 2).sum())
        P, _ = sfc_np.forward(xi, v)
        g = sfc_np.backward(xi, v, np.cos(P @ a) * a + 2.0 * (P - c))
        fd = np.array([(J(xi + h * e) - J(xi - h * e)) / (2 * h) for e in np.eye(K)[:k]])
        assert np.abs(fd - g[:k]).max() <= 1e-7 * max(1.0, np.abs(g).max()), k
        assert (g[k:] == 0.0).all() and (sfc_np.backward(xi, v, a, w_norm=1.0)[k:] == 0.0).all()


def test_norm_term_is_zero_inside_the_unit_ball_and_its_gradient_matches():
    rng = np.random.default_rng(6)
    h = 1e-6
    for scale in (0.2, 0.99, 1.0):
        xi = rng.normal(size=12); xi *= scale / np.linalg.norm(xi)
        f, g = sfc_np.norm_term(xi, 1.0)
        assert f == 0.0 and (g == 0.0).all()
    for scale in (1.3, 2.0, 6.0):
        xi = rng.normal(size=12); xi *= scale / np.linalg.norm(xi)
        f, g = sfc_np.norm_term(xi, 0.7)
        assert f > 0.0
        fd = np.array([(sfc_np.norm_term(xi + h * e, 0.7)[0] - sfc_np.norm_term(xi - h * e, 0.7)[0]) / (2 * h) for e in np.eye(12)])
        assert np.abs(fd - g).max() <= 1e-7 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("s,seed,N", [(3, 7, 3), (4, 1, 8)])
def test_composed_cpu_objective_matches_central_differences(overlaps, s, seed, N):
    """forward -> oracle/minco_costgrad.c -> backward in (xi, tau).  Bound: the project's finite-difference bar for the cost +
    gradient kernels (tests/test_grad_gpu.py: h = 1e-6, 2e-5 max(1, |g|)): the rounding of a cost of 1e3..1e5 over 2 h and the
    h^2 truncation term both stay below it."""
    (head, tail, wps, T, hp), st, dv = overlaps[seed]
    b, K = 2, sfc_np.K_OF[seed]
    verts, count = sfc_np.pack_vertices([dv[b][w][1] for w in range(N - 1)], K)
    rng = np.random.default_rng(8)
    xi = np.zeros((N - 1, K))
    for w in range(N - 1):
        xi[w, :count[w]] = rng.uniform(0.2, 1.0, size=count[w]) * 0.45      # S > 1 for the larger counts: the norm term is live
    f = sfc_np.Composed(s, head[b], tail[b], hp[b], verts, PEN, w_norm=1.0)
    x = np.concatenate([xi.ravel(), sfc_np.backward_T(T[b])])
    f0, g = f(x)
    assert np.isfinite(f0) and any(np.square(xi[w]).sum() > 1.0 for w in range(N - 1))
    h = 1e-6
    idx = [i for i in rng.choice(len(x) - N, size=12, replace=False)] + list(range(len(x) - N, len(x)))
    for i in idx:
        e = np.zeros(len(x)); e[i] = h
        fd = (f(x + e)[0] - f(x - e)[0]) / (2 * h)
        assert abs(fd - g[i]) <= 2e-5 * max(1.0, np.abs(g).max()), (i, fd, g[i])
    pad = np.array([[j >= count[w] for j in range(K)] for w in range(N - 1)]).ravel()
    assert (g[:len(pad)][pad] == 0.0).all()


def test_cpp_sfc_program_compiles_as_cxx14():
    src = os.path.join(ROOT, "tests", "cpp", "test_sfc_opt.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_sfc_workspaces_carve_without_overlap_under_sanitizers(tmp_path):
    """tests/cpp/test_sfc_workspace_layout.cpp, a stand-alone program over csrc/workspace.h alone, built with the host compiler
    under AddressSanitizer and UBSan and run as an ordinary executable: the three new layouts against the sizes the library's
    anet_sfc_*workspace() functions return."""
    import ctypes
    from allocnet_amd import _lib
    lib = _lib.load()
    exe = str(tmp_path / "test_sfc_workspace_layout")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                          os.path.join(ROOT, "tests", "cpp", "test_sfc_workspace_layout.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = []
    for s, N, K, ld, m, past in [(3, 2, 16, 65, 8, 3), (3, 3, 24, 1, 8, 3), (4, 4, 32, 72, 8, 0), (4, 8, 32, 264, 6, 5), (2, 16, 8, 7, 20, 1)]:
        prm = _lib.LbfgsParams()
        lib.anet_lbfgs_default_params(ctypes.byref(prm))
        prm.mem_size, prm.past = m, past
        want = lib.anet_sfc_workspace(s, N, K, ld, ctypes.cast(ctypes.pointer(prm), ctypes.c_void_p))
        assert want > 0
        lines.append("sfc %d %d %d %d %d %d %d" % (s, N, K, ld, m, past, want))
    for N, B, M, K in [(2, 1, 8, 16), (3, 65, 12, 24), (8, 257, 16, 32), (8, 65, 16, 8), (5, 3, 50, 5)]:
        lines.append("sfc_overlap %d %d %d %d %d" % (N, B, M, K, lib.anet_sfc_overlap_workspace(N, B, M, K)))
    for N, K, ld in [(2, 16, 1), (3, 24, 72), (8, 32, 264), (16, 3, 5)]:
        lines.append("sfc_backward_p %d %d %d %d" % (N, K, ld, lib.anet_sfc_backward_p_workspace(N, K, ld)))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert " 0 failures" in res.stdout


def test_sfc_kernels_use_no_scratch_memory():
    """The new unit compiled for gfx950 with the product's flags: the transform kernels and the tiny NLS keep everything in
    registers (the figures are recorded in DESIGN.md 8j and printed here)."""
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
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    for want in ("k_sfc_forward_p", "k_sfc_backward_grad", "k_sfc_tiny_nls"):
        hit = {fn: u for fn, u in usage.items() if want in fn}
        assert len(hit) == 1, (want, list(usage))
        for fn, u in hit.items():
            print(fn, u)
            assert u["ScratchSize"] == 0, (fn, u)
    assert all(u["ScratchSize"] == 0 for fn, u in usage.items() if "k_sfc_" in fn), usage
