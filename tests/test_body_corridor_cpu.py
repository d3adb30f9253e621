"""CPU suite for the whole-body corridor terms: the restatement of tests/body_np.py against facts that do not depend on it, the
structure of the C ABI (header, ctypes table, build list, struct layout) and the host-side helpers.  Nothing here needs a GPU."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import body_np as bnp
from tests import flatness_np as fnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hover(pos, B=1, N=1, D=8):
    """pieces that stand still at pos"""
    co = np.zeros((B, N, 3, D))
    co[..., D - 1] = pos
    return co, np.ones((B, N))


def test_restatement_at_hover_is_the_translated_body():
    """v = a = j = 0: the attitude is the identity and the terms are a_r . (p + b_k) - h_r"""
    rng = np.random.default_rng(1)
    pos = np.array([0.3, -1.2, 2.0])
    co, T = _hover(pos)
    verts = rng.normal(size=(5, 3))
    hp = rng.normal(size=(1, 1, 4, 4))
    g = bnp.terms(co, T, hp, verts, 3)[0].numpy()
    ref = np.einsum("mx,kx->mk", hp[0, 0, :, :3], pos + verts) - hp[0, 0, :, 3][:, None]
    assert np.abs(g[0, 0] - ref[None]).max() <= 1e-14


def test_restatement_rolls_the_plate_with_the_acceleration():
    """A piece that accelerates sideways at g tan(40 deg) without drag is rolled by 40 degrees about x.  Along the normal of a slab
    tilted by the same angle the rolled plate (half extents 0.25, 0.25, 0.05) reaches only its half thickness, 0.05; level it
    reaches 0.25 sin(40 deg) + 0.05 cos(40 deg) = 0.199."""
    th = math.radians(40.0)
    D = 8
    co = np.zeros((1, 1, 3, D))
    co[0, 0, 1, D - 3] = -0.5 * 9.8 * math.tan(th)          # y(t) = -1/2 g tan(th) t^2: thrust direction (0, -sin, cos)
    T = np.ones((1, 1))
    n = np.array([0.0, -math.sin(th), math.cos(th)])        # the slab's normal = the body z axis
    hp = np.zeros((1, 1, 2, 4))
    hp[0, 0, 0, :3], hp[0, 0, 1, :3] = n, -n
    plate = np.array([[sx * 0.25, sy * 0.25, sz * 0.05] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    par = dict(fnp.LAUNCH, dh=0.0, cp=0.0)
    g = bnp.terms(co, T, hp, plate, 1, **par)[0].numpy()[0, 0, 0]       # t = 0: p = 0
    assert abs(g.max() - 0.05) <= 1e-12                      # rolled with the slab: only the thickness
    level = bnp.terms(np.zeros((1, 1, 3, D)), T, hp, plate, 1, **par)[0].numpy()[0, 0, 0]
    assert abs(level.max() - (0.25 * math.sin(th) + 0.05 * math.cos(th))) <= 1e-12


def test_restatement_penalty_and_margin_conventions():
    rng = np.random.default_rng(2)
    co = rng.normal(size=(2, 3, 3, 6)) * 0.1
    T = rng.uniform(1.0, 2.0, (2, 3))
    verts = rng.normal(size=(4, 3)) * 0.3
    hp = rng.normal(size=(2, 3, 5, 4))
    hp[:, :, 3:] = 0.0                                       # two padding rows
    j = bnp.j_body(co, T, hp, verts, 6, 2.0, 0.1).numpy()
    j3 = bnp.j_body(co, T, hp[:, :, :3], verts, 6, 2.0, 0.1).numpy()
    assert np.allclose(j, j3, rtol=1e-14, atol=0.0) and (j > 0.0).any()         # padding rows add nothing
    far = hp.copy()
    far[:, :, :3, 3] += 1e6
    pc, gC, gT = bnp.j_body_grads(co, T, far, verts, 6, 2.0, 0.1)
    assert not pc.any() and not gC.any() and not gT.any()
    m, g, t = bnp.margin(co, T, hp, verts, 6)
    assert g.shape == (2, 3, 7, 5, 4) and np.array_equal(t[..., -1], T) and np.isfinite(m).all()
    hp[0, 1] = 0.0
    assert bnp.margin(co, T, hp, verts, 6)[0][0, 1] == -np.inf
    # the gradient w.r.t. a duration by central differences of the restatement itself
    pc, gC, gT = bnp.j_body_grads(co, T, hp, verts, 6, 2.0, 0.1)
    h = 1e-6
    Tp, Tm = T.copy(), T.copy()
    Tp[1, 2] += h
    Tm[1, 2] -= h
    fd = (bnp.j_body(co, Tp, hp, verts, 6, 2.0, 0.1).sum() - bnp.j_body(co, Tm, hp, verts, 6, 2.0, 0.1).sum()).item() / (2 * h)
    assert abs(fd - gT[1, 2]) <= 1e-6 * max(1.0, abs(gT[1, 2]))


def test_homogeneous_rotation_and_its_derivatives():
    """R b = (w^2 - v.v) b + 2 (v.b) v + 2 w (v x b) is quat_to_rot on the unit sphere, and the derivatives of g = a . R(q) b stated
    in include/allocnet_amd.h are those of this form."""
    rng = np.random.default_rng(3)
    q = torch.tensor(rng.normal(size=4), dtype=torch.float64)
    a, b = (torch.tensor(rng.normal(size=3), dtype=torch.float64) for _ in range(2))

    def g_of(q):
        w, v = q[0], q[1:]
        return a @ ((w * w - v @ v) * b + 2.0 * (v @ b) * v + 2.0 * w * torch.linalg.cross(v, b))
    qn = q / q.norm()
    assert abs(g_of(qn).item() - (a @ (fnp.quat_to_rot(qn) @ b)).item()) <= 1e-14
    qr = q.clone().requires_grad_(True)
    grad, = torch.autograd.grad(g_of(qr), qr)
    w, v = q[0], q[1:]
    dw = 2.0 * w * (a @ b) + 2.0 * a @ torch.linalg.cross(v, b)
    dv = -2.0 * (a @ b) * v + 2.0 * (v @ b) * a + 2.0 * (a @ v) * b + 2.0 * w * torch.linalg.cross(b, a)
    assert abs(grad[0] - dw).item() <= 1e-13 and (grad[1:] - dv).abs().max().item() <= 1e-13


def test_abi_structure():
    import allocnet_amd as aa
    from allocnet_amd import _lib, build
    for name, nargs in (("anet_minco_body_partial_grads_dev", 15), ("anet_traj_body_margin_dev", 15), ("anet_traj_body_margin", 13)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
    assert "api_body.hip" in build.SOURCES
    assert "api_body.hip" in open(os.path.join(build.SRC_DIR, "api_internal.h")).read()
    hdr = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    assert "#define ANET_MAX_BODY_VERTS 16" in hdr and "#define ANET_ABI_VERSION 2 " in hdr
    assert _lib.ANET_MAX_BODY_VERTS == 16
    # struct anet_body_penalty: two doubles, four int32, 16 x 3 doubles
    assert ctypes.sizeof(_lib.BodyPenalty) == 16 + 16 + 16 * 3 * 8
    assert _lib.BodyPenalty.verts.offset == 32 and _lib.BodyPenalty.n_verts.offset == 24
    for n in ("make_body_penalty", "box_body", "minco_body_partial_grads_dev", "minco_body_cost_grad", "minco_body_cost_grad_dev",
              "body_objective_dev", "traj_body_margin", "traj_body_margin_dev"):
        assert callable(getattr(aa, n)), n
    assert callable(aa.Trajectory.getBodyMargin) and callable(aa.Trajectory.checkBodyCorridor)


def test_host_helpers():
    import allocnet_amd as aa
    box = aa.box_body((0.25, 0.2, 0.05))
    assert box.shape == (8, 3) and len({tuple(v) for v in box}) == 8
    assert np.array_equal(np.abs(box), np.broadcast_to([0.25, 0.2, 0.05], (8, 3)))
    pen = aa.make_body_penalty(box, w=3.0, smooth_mu=0.02, res=11, poly_rows=9)
    assert (pen.w_body, pen.smooth_mu, pen.res, pen.poly_rows, pen.n_verts) == (3.0, 0.02, 11, 9, 8)
    assert np.array_equal(np.array([[pen.verts[k][c] for c in range(3)] for k in range(8)]), box)
    assert all(pen.verts[k][c] == 0.0 for k in range(8, 16) for c in range(3))
    for bad in (np.zeros((0, 3)), np.zeros((17, 3)), np.zeros((4, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            aa.make_body_penalty(bad)


def test_cpp_facade_sees_the_body_margin():
    """tests/cpp/test_body_corridor.cpp builds at the reference's language level without HIP or Eigen on the include path."""
    import subprocess
    src = os.path.join(ROOT, "tests", "cpp", "test_body_corridor.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
