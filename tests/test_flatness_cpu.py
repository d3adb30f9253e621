"""Differential flatness without a GPU: the restatement the GPU tests compare against (tests/flatness_np.py) is checked
against facts that do not depend on it; the new entry points are declared, exported and bound; the C++ facade compiles as
C++14; the pointwise and trajectory kernels keep their state in registers; and without a device the map fails loudly."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import flatness_np as fnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["anet_flat_forward", "anet_flat_forward_dev", "anet_flat_backward", "anet_flat_backward_dev",
             "anet_traj_flat_states", "anet_traj_flat_states_dev", "anet_traj_flat_extrema", "anet_traj_flat_extrema_dev",
             "anet_minco_flat_partial_grads_dev"]


def _states(n=2000, seed=5):
    """Random states inside the planner's boxes: |v| <= 4, |a| <= 6 per axis (planner.yaml:17-19)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-4.0, 4.0, (n, 3)), rng.uniform(-6.0, 6.0, (n, 3)), rng.normal(size=(n, 3)) * 5.0,
            rng.uniform(-math.pi, math.pi, n), rng.normal(size=n))


def test_restatement_hover():
    z3 = np.zeros((1, 3))
    thr, quat, omg, z = fnp.forward(z3, z3, z3)
    assert abs(float(thr) - 9.8) <= 1e-15 * 9.8
    assert np.abs(quat.numpy() - [[1.0, 0.0, 0.0, 0.0]]).max() == 0.0
    assert np.abs(omg.numpy()).max() == 0.0
    thr2, *_ = fnp.forward(z3, z3, z3, mass=2.5, grav=9.81)
    assert abs(float(thr2) - 2.5 * 9.81) <= 1e-14


def test_restatement_attitude_identities():
    v, a, j, psi, dpsi = _states()
    thr, quat, omg, z = fnp.forward(v, a, j, psi, dpsi)
    assert float(z[:, 2].min()) > 0.0                                   # zu_3 >= 0.8 inside the boxes: no singular attitude
    assert float((quat.norm(dim=-1) - 1.0).abs().max()) <= 1e-14
    R = fnp.quat_to_rot(quat)
    assert float((R[:, :, 2] - z).abs().max()) <= 1e-14                 # the body z axis is the thrust direction
    tilt_q = fnp.tilt_of_quat(quat)
    assert float((tilt_q - torch.acos(z[:, 2])).abs().max()) <= 1e-13
    # the body x axis has the heading psi: its projection on the horizontal plane before the tilt
    thr0, quat0, _, _ = fnp.forward(v, a, j)
    yaw = torch.stack([torch.cos(torch.as_tensor(psi) / 2), torch.zeros(len(psi), dtype=torch.float64),
                       torch.zeros(len(psi), dtype=torch.float64), torch.sin(torch.as_tensor(psi) / 2)], -1)
    assert float((fnp.quat_mul(quat0, yaw) - quat).abs().max()) <= 1e-14
    assert float((thr0 - thr).abs().max()) == 0.0                       # thrust does not depend on the yaw
    # equal drag coefficients: the force to produce is along z, so thr is its norm
    thr_e, _, _, _ = fnp.forward(v, a, j, dh=0.8, dv=0.8)
    sp = np.sqrt((v * v).sum(-1, keepdims=True) + 1e-4)
    f = a + 0.8 * (1.0 + 0.01 * sp) * v + np.array([0.0, 0.0, 9.8])
    assert np.abs(thr_e.numpy() - np.linalg.norm(f, axis=-1)).max() <= 1e-13


def test_restatement_body_rate_is_the_quaternion_rate():
    """omg = 2 conj(q) (x) dq/dt with dq/dt by central differences (h = 1e-5) along quintic trajectories with a quadratic yaw."""
    rng = np.random.default_rng(11)
    n, h = 400, 1e-5
    co = rng.uniform(-1.0, 1.0, (n, 3, 6)) * np.array([0.1, 0.15, 0.25, 0.5, 1.0, 1.0])   # |v| <= 3.85, |a| <= 5.3 on [0, 0.9]
    yc = rng.normal(size=(n, 3))
    t0 = rng.uniform(0.1, 0.9, n)

    def at(t):
        _, v, a, j = fnp.piece_derivs(co, t)
        psi = yc[:, 0] + yc[:, 1] * t + yc[:, 2] * t * t
        dpsi = yc[:, 1] + 2.0 * yc[:, 2] * t
        assert float(v.abs().max()) <= 4.0 and float(a.abs().max()) <= 6.0
        return fnp.forward(v, a, j, psi, dpsi)
    _, q, omg, _ = at(t0)
    _, qp, _, _ = at(t0 + h)
    _, qm, _, _ = at(t0 - h)
    qd = (qp - qm) / (2.0 * h)
    conj = q * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float64)
    w = 2.0 * fnp.quat_mul(conj, qd)
    assert float(w[:, 0].abs().max()) <= 1e-7                                        # a unit quaternion's rate is pure
    err = (w[:, 1:] - omg).abs() / torch.clamp(omg.abs(), min=1.0)
    assert float(err.max()) <= 1e-7, float(err.max())


def test_restatement_backward_is_the_gradient():
    """autograd of the restatement against central differences of the restatement (1e-6 steps)."""
    v, a, j, psi, dpsi = _states(20, seed=3)
    rng = np.random.default_rng(4)
    gt, gq, go = rng.normal(size=20), rng.normal(size=(20, 4)), rng.normal(size=(20, 3))
    grads = fnp.backward(v, a, j, psi, dpsi, gt, gq, go)

    def loss(*ins):
        thr, quat, omg, _ = fnp.forward(*ins)
        return (thr.numpy() * gt + (quat.numpy() * gq).sum(-1) + (omg.numpy() * go).sum(-1))
    ins = [v, a, j, psi, dpsi]
    h = 1e-6
    for k, x in enumerate(ins):
        for ax in range(3 if x.ndim == 2 else 1):
            xp, xm = x.copy(), x.copy()
            if x.ndim == 2:
                xp[:, ax] += h; xm[:, ax] -= h
            else:
                xp += h; xm -= h
            fd = (loss(*(ins[:k] + [xp] + ins[k + 1:])) - loss(*(ins[:k] + [xm] + ins[k + 1:]))) / (2 * h)
            g = grads[k][:, ax] if x.ndim == 2 else grads[k]
            assert np.abs(fd - g).max() <= 1e-6 * max(1.0, np.abs(g).max())


def _declared():
    txt = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(anet_[A-Za-z0-9_]+)\s*\(", txt))


def test_flat_entry_points_are_declared_exported_and_bound():
    from allocnet_amd import _lib
    declared = _declared()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared in the header"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.PROTOTYPES, f"{n} is not in the ctypes table"
    flat = {n for n in declared if re.match(r"anet_flat_|anet_.*flat", n)}
    assert flat == set(NEW_NAMES), flat ^ set(NEW_NAMES)
    assert _lib.load().anet_abi_version() == 2


def test_flat_struct_sizes_match_ctypes():
    """sizeof and the field offsets of the two structs as a C compiler lays them out against the ctypes mirrors."""
    from allocnet_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "allocnet_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(anet_flat_params), offsetof(anet_flat_params, speed_eps), sizeof(anet_flat_penalty), '
           'offsetof(anet_flat_penalty, min_thrust), offsetof(anet_flat_penalty, max_bdr), offsetof(anet_flat_penalty, res)); '
           'return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "sz.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(td, "sz")],
                       check=True, capture_output=True)
        got = [int(x) for x in subprocess.run([os.path.join(td, "sz")], capture_output=True, text=True, check=True).stdout.split()]
    P, Q = _lib.FlatParams, _lib.FlatPenalty
    assert got == [ctypes.sizeof(P), P.speed_eps.offset, ctypes.sizeof(Q), Q.min_thrust.offset, Q.max_bdr.offset, Q.res.offset]


def test_no_cpu_result_without_a_device():
    import allocnet_amd as aa
    from allocnet_amd import _lib
    if _lib.load().anet_device_count() != 0:
        thr, quat, omg = aa.FlatnessMap().forward([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
        assert abs(thr - 9.8) <= 1e-12                                  # (a GPU box: the product path answers)
        return
    with pytest.raises(aa.AnetError) as ei:
        aa.FlatnessMap().forward([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    assert ei.value.code == _lib.ANET_ERR_NODEVICE
    z = np.zeros((1, 1, 3, 6))
    with pytest.raises(aa.AnetError):
        aa.traj_flat_extrema(aa.FlatnessMap(), z, np.ones((1, 1)))


def test_cpp_flatness_facade_compiles_as_cxx14():
    src = os.path.join(ROOT, "tests", "cpp", "test_flatness.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_flat_kernels_keep_their_state_in_registers():
    """The new unit compiled for gfx950 with the product's flags: the pointwise and the trajectory kernels hold well under 100 live
    doubles and must not use scratch memory; k_flat_piece_grad's figures are recorded in DESIGN.md 8f and printed here."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_flatness.hip"), "-o", os.path.join(td, "u.o")],
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
    seen = set()
    for fn, u in usage.items():
        for k in ("k_flat_forward", "k_flat_backward", "k_traj_flat_states", "k_traj_flat_extrema", "k_flat_piece_grad"):
            if k in fn:
                seen.add(k)
                print(fn, u)
                if k != "k_flat_piece_grad":
                    assert u["ScratchSize"] == 0, (fn, u)
    assert len(seen) == 5, seen
