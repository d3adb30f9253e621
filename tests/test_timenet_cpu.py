"""The time-allocation network without a GPU: the numpy restatement (tests/timenet_np.py) against the recorded outputs of the
reference's model; the weights file round trip; the new entry points declared, exported and bound; the kernels compiled for
gfx950 with no scratch memory; the C++ facade as C++14; and, without a device, a loud failure instead of a host result."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import timenet_np as tnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_NAMES = ["anet_timenet_create", "anet_timenet_destroy", "anet_timenet_device_bytes", "anet_timenet_forward",
             "anet_timenet_forward_dev"]


def _fixtures():
    return tnp.load_golden_weights(os.path.join(GOLDEN, "timenet_seq5")), np.load(os.path.join(GOLDEN, "timenet_seq5_cases.npz"))


def test_restatement_matches_the_reference_fixtures():
    """All 256 cases: the same count; the float64 restatement within 1e-6 of tf, stop and times (about 4 float32 ulps at the
    largest time, 2.1); the float32 one within 2e-6 (twice that: its own rounding on top)."""
    w, d = _fixtures()
    assert d["state"].shape == (256, 9, 2) and d["hpolys"].shape == (256, 50, 4, 5)
    for dtype, tol in ((np.float64, 1e-6), (np.float32, 2e-6)):
        times, count, tf, stop = tnp.forward(w, d["state"], d["hpolys"], 0.5, dtype)
        errs = [float(np.abs(a - d[k]).max()) for a, k in ((tf, "tf"), (stop, "stop"), (times, "times"))]
        print(dtype.__name__, errs)
        assert (count == d["count"]).all()
        assert max(errs) <= tol, errs


def test_fixtures_are_what_the_docs_say():
    """The recorded per-step outputs reproduce the whole model's times; no case sits within 1e-4 of the thresholds 0.5 and
    0.42, so the GPU tests leave none out there; the yardstick (torch against itself) is in the file."""
    _, d = _fixtures()
    count, times = tnp.count_times(d["tf"], d["stop"], 0.5)
    assert (count == d["count"]).all()
    dis = float(np.abs(times - d["times"]).max())
    assert dis == float(d["self_disagreement"]) and dis <= 1e-6
    assert sorted(set(d["count"].tolist())) == [2, 3, 4]
    for thr in (0.5, 0.42):
        assert tnp.stop_margin(d["stop"], thr).min() > 1e-4
    assert (tnp.count_times(d["tf"], d["stop"], 0.0)[0] == 1).all()
    c999 = tnp.count_times(d["tf"], d["stop"], 0.999)[0]
    assert c999.max() == 5 and (d["stop"].max(axis=1) <= 0.999).any()            # 0.999 covers "no stop -> count = L"


def test_restatement_seq10_shapes_and_pools():
    """L = 10 (unpinned: no reference output exists): 32 flattened features, channel-major, from columns 0..7 only."""
    w = tnp.random_weights(10, 1)
    rng = np.random.default_rng(2)
    s = rng.normal(size=(3, 9, 2)); hp = rng.normal(size=(3, 50, 4, 10))
    x = tnp.encode(w, s, hp)
    assert x.shape == (3, 38)
    hp2 = hp.copy(); hp2[:, :, :, 9] += 5.0                                       # column 9 reaches conv column 8, which the pools drop
    assert np.abs(tnp.encode(w, s, hp2) - x).max() == 0.0
    hp3 = hp.copy(); hp3[:, :, :, 8] += 5.0                                       # column 8 reaches conv column 7
    assert np.abs(tnp.encode(w, s, hp3) - x).max() > 0.0
    times, count, tf, stop = tnp.forward(w, s, hp, 0.5)
    assert times.shape == (3, 10) and ((times != 0).sum(axis=1) == count).all()


def test_weights_file_round_trip_and_malformed(tmp_path):
    import allocnet_amd as aa
    w, _ = _fixtures()
    net = aa.TimeAllocNet.from_state_dict(w)
    assert net.seq_len == 5 and net.hidden == 256
    p = str(tmp_path / "seq5.anetw")
    net.save(p)
    back = aa.TimeAllocNet.load(p)
    for k in aa.time_net.TENSOR_KEYS:
        assert back.weights[k].dtype == np.float32 and back.weights[k].shape == w[k].shape
        assert (back.weights[k].view(np.uint32) == np.ascontiguousarray(w[k]).view(np.uint32)).all(), k
    assert list(aa.time_net.TENSOR_KEYS) == tnp.KEYS
    raw = open(p, "rb").read()
    assert len(raw) == 20 + 4 * 311656
    for bad in (raw[:-4], raw + b"\0\0\0\0", b"NOTANETW" + raw[8:], raw[:8] + b"\x02\0\0\0" + raw[12:],
                raw[:12] + b"\x07\0\0\0" + raw[16:], raw[:10]):
        q = str(tmp_path / "bad.anetw")
        open(q, "wb").write(bad)
        with pytest.raises(ValueError):
            aa.TimeAllocNet.load(q)
    sd = dict(w); del sd["tfs_output_layer.bias"]
    with pytest.raises(ValueError):
        aa.TimeAllocNet.from_state_dict(sd)
    sd = dict(w); sd["output_module.weight_ih_l0"] = w["output_module.weight_ih_l0"][:, :37]
    with pytest.raises(ValueError):
        aa.TimeAllocNet.from_state_dict(sd)
    planner = aa.LearningPlanner(aa.LearningPlannerConfig(ModelMaxSeg=5))
    assert planner.loadModel(str(tmp_path / "missing.anetw")) is False
    assert planner.loadModel(q) is False
    assert planner.loadModel(p) is True
    assert aa.LearningPlanner(aa.LearningPlannerConfig(ModelMaxSeg=10)).loadModel(p) is False


def _declared():
    txt = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(anet_[A-Za-z0-9_]+)\s*\(", txt))


def test_timenet_entry_points_are_declared_exported_and_bound():
    from allocnet_amd import _lib, time_net
    declared = _declared()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared in the header"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.PROTOTYPES, f"{n} is not in the ctypes table"
    assert {n for n in declared if n.startswith("anet_timenet")} == set(NEW_NAMES)
    assert _lib.load().anet_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    for name, val in (("KEEP_PADDING", time_net.KEEP_PADDING), ("FORM_SINGLE", time_net.FORM_SINGLE),
                      ("FORM_TILE", time_net.FORM_TILE), ("SINGLE_MAX", time_net.SINGLE_MAX), ("TENSORS", len(time_net.TENSOR_KEYS))):
        assert int(re.search(rf"#define ANET_TIMENET_{name} (\d+)", hdr).group(1)) == val, name


def test_no_cpu_result_without_a_device():
    import allocnet_amd as aa
    from allocnet_amd import _lib
    w, d = _fixtures()
    net = aa.TimeAllocNet.from_state_dict(w)
    if _lib.load().anet_device_count() != 0:
        times, count = net.forward(d["state"][:2], d["hpolys"][:2])                # (a GPU box: the product path answers)
        assert (count == d["count"][:2]).all()
        return
    with pytest.raises(aa.AnetError) as ei:
        net.forward(d["state"][:2], d["hpolys"][:2])
    assert ei.value.code == _lib.ANET_ERR_NODEVICE


def test_facades_do_not_name_the_test_side():
    for rel in ("include/allocnet_amd/time_net.hpp", "include/allocnet_amd/learning_planner.hpp", "allocnet_amd/time_net.py",
                "allocnet_amd/learning_planner.py", "allocnet_amd/csrc/timenet_kernels.h", "allocnet_amd/csrc/api_timenet.hip"):
        assert "oracle" not in open(os.path.join(ROOT, rel)).read(), rel


def test_cpp_learning_planner_facade_compiles_as_cxx14():
    src = os.path.join(ROOT, "tests", "cpp", "test_learning_planner.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                          src], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_timenet_kernels_use_no_scratch():
    """The new unit compiled for gfx950 with the product's flags: no kernel of it may use scratch memory; the recurrent tile
    kernel holds its accumulators, the input's share of the gates and c in registers (DESIGN.md 8g has the table)."""
    from allocnet_amd import build as b
    cflags = [f for f in b.FLAGS if f not in ("-shared", "-ldl")] + b.probe_flags(b.MFMA_VGPR_FORM)
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([b.HIPCC] + cflags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                   os.path.join(b.SRC_DIR, "api_timenet.hip"), "-o", os.path.join(td, "u.o")],
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
    seen = set()
    for fn, u in usage.items():
        for k in ("k_timenet_encode", "k_timenet_single", "k_timenet_tile"):
            if k in fn:
                seen.add((k, "Li10E" in fn))
                print(fn, u)
                assert u["ScratchSize"] == 0, (fn, u)
                assert u["VGPRs"] + u["AGPRs"] <= 512, (fn, u)
    assert len(seen) == 6, seen
    assert "api_timenet.hip" in b.SOURCES
