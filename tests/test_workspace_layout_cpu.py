"""The workspaces keep their sizes, and their layouts (csrc/workspace.h) carve without overlap.

Sizes: every anet_*_workspace function over the shape list of tools/record_workspace_sizes.py against
tests/golden/workspace_sizes.json, recorded before the layouts moved to workspace.h.  The query runs in a child process with the
ANET_* switches removed: tuning() reads them once per process and two of them enter anet_lbfgs_minco_workspace.

Carves: tests/cpp/test_workspace_layout.cpp, a stand-alone program over workspace.h alone, built with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary executable on the same list."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
LAYOUT_OF = {"anet_minco_cost_grad_workspace": "cost_grad", "anet_qp_solve_workspace": "qp", "anet_lbfgs_workspace": "lbfgs",
             "anet_lbfgs_minco_workspace": "lbfgs_minco", "anet_firi_workspace": "firi"}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_fixture_covers_the_shape_list(recorded):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from record_workspace_sizes import cases
    finally:
        sys.path.pop(0)
    want = cases()
    assert sorted(recorded) == sorted(want)
    for fn, rows in want.items():
        flat = [[x for e in a for x in (e if isinstance(e, tuple) else (e,))] for a in rows]
        assert [r[:-1] for r in recorded[fn]] == flat, fn


def test_workspace_sizes_are_the_recorded_ones(recorded):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ANET_")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_workspace_sizes.py")], capture_output=True, text=True,
                         env=env, timeout=300)
    assert res.returncode == 0, res.stderr
    now = json.loads(res.stdout)
    assert sorted(now) == sorted(recorded)
    for fn in recorded:
        diff = [(a, b) for a, b in zip(recorded[fn], now[fn]) if a != b]
        assert not diff and len(now[fn]) == len(recorded[fn]), (fn, diff[:5])


def test_layouts_carve_without_overlap_under_sanitizers(recorded, tmp_path):
    from allocnet_amd import _lib
    lib = _lib.load()
    exe = str(tmp_path / "test_workspace_layout")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                          os.path.join(ROOT, "tests", "cpp", "test_workspace_layout.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = []
    for fn, layout in LAYOUT_OF.items():
        for row in recorded[fn]:
            if layout == "firi":  # the row stride of its MVIE rows is the library's choice for the batch
                row = row[:-1] + [lib.anet_recommended_ld(row[0]), row[-1]]
            lines.append(layout + " " + " ".join(str(x) for x in row))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=540)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert " 0 failures" in res.stdout
