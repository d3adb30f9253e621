"""The shared pieces of the exact trajectory queries (csrc/bernstein_walk.h) on the host.

tests/cpp/test_bernstein_walk.cpp, a stand-alone program over the header alone, built with hipcc for the host only and run as an
ordinary executable (it makes no HIP runtime call): halving, descent, sign scan, order of visit and the depth bound of the walk,
for both index widths, in exact arithmetic."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bernstein_walk_on_the_host(tmp_path):
    from allocnet_amd import build as b
    exe = str(tmp_path / "test_bernstein_walk")
    res = subprocess.run([b.HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                          os.path.join(ROOT, "tests", "cpp", "test_bernstein_walk.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-2000:]
    assert "bernstein walk: 0 failures" in res.stdout
