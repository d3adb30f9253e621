"""The staging statements of the host entry points (csrc/staging.h) measure what they carve, and never more than the sums they replaced.

tests/cpp/test_staging_layout.cpp, a stand-alone program over staging.h alone with a memcpy transport, built with the host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary executable: it replays the field sequence of every
trajectory-major host entry point in a buffer of exactly the measured size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staging_statements_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_staging_layout")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                          os.path.join(ROOT, "tests", "cpp", "test_staging_layout.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=540)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert " 0 failures" in res.stdout

