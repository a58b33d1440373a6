"""The frame policy of the host layer (software-renderer_amd/csrc/swr_frame_policy.h: where a frame's bins are sorted, whether it
defers large triangles, whether it keeps the 32-bit depth keys) at the edges of its thresholds, as a stand-alone program under the
address and undefined-behaviour sanitizers: tests/host/frame_policy_test.cpp.  CPU only; the program includes nothing but the header,
needs no HIP and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_policy_thresholds_under_address_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "frame_policy_test"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           os.path.join(ROOT, "tests", "host", "frame_policy_test.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and any(r in build.stderr.lower() for r in ("asan", "ubsan")) and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout + run.stderr
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert run.returncode == 0 and "frame policy test: ok" in out, out[-2000:]
