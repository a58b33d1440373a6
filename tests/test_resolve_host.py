"""The host layer of the supersampled resolve on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program
under the address and undefined-behaviour sanitizers: tests/host/resolve_host_test.cpp.  CPU only.  The program supplies the resolve
launch itself (a CPU loop over the header's formulas), so what is checked is the host side: the sizes of the resolved buffers, band
offsets, the row pitch and destination rows of the generalised copy_band, the page-locked path and the staged path across an 8 MiB
chunk, the group fan-out and swr_render_resolved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resolve_host_layer_under_address_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "resolve_host_test"
    stub = os.path.join(ROOT, "tests", "host", "hip_stub")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + stub,
           "-x", "c++", os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_api.hip"),
           os.path.join(stub, "stub_runtime.cpp"), os.path.join(stub, "stub_launch.cpp"),
           os.path.join(ROOT, "tests", "host", "resolve_host_test.cpp"), "-lpthread", "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and any(r in build.stderr.lower() for r in ("asan", "ubsan")) and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout + run.stderr
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert run.returncode == 0 and "resolve host test: ok" in out, out[-2000:]
