"""Thread-sanitizer run of the C-ABI's host layer (helper threads, host-paced stream ordering, present / regrow /
failure protocols) on a fake HIP runtime: tests/host/tsan_host_test.cpp.  CPU only: no GPU, no pixels — order and
error protocol are checked, and ThreadSanitizer must stay silent.  A second build under the address
sanitizer checks the sizes of what the host layer allocates against what the stand-in kernels touch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, sanitize, runtime):
    """The host test built with -fsanitize=<sanitize>; skips where the compiler or the sanitizer's runtime is missing."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "tsan_host_test"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitize, "-I" + os.path.join(ROOT, "tests", "host", "hip_stub"),
           "-x", "c++", os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_api.hip"),
           os.path.join(ROOT, "tests", "host", "hip_stub", "stub_runtime.cpp"),
           os.path.join(ROOT, "tests", "host", "hip_stub", "stub_launch.cpp"),
           os.path.join(ROOT, "tests", "host", "tsan_host_test.cpp"), "-lpthread", "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and any(r in build.stderr.lower() for r in runtime) and "cannot find" in build.stderr.lower():
        pytest.skip("lib%s is not installed" % runtime[0])
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def test_host_layer_is_race_free_under_thread_sanitizer(tmp_path):
    exe = _build(tmp_path, "thread", ("tsan",))
    # gcc's TSan runtime cannot map a process laid out with the high mmap ASLR entropy of recent kernels (it stops before
    # main: "unexpected memory mapping", or a segfault); address randomisation off for this one process avoids that
    setarch = shutil.which("setarch")
    norand = [setarch, os.uname().machine, "-R"] if setarch else []
    run = subprocess.run(norand + [str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66"))
    out = run.stdout + run.stderr
    assert "WARNING: ThreadSanitizer" not in out, out[-4000:]
    assert run.returncode == 0 and "tsan host test: ok" in out, out[-2000:]


def test_host_layer_sizes_its_buffers_under_address_sanitizer(tmp_path):
    """The same program under ASan + UBSan: the stand-in kernels touch both ends of every table of their frame, so a lane buffer
    or the bins sized, checked or grown at the wrong size is a heap-buffer-overflow here (on the GPU it would land in the
    allocator's slack and nothing would report it)."""
    exe = _build(tmp_path, "address,undefined", ("asan", "ubsan"))
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout + run.stderr
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert run.returncode == 0 and "tsan host test: ok" in out, out[-2000:]
