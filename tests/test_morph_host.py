"""The host layer of the morph targets on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under
the address and undefined-behaviour sanitizers: tests/host/morph_host_test.cpp.  CPU only; nothing is loaded into Python and nothing
is preloaded.  The program supplies the morph launch and the two skin launches itself (CPU loops over the header's arithmetic that
read and write every element they are given), so what is checked is the host side: the stream every band holds after each call
against the model, for 1 and 3 bands and for 1, 129 and 200 triangles — weights behind an un-waited frame and behind an overflowed
one, a morph under a pose and a pose under a morph, re-application after the stream was cut for a draw list and after attributes
arrived (normal deltas given earlier take effect), zero and NULL weights restoring the uploaded or posed stream, new targets zeroing
the weights and keeping the pose, removal, an upload dropping everything, deltas from pageable and from page-locked memory, 256
targets with all and with only the last active, every error the header names (SWR_ERR_NOMEM excepted: the fake runtime never refuses
an allocation) with stream, targets and weights untouched, and the sticky error.  Built a second time without the morph launch, the
program must still link (as the older stand-alone programs do) and swr_morph_set must fail loudly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    stub = os.path.join(ROOT, "tests", "host", "hip_stub")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + stub, *extra,
           "-x", "c++", os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_api.hip"),
           os.path.join(stub, "stub_runtime.cpp"), os.path.join(stub, "stub_launch.cpp"),
           os.path.join(ROOT, "tests", "host", "morph_host_test.cpp"), "-lpthread", "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and any(r in build.stderr.lower() for r in ("asan", "ubsan")) and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout + run.stderr
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert run.returncode == 0 and "morph host test: ok" in out, out[-2000:]


def test_morph_host_layer_under_address_sanitizer(tmp_path):
    build_and_run(tmp_path, "morph_host_test", [])


def test_a_program_without_the_morph_launch_links_and_the_weights_fail_loudly(tmp_path):
    build_and_run(tmp_path, "morph_host_test_no_launch", ["-DMORPH_HOST_NO_LAUNCH"])
