"""The host layer of the delta reads on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under the
address and undefined-behaviour sanitizers: tests/host/delta_host_test.cpp.  CPU only; nothing is loaded into Python.  The program
supplies the two delta launches itself (CPU loops over the header's definition), so what is checked is the host side: the rectangle and
the counts derived from the flag tables for 1 and 3 bands and for one band of a larger target, the sums across bands, words planted
outside the rectangle found again, pageable and page-locked destinations, baselines kept (the same target again, the other reads, a
reset of the other kind) and dropped (a reset, another target), the staging growing and a rectangle larger than a stage chunk, and
every error the header names.  Built a second time without the launches, the program must still link (as the older stand-alone
programs do) and a delta read must fail loudly.  A third build takes the other way the changed part can reach a page-locked
destination (SWR_TUNE_DELTA_DIRECT=0: gathered and staged, as for a pageable one), so that the alternative the
measurements compare stays correct."""
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
           os.path.join(ROOT, "tests", "host", "delta_host_test.cpp"), "-lpthread", "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and any(r in build.stderr.lower() for r in ("asan", "ubsan")) and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout + run.stderr
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert run.returncode == 0 and "delta host test: ok" in out, out[-2000:]


def test_delta_host_layer_under_address_sanitizer(tmp_path):
    build_and_run(tmp_path, "delta_host_test", [])


def test_a_program_without_the_delta_launch_links_and_the_read_fails_loudly(tmp_path):
    build_and_run(tmp_path, "delta_host_test_no_launch", ["-DDELTA_HOST_NO_LAUNCH"])


def test_delta_host_layer_with_the_other_way_to_a_page_locked_destination(tmp_path):
    build_and_run(tmp_path, "delta_host_test_staged", ["-DSWR_TUNE_DELTA_DIRECT=0"])
