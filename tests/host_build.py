"""Builds and runs the stand-alone host test programs of tests/host on the fake HIP runtime (tests/host/hip_stub).  The host layer
(software-renderer_amd/csrc/swr_api.hip as plain C++), the fake runtime and the stand-in launch set are compiled once per sanitizer and
set of defines and kept for the session; each program compiles its own source and links with those objects.  CPU only: the programs
have their own main, nothing is loaded into Python and nothing is preloaded."""
import atexit
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "host", "hip_stub")
SHARED = (os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_api.hip"),
          os.path.join(STUB, "stub_runtime.cpp"), os.path.join(STUB, "stub_launch.cpp"))

_objects = {}       # (sanitize, defines) -> the object files of SHARED


def _gxx(args, sanitize, defines):
    """One g++ call with the flags every host test is built with; skips where the compiler or the sanitizer's runtime is missing."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitize, "-I" + STUB, *defines, *args]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    runtime = ("tsan",) if sanitize == "thread" else ("asan", "ubsan")
    if build.returncode != 0 and any(r in build.stderr.lower() for r in runtime) and "cannot find" in build.stderr.lower():
        pytest.skip("lib%s is not installed" % runtime[0])
    assert build.returncode == 0, build.stderr[-2000:]


def objects(sanitize, defines=()):
    """The host layer, the fake runtime and the stand-in launches as object files, compiled once per (sanitize, defines)."""
    key = (sanitize, tuple(defines))
    if key not in _objects:
        out = tempfile.mkdtemp(prefix="swr_host_")
        atexit.register(shutil.rmtree, out, ignore_errors=True)
        objs = []
        for src in SHARED:
            objs.append(os.path.join(out, os.path.splitext(os.path.basename(src))[0] + ".o"))
            _gxx(["-x", "c++", "-c", src, "-o", objs[-1]], sanitize, key[1])
        _objects[key] = objs
    return _objects[key]


def build_program(tmp_path, source, sanitize, defines=()):
    """tests/host/<source> compiled and linked with objects(sanitize, defines); the path of the program."""
    exe = tmp_path / os.path.splitext(source)[0]
    _gxx([os.path.join(ROOT, "tests", "host", source), *objects(sanitize, defines), "-lpthread", "-o", str(exe)], sanitize, defines)
    return exe


def run_clean(exe, ok_line, sanitize):
    """Runs the program: the sanitizer must stay silent, the exit code be 0 and the program's own verdict `ok_line`."""
    if sanitize == "thread":
        # gcc's TSan runtime cannot map a process laid out with the high mmap ASLR entropy of recent kernels (it stops before
        # main: "unexpected memory mapping", or a segfault); address randomisation off for this one process avoids that
        setarch = shutil.which("setarch")
        prefix = [setarch, os.uname().machine, "-R"] if setarch else []
        env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66")
        reports = ("WARNING: ThreadSanitizer",)
    else:
        prefix = []
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1")
        reports = ("AddressSanitizer", "LeakSanitizer", "runtime error:")
    run = subprocess.run(prefix + [str(exe)], capture_output=True, text=True, timeout=600, env=env)
    out = run.stdout + run.stderr
    assert not any(r in out for r in reports), out[-4000:]
    assert run.returncode == 0 and ok_line in out, out[-2000:]
