"""Thread-sanitizer run of the C-ABI's host layer (helper threads, host-paced stream ordering, present / regrow /
failure protocols) on a fake HIP runtime: tests/host/tsan_host_test.cpp.  CPU only: no GPU, no pixels — order and
error protocol are checked, and ThreadSanitizer must stay silent.  A second build under the address
sanitizer checks the sizes of what the host layer allocates against what the stand-in kernels touch."""
import host_build


def test_host_layer_is_race_free_under_thread_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "tsan_host_test.cpp", "thread"), "tsan host test: ok", "thread")


def test_host_layer_sizes_its_buffers_under_address_sanitizer(tmp_path):
    """The same program under ASan + UBSan: the stand-in kernels touch both ends of every table of their frame, so a lane buffer
    or the bins sized, checked or grown at the wrong size is a heap-buffer-overflow here (on the GPU it would land in the
    allocator's slack and nothing would report it)."""
    exe = host_build.build_program(tmp_path, "tsan_host_test.cpp", "address,undefined")
    host_build.run_clean(exe, "tsan host test: ok", "address,undefined")
