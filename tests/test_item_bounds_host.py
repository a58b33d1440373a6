"""The host layer of the item bounds on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under the
address and undefined-behaviour sanitizers: tests/host/item_bounds_host_test.cpp.  CPU only; nothing is loaded into Python.  The
stand-in of launch_item_bounds is the stand-in launch set's (a CPU loop over the stream slots of the items it is handed), so what is
checked is the host side: the items resolved to stream ranges and work units, the stream cut once for a
repeated list and found in place by the list drawn afterwards, band 0 alone launching on a 3-band context, one band of a larger
target answering for the full target, the staging growing and starting from zero across calls of 1, 4096 and 2 items, n == 0, every
error the header names with nothing written, and the sticky error."""
import host_build

ASAN = "address,undefined"


def test_item_bounds_host_layer_under_address_sanitizer(tmp_path):
    exe = host_build.build_program(tmp_path, "item_bounds_host_test.cpp", ASAN)
    host_build.run_clean(exe, "item bounds host test: ok", ASAN)
