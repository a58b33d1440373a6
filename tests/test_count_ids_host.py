"""The host layer of the visibility counts on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under
the address and undefined-behaviour sanitizers: tests/host/count_host_test.cpp.  CPU only; nothing is loaded into Python.  The count
launch is the stand-in of tests/host/hip_stub (a CPU loop over the header's definition), so what is checked is the host side: the rectangle clipped
to every band's rows for 1 and 3 bands and for one band of a larger target, the sum across bands and `none`, the counter buffer growing
and being zeroed between queries of different n, n == 0, and every error the header names."""
import host_build

ASAN = "address,undefined"


def test_count_host_layer_under_address_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "count_host_test.cpp", ASAN), "count host test: ok", ASAN)
