"""The host layer of the depth queries on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under the
address and undefined-behaviour sanitizers: tests/host/depth_query_host_test.cpp.  CPU only; nothing is loaded into Python.  The
depth-query launch is the stand-in of tests/host/hip_stub (a CPU loop over the header's definition), so what is checked is the host side: the
boxes clipped to every band's rows for 1 and 3 bands and for one band of a larger target, the sum across bands, the list of large
boxes and the total area handed to the launch, the staging growing and being re-zeroed between queries of different n, n == 0, and
every error the header names."""
import host_build

ASAN = "address,undefined"


def test_depth_query_host_layer_under_address_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "depth_query_host_test.cpp", ASAN), "depth query host test: ok", ASAN)
