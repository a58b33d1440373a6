"""What a context owns goes with it (CPU): tests/host/owners_host_test.cpp on the fake HIP runtime of tests/host/hip_stub, as a stand-alone
program under the address, undefined-behaviour and leak sanitizers.  With 1 band and with 3 it touches everything a context allocates
lazily, then destroys the context: a buffer, pinned word, event, stream or worker nobody owns is a leak the sanitizer reports.  Nothing
is loaded into Python and nothing is preloaded."""
import host_build

ASAN = "address,undefined"


def test_owners_host_layer_under_address_and_leak_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "owners_host_test.cpp", ASAN), "owners host test: ok", ASAN)
