"""The host layer of the delta reads on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under the
address and undefined-behaviour sanitizers: tests/host/delta_host_test.cpp.  CPU only; nothing is loaded into Python.  The two
delta launches are the stand-ins of tests/host/hip_stub (CPU loops over the header's definition), so what is checked is the host side: the rectangle and
the counts derived from the flag tables for 1 and 3 bands and for one band of a larger target, the sums across bands, words planted
outside the rectangle found again, pageable and page-locked destinations, baselines kept (the same target again, the other reads, a
reset of the other kind) and dropped (a reset, another target), the staging growing and a rectangle larger than a stage chunk, and
every error the header names.  A second build takes the other way the changed part can reach a page-locked
destination (SWR_TUNE_DELTA_DIRECT=0: gathered and staged, as for a pageable one), so that the alternative the
measurements compare stays correct."""
import host_build

ASAN = "address,undefined"


def test_delta_host_layer_under_address_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "delta_host_test.cpp", ASAN), "delta host test: ok", ASAN)


def test_delta_host_layer_with_the_other_way_to_a_page_locked_destination(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "delta_host_test.cpp", ASAN, ("-DSWR_TUNE_DELTA_DIRECT=0",)), "delta host test: ok", ASAN)
