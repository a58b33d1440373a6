"""The host layer of the supersampled resolve on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program
under the address and undefined-behaviour sanitizers: tests/host/resolve_host_test.cpp.  CPU only.  The resolve launch is the
stand-in of tests/host/hip_stub (a CPU loop over the header's formulas), so what is checked is the host side: the sizes of the resolved buffers, band
offsets, the row pitch and destination rows of the generalised copy_band, the page-locked path and the staged path across an 8 MiB
chunk, the group fan-out and swr_render_resolved."""
import host_build

ASAN = "address,undefined"


def test_resolve_host_layer_under_address_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "resolve_host_test.cpp", ASAN), "resolve host test: ok", ASAN)
