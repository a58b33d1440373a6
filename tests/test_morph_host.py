"""The host layer of the morph targets on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under
the address and undefined-behaviour sanitizers: tests/host/morph_host_test.cpp.  CPU only; nothing is loaded into Python and nothing
is preloaded.  The morph launch and the two skin launches are the stand-ins of tests/host/hip_stub (CPU loops over the header's arithmetic that
read and write every element they are given), so what is checked is the host side: the stream every band holds after each call
against the model, for 1 and 3 bands and for 1, 129 and 200 triangles — weights behind an un-waited frame and behind an overflowed
one, a morph under a pose and a pose under a morph, re-application after the stream was cut for a draw list and after attributes
arrived (normal deltas given earlier take effect), zero and NULL weights restoring the uploaded or posed stream, new targets zeroing
the weights and keeping the pose, removal, an upload dropping everything, deltas from pageable and from page-locked memory, 256
targets with all and with only the last active, every error the header names (SWR_ERR_NOMEM excepted: the fake runtime never refuses
an allocation) with stream, targets and weights untouched, and the sticky error."""
import host_build

ASAN = "address,undefined"


def test_morph_host_layer_under_address_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "morph_host_test.cpp", ASAN), "morph host test: ok", ASAN)
