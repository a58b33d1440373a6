"""The host layer of the skinned meshes on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under
the address and undefined-behaviour sanitizers: tests/host/skin_host_test.cpp.  CPU only; nothing is loaded into Python.  The two
skin launches are the stand-ins of tests/host/hip_stub (CPU loops over the header's arithmetic that read and write every element they are given), so
what is checked is the host side: the arrays and sizes it hands over for 1 and 3 bands, a pose behind an un-waited frame and behind
an overflowed one, the pose applied again after the stream was cut for a draw list and after attributes arrived, the bind pose
restored by a NULL pose, a new skin and a removed one, an upload dropping skin and pose, and every error the header names, each
leaving the stream alone."""
import host_build

ASAN = "address,undefined"


def test_skin_host_layer_under_address_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "skin_host_test.cpp", ASAN), "skin host test: ok", ASAN)
