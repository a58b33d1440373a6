"""The host layer of the dual-quaternion skinning on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone
program under the address and undefined-behaviour sanitizers: tests/host/skin_dq_host_test.cpp.  The stand-in launch set's
swr::launch_skin_vertices_dq (a CPU loop over the header's arithmetic that reads and writes every element it is handed) is the launch
the host layer calls.  CPU only; nothing is loaded into Python and nothing is preloaded.  What is checked is
the host side: the table and the arrays it hands over for 1 and 3 bands and 1, 129 and 200 triangles, the stream every band holds
after each call (NaN compared as NaN), the pose behind an un-waited frame and behind an overflowed one, the pose re-applied as a
dual-quaternion pose after a restream, after attributes, after swr_scene_morph and after swr_morph_set, matrix and dual-quaternion
poses in turn, each NULL pose after the other kind, 1024 joints, every error with the stream untouched, and the sticky error."""
import host_build

ASAN = "address,undefined"


def test_skin_dq_host_layer_under_address_sanitizer(tmp_path):
    host_build.run_clean(host_build.build_program(tmp_path, "skin_dq_host_test.cpp", ASAN), "skin dq host test: ok", ASAN)
