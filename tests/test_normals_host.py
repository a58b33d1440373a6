"""The host layer of the computed normals on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under
the address and undefined-behaviour sanitizers: tests/host/normals_host_test.cpp.  The stand-ins of the three launches of
swr_normals.hip are the launch set's (CPU loops over the header's arithmetic that read and write every element they are handed, and
note when they were called), so the program shares the objects every host program without a tuning define links.  CPU only; nothing is
loaded into Python and nothing is preloaded.  What is checked is the host side: every error except SWR_ERR_NOMEM and SWR_ERR_UNSUPPORTED
leaves mode and scene; the launches of enqueue_pose and their order under each mode for no deformation, a dense and a sparse morph, a
matrix and a dual-quaternion pose and the combined call, with the vertex passes handed no normals under a computed mode and today's
launches exactly under UPLOADED; the adjacency the counting sort built for the hub scene, entry for entry; the stream every band holds,
for 1 and 3 bands; the mode before attributes, behind an un-waited and an overflowed frame, across skin, targets, poses, new attributes
and a restream, dropped by an upload; empty scenes; and the sticky error."""
import host_build

ASAN = "address,undefined"


def test_normals_host_layer_under_address_sanitizer(tmp_path):
    exe = host_build.build_program(tmp_path, "normals_host_test.cpp", ASAN)
    host_build.run_clean(exe, "normals host test: ok", ASAN)
