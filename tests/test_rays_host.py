"""The host layer of the ray casts on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under the
address and undefined-behaviour sanitizers: tests/host/rays_host_test.cpp.  The stand-in of swr::launch_cast_rays is the launch set's (a
CPU loop that touches every element it is handed and answers with an echo of the rays), so the program shares the objects every host
program without a tuning define links.  CPU only; nothing is loaded into Python and nothing is preloaded.  What is checked is the host
side: every error, with the ray's index in the message, launches nothing, writes nothing and leaves scene and pose; n == 0; the upload
in front of the launch and the read-back behind it; one launch, on the first band, for 1 and 3 bands; buffer regrowth from 1 to 65 536
rays and back; the resident stream behind an un-waited, an overflowed and a depth-clip frame and a draw list that cuts it; the pose
after the casts; a scene without triangles; and the sticky error."""
import host_build

ASAN = "address,undefined"


def test_rays_host_layer_under_address_sanitizer(tmp_path):
    exe = host_build.build_program(tmp_path, "rays_host_test.cpp", ASAN)
    host_build.run_clean(exe, "rays host test: ok", ASAN)
