"""The host layer of the sparse morph targets and of swr_morph_pose_set on the fake HIP runtime (tests/host/hip_stub, used as it is),
as a stand-alone program under the address and undefined-behaviour sanitizers: tests/host/morph_sparse_host_test.cpp.  The stand-in of
swr::launch_morph_sparse is the launch set's (a CPU loop over the header's arithmetic that checks the rows and reads and writes every
element it is handed), so the program shares the objects every host program without a tuning define links.  CPU only; nothing is loaded
into Python and nothing is preloaded.  What is checked is the host side: the rows and the pre-filled arrays for 1 and 3 bands and 1, 129
and 200 triangles, the stream every band holds after each call, weights behind an un-waited and behind an overflowed frame, sparse
under a pose and a pose under sparse, re-application after a restream and when attributes arrive or change, dense and sparse targets
replacing each other, removal by either call, an upload, pageable and page-locked sources freed on return, entries over three staging
chunks, all-empty targets, swr_morph_pose_set against the two calls (one skin and one stream launch, the state untouched after each
half's errors), every error except SWR_ERR_NOMEM, and the sticky error."""
import host_build

ASAN = "address,undefined"


def test_morph_sparse_host_layer_under_address_sanitizer(tmp_path):
    exe = host_build.build_program(tmp_path, "morph_sparse_host_test.cpp", ASAN)
    host_build.run_clean(exe, "morph sparse host test: ok", ASAN)
