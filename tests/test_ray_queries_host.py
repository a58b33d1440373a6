"""The host layer of the ray queries on the fake HIP runtime (tests/host/hip_stub, used as it is), as a stand-alone program under the
address and undefined-behaviour sanitizers: tests/host/ray_queries_host_test.cpp.  The stand-in of swr::launch_cast_rays is the launch
set's: it refuses a launch whose groups are not those of the whole stream, touches every element it is handed, answers with an echo of
the rays and notes its RaysArgs.  CPU only; nothing is loaded into Python and nothing is preloaded.  What is checked is the host side:
every new refusal (and the carried-over ones, with swr_query_rays and the ray's index in the message) launches nothing and writes
nothing; query == NULL and the all-defaults query hand the launch the RaysArgs swr_cast_rays hands it; flags, p_begin and p_end arrive as
given, -1 resolved to the triangle count, ntri and groups those of the whole stream; empty ranges; one launch for 1 and 3
bands, on one band's stream and boxes as a pose put them on record, the same in every call; the call behind an un-waited frame and behind a draw list that cuts the stream; a scene without triangles; and the sticky
error."""
import host_build

ASAN = "address,undefined"


def test_ray_queries_host_layer_under_address_sanitizer(tmp_path):
    exe = host_build.build_program(tmp_path, "ray_queries_host_test.cpp", ASAN)
    host_build.run_clean(exe, "ray queries host test: ok", ASAN)
