"""CPU-only checks of the load action's boundary (SWR_FLAG_LOAD, swr_target_write; ABI 6): the header, the Python binding and
the library agree.  The GPU behaviour is tested in tests/test_load_action.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_load_flag_and_target_write_are_in_the_abi(swr):
    swr.build()
    text = open(os.path.join(ROOT, "include", "swr.h")).read()
    m = re.search(r"SWR_FLAG_LOAD\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and int(m.group(1)) == 4
    assert swr.binding.FLAG_LOAD == 1 << 4
    assert re.search(r"#define SWR_ABI_VERSION 6\b", text)
    assert re.search(r"\bint swr_target_write\(swr_context\* ctx, const void\* color_full_image, const float\* depth_full_image\);", text)
    assert "swr_target_write" in swr.binding.ABI_SYMBOLS
    lib = ctypes.CDLL(swr.library_path())
    assert hasattr(lib, "swr_target_write")
    assert lib.swr_abi_version() == 6
    # a NULL context is refused before anything else (no device needed)
    lib.swr_target_write.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.swr_target_write(None, None, None) == -1


def test_render_pass_mirror_has_a_load_action():
    text = open(os.path.join(ROOT, "software-renderer_amd", "host", "Renderer.hpp")).read()
    assert "enum class LoadAction { clear, load };" in text
    assert "LoadAction loadAction = LoadAction::clear;" in text
