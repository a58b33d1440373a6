"""The register figures DESIGN.md §5.2 and §6 promise for the raster kernels of the headline and of its colour variant, read from the
built library itself (CPU): no SGPR spill code (scalar registers parked in VGPR lanes: v_writelane / v_readlane), at most 88 VGPRs,
no VGPR spills, no scratch.  The kernels keep them with empty asm statements and readfirstlane calls that steer the compiler's register
allocation (raster_tile: own_s / own_v, ctid, interior_path, Rp0 / Rp1, nchunks); a toolchain that allocates differently must fail
here, not pass unnoticed until someone runs tools/vgprs.sh."""
import os
import re
import struct
import subprocess

import pytest

LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNELS = {
    "k_raster_depth<false>": "_ZN3swr14k_raster_depthILb0EEEvNS_10RasterArgsE",
    "k_raster_depth<true>": "_ZN3swr14k_raster_depthILb1EEEvNS_10RasterArgsE",
    "k_raster<true, 0, false, true>": "_ZN3swr8k_rasterILb1ELi0ELb0ELb1ELb0ELb0ELb0EEEvNS_10RasterArgsE",
}


def code_objects(fatbin):
    """The gfx950 code objects of a .hip_fatbin section: one offload bundle per translation unit, back to back."""
    at = fatbin.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", fatbin, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", fatbin, p)
            ident = fatbin[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident and size:
                yield fatbin[at + off:at + off + size]
        at = fatbin.find(MAGIC, at + 1)


@pytest.fixture(scope="module")
def kernel_metadata(swr, tmp_path_factory):
    lib = swr.build()
    tmp = tmp_path_factory.mktemp("code_objects")
    fat = str(tmp / "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    with open(fat, "rb") as f:
        data = f.read()
    found = {}
    for i, co in enumerate(code_objects(data)):
        path = str(tmp / f"co{i}.elf")
        with open(path, "wb") as f:
            f.write(co)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name:
                found[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|"
                                                                         r"private_segment_fixed_size):\s+(\d+)", block)}
    assert found, "no kernel metadata found in the library's code objects"
    return found


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_headline_raster_kernels_keep_their_register_budget(kernel_metadata, kernel):
    assert KERNELS[kernel] in kernel_metadata, f"{kernel} is not in the library"
    m = kernel_metadata[KERNELS[kernel]]
    assert m["sgpr_spill_count"] == 0, f"{kernel}: {m['sgpr_spill_count']} SGPRs spilled to VGPR lanes (DESIGN.md §5.2)"
    assert m["vgpr_count"] <= 88, f"{kernel}: {m['vgpr_count']} VGPRs, the budget is 88 (DESIGN.md §6)"
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, f"{kernel}: VGPR spills or scratch: {m}"
