#!/usr/bin/env python3
"""kernel_diff.py LIB_A LIB_B — are the gfx950 kernels of two builds of the library the same machine code?  (CPU only.)

Pulls the gfx950 code objects out of both libraries' .hip_fatbin sections (as tests/test_raster_register_budget.py does) and prints one
line per kernel symbol: `same` when the kernel's instruction bytes are identical on both sides, `DIFF` when they are not, `only A` /
`only B` for a kernel one side lacks; then for each side VGPRs, SGPRs, VGPR spills, SGPR spills, scratch bytes, static LDS bytes and
code bytes (one set when the two agree).  The last line counts the three kinds.  Exit status 1 when any kernel differs or is missing.
A refactor of device code that must not move the frame kernels is checked with this before any GPU run (profiles/shared_rules/)."""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


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


def functions(elf):
    """name -> the bytes of every function symbol of an ELF64 little-endian code object."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _, kind, _, _, off, size, link, _, _, entsize in sections:
        if kind != 2:       # SHT_SYMTAB
            continue
        strtab = sections[link][4]
        for at in range(off, off + size, entsize):
            name, info, _, shndx, value, fsize = struct.unpack_from("<IBBHQQ", elf, at)
            if info & 0xF != 2 or not fsize or not 0 < shndx < shnum:       # STT_FUNC, defined
                continue
            _, _, _, saddr, soff, _, _, _, _, _ = sections[shndx]
            end = elf.index(b"\0", strtab + name)
            out[elf[strtab + name:end].decode()] = elf[soff + value - saddr:soff + value - saddr + fsize]
    return out


def kernels(lib, tmp):
    """kernel symbol -> (instruction bytes, resources) over every gfx950 code object of the library."""
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    with open(fat, "rb") as f:
        data = f.read()
    found = {}
    for co in code_objects(data):
        path = os.path.join(tmp, "co.elf")
        with open(path, "wb") as f:
            f.write(co)
        code = functions(co)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if not name or name.group(1) not in code:
                continue
            res = dict.fromkeys(FIELDS, 0)
            res.update({k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), block)})
            found[name.group(1)] = (code[name.group(1)], res)
    if not found:
        sys.exit(f"{lib}: no gfx950 kernel found")
    return found


def figures(entry):
    text, r = entry
    return "vgpr %3d sgpr %3d vspill %d sspill %d scratch %d lds %5d code %6d" % (
        r["vgpr_count"], r["sgpr_count"], r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"],
        r["group_segment_fixed_size"], len(text))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = kernels(sys.argv[1], ta), kernels(sys.argv[2], tb)
    symbols = sorted(set(a) | set(b))
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")       # (without one the names stay mangled)
    demangled = subprocess.run([filt], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n") if filt else symbols
    counts = {"same": 0, "DIFF": 0, "only A": 0, "only B": 0}
    print(f"A = {sys.argv[1]}\nB = {sys.argv[2]}")
    for sym, name in zip(symbols, demangled):
        if sym in a and sym in b:
            verdict = "same" if a[sym][0] == b[sym][0] else "DIFF"
            fa, fb = figures(a[sym]), figures(b[sym])
            line = fa if fa == fb else f"A: {fa} | B: {fb}"
        else:
            verdict = "only A" if sym in a else "only B"
            line = figures(a[sym] if sym in a else b[sym])
        counts[verdict] += 1
        print(f"{verdict:6s}  {line}  {name}")
    print("kernels: %d same, %d differ, %d only in A, %d only in B" % (counts["same"], counts["DIFF"], counts["only A"], counts["only B"]))
    return 1 if counts["DIFF"] or counts["only A"] or counts["only B"] else 0


if __name__ == "__main__":
    sys.exit(main())
