"""The table of target-size thresholds cannot rot (CPU): the constants of tests/target_sizes.py stand in the sources where the table
says, the sizes of its rows lie on the sides it says, the cases of tests/test_large_targets.py reach them, every kernel that can ask
for more than 64 KB of dynamic LDS at a legal target is named in prepare_device, and every row is used by a collected GPU case."""
import ast
import os
import re

import pytest

import target_sizes as TS
import test_grid_caps_table as GT
import test_large_targets as LT

ROOT = GT.ROOT
KRN, API = "swr_kernels.hip", "swr_api.hip"


def sources():
    return GT.sources()


def function_text(src, name):
    """The bodies of every definition of `name` in a source (a declaration has none), comments blanked."""
    code = GT._code(src)
    out = []
    for m in re.finditer(r"\b%s\(" % re.escape(name), code):
        end = GT._close(code, m.end() - 1)
        rest = code[end:end + 40].lstrip()
        line = code[code.rfind("\n", 0, m.start()) + 1:m.start()]
        if rest.startswith("{") and re.search(r"\b(void|bool|int|uint2|uint32_t|PixBox|BinPlan|BinKernel|hipError_t)\b", line):
            brace = code.index("{", end)
            out.append(code[brace:GT._close(code, brace, "{", "}")])
    assert out, f"no definition of {name}"
    return "\n".join(out)


def number(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: not found"
    return int(m.group(1))


def constants(srcs):
    """The thresholds as the sources have them."""
    k, a = srcs[KRN], srcs[API]
    setup, plan, cap = function_text(k, "setup_triangle_r"), function_text(k, "plan_binning"), function_text(k, "fixed_cap_max")
    scan = function_text(k, "k_scan")
    c = {
        "small_x": number(r"\(int64_t\)maxx - \(int64_t\)minx < (\d+)\)", setup, "the small bound in x"),
        "small_y": number(r"\(int64_t\)s2y - \(int64_t\)s0y < (\d+) - TILE_H\)", setup, "the small bound in y") - TS.TILE_H,
        "dense_x": number(r"big = !t\.ch\.small \|\| maxx - minx >= (\d+) \|\|", function_text(k, "raster_tile"), "the raster's big"),
        "plan_kb": number(r"p\.use_lds = p\.lds_bytes <= (\d+) \* 1024 &&", plan, "plan_binning's LDS bound"),
        "groups_kb": number(r"\+ 1\) \* 4 > (\d+) \* 1024\) p\.use_lds = false", plan, "plan_binning's group-list bound"),
        "cap_kb": number(r"\+ 64 > (\d+) \* 1024\) return 0u", cap, "fixed_cap_max's bound"),
        "scan_threads": number(r"const int per = \(n \+ (\d+)\) / 1024;", scan, "k_scan's tiles per thread") + 1,
        "attr_kb": number(r"hipFuncAttributeMaxDynamicSharedMemorySize, (\d+) \* 1024\)", function_text(k, "prepare_device"),
                          "prepare_device's limit"),
        "max_dim": number(r"width > (\d+) \|\| height > \1\)", function_text(a, "check_target_args"), "check_target_args"),
        "bin_g": number(r"#define SWR_TUNE_BIN_G (\d+)\b", k, "SWR_TUNE_BIN_G"),
    }
    assert "p.lds_bytes = (size_t)ntiles * 4;" in plan and "p.threads = 256;" in plan
    assert "__launch_bounds__(1024) void k_scan(" in k and "hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024)," in k
    assert "(uint32_t)x0 | ((uint32_t)x1 << 16)" in setup and "((uint32_t)(y1 - a.tg.row_begin) << 16)" in setup
    assert "b.x0 = r.x & 0xFFFF; b.x1 = r.x >> 16; b.y0 = r.y & 0xFFFF; b.y1 = r.y >> 16;" in function_text(k, "unpack_box")
    return c


def check_constants_stand(srcs):
    for r in TS.ROWS:
        assert r.constant in function_text(srcs[r.file], r.function), f"{r.key}: `{r.constant}` is not in {r.function} ({r.file})"


def check_sides(srcs):
    """Every row's sizes against the constants of the sources, and the targets of the cases against the rows."""
    c, row, tiles = constants(srcs), TS.BY_KEY, TS.tiles
    ntri = TS.SMALL_TRIANGLES + TS.LONG_TRIANGLES
    assert c["max_dim"] == TS.MAX_DIM == max(TS.TARGETS["WIDE"]) == max(TS.TARGETS["TALL"]) and TS.MAX_DIM - 1 < 1 << 16
    for key in ("small_x", "small_y", "dense_x"):
        assert (row[key].below, row[key].above) == (c[key] - 1, c[key]), f"{key}: the source says {c[key]}"
    assert row["small_x"].at_least >= row["small_x"].above and row["small_x"].at_least <= TS.MAX_DIM - 6
    # X16K: its widest triangle stays GEOM_SMALL, so that only the second bound decides
    assert row["dense_x"].above < TS.TARGETS["X16K"][0] <= c["small_x"] and TS.TARGETS["X16K"][0] % TS.TILE_W == 0
    # a box's halves: 16 bits each; the 16th is needed from coordinate 32768 on, and 65534 is the last one
    for key, size in (("box_x", TS.TARGETS["WIDE"][0]), ("box_y", TS.TARGETS["TALL"][1])):
        assert (row[key].below, row[key].above) == ((1 << 15) - 1, 1 << 15) and row[key].at_least == size - 1 == (1 << 16) - 2
    # the LDS plan: tiles * 4 bytes against 136 KB
    limit = c["plan_kb"] * 1024 // 4
    assert (row["plan_lds"].below, row["plan_lds"].above) == (limit, limit + 1)
    assert tiles("LDS_TOP") == limit and limit < tiles("ATOMIC") == row["plan_lds"].at_least
    assert tiles((TS.TARGETS["ATOMIC"][0], TS.TARGETS["ATOMIC"][1] - 1)) == limit, "ATOMIC is one row of pixels more than LDS_TOP"
    assert c["groups_kb"] == c["cap_kb"] == row["plan_groups"].below // 1024 and c["bin_g"] == TS.BIN_G
    assert limit * 4 + (TS.groups_per_workgroup(ntri) + 1) * 4 <= c["groups_kb"] * 1024, "LDS_TOP's scene stays on the LDS path"
    need = (c["groups_kb"] * 1024 - limit * 4) // 4                    # groups per workgroup + 1 must exceed this
    assert need * 64 * TS.BIN_G > 50_000_000, "the second bound of plan_binning takes tens of millions of triangles"
    # k_scan: one workgroup of 1024 threads
    assert c["scan_threads"] == 1024 == row["scan_per"].below and (tiles("ATOMIC") + 1023) // 1024 == 35
    assert (tiles(LT.K.TARGETS["large"]) + 1023) // 1024 == 1, "the older tests' atomic chain has one tile per thread"
    # more than 64 KB of dynamic LDS
    lds = TS.lds_bytes
    assert lds("k_fill_lds", tiles("EXACT"), ntri) > TS.LDS_DEFAULT and row["fill_lds"].at_least == lds("k_fill_lds", tiles("EXACT"), ntri)
    assert lds("k_bin", tiles("EXACT"), ntri) <= TS.LDS_DEFAULT < lds("k_bin", tiles("LDS_TOP"), ntri)
    assert lds("k_setup_hist", tiles("EXACT"), ntri) <= TS.LDS_DEFAULT < lds("k_setup_hist", tiles("LDS_TOP"), ntri)
    assert lds("k_bin", tiles(LT.K.TARGETS["large"]), ntri) < TS.LDS_DEFAULT and lds("k_bin", 120 * 135, ntri) < TS.LDS_DEFAULT
    for kernel in ("k_bin", "k_fill_lds", "k_setup_hist"):
        assert lds(kernel, limit, 1 << 24) <= c["attr_kb"] * 1024, f"{kernel} at the plan's limit fits what prepare_device allows"


def dynamic_lds_kernels(srcs):
    """{kernel: file} of every kernel with an `extern __shared__` array."""
    out = {}
    for name, src in srcs.items():
        code = GT._code(src)
        for m in re.finditer(r"extern __shared__", code):
            out[[k.group(1) for k in re.finditer(r"\bvoid (k_\w+)\(", code[:m.start()])][-1]] = name
    return out


def prepared(srcs):
    """The kernels prepare_device raises the limit for: {name: instantiations}."""
    body = function_text(srcs[KRN], "prepare_device")
    out = {}
    for m in re.finditer(r"whole_lds\(", body):
        arg = body[m.end():GT._close(body, m.end() - 1) - 1]
        if arg.startswith("bin_kernel("):
            loop = re.search(r"for \(int v = 0; v < (\d+); v\+\+\)\s*if \(\(e = whole_lds\(bin_kernel\(v & 1, v & 2, v & 4, v & 8\)\)\)", body)
            assert loop, "prepare_device no longer walks bin_kernel's variants"
            assert "return k_bin<256, MT, DEFER, AFF, LIST>;" in function_text(srcs[KRN], "bin_kernel")
            out["k_bin"] = out.get("k_bin", 0) + int(loop.group(1))
        else:
            k = re.match(r"(k_\w+)<", arg)
            assert k, arg
            out[k.group(1)] = out.get(k.group(1), 0) + 1
    return out


def check_prepared(srcs):
    """Every kernel whose dynamic LDS grows with the tile count is launched with the table's expression and named in prepare_device,
    in all its instantiations."""
    dyn = dynamic_lds_kernels(srcs)
    # (the two skin kernels' tables hold joints: their size does not depend on the target)
    assert dyn == {"k_setup_hist": KRN, "k_fill_lds": KRN, "k_bin": KRN, "k_skin_vertices": "swr_skin.hip",
                   "k_skin_vertices_dq": "swr_skin_dq.hip"}, f"a kernel with dynamic LDS that tests/target_sizes.py does not know: {dyn}"
    limit = constants(srcs)["plan_kb"] * 1024 // 4
    want = {"k_setup_hist": 2, "k_bin": 16, "k_fill_lds": 1}
    got = prepared(srcs)
    for kernel, n in want.items():
        assert TS.lds_bytes(kernel, limit, 1 << 20) > TS.LDS_DEFAULT, kernel
        assert got.get(kernel, 0) == n, f"{kernel} can ask for {TS.lds_bytes(kernel, limit, 1 << 20)} bytes of LDS at {limit} tiles: " \
                                        f"prepare_device names {got.get(kernel, 0)} of its {n} instantiations"
    assert set(got) == set(want)
    k = srcs[KRN]
    assert "hipLaunchKernelGGL((k_setup_hist<256, H16>), dim3(f.plan.G), dim3(256), lds, s," in function_text(k, "launch_setup_bin")
    assert "bin_kernel(b.a.metal != 0, b.defer_ok != 0, aff, f.items != nullptr), dim3(f.plan.G), dim3(256), lds, s, b)" in function_text(k, "launch_bin")
    assert "launch_on(stop, k_fill_lds<256>, dim3(f.plan.G), dim3(256), f.plan.lds_bytes + 4 * 256, s," in function_text(k, "launch_fill")
    assert "prepare_device() != hipSuccess" in srcs[API].replace("(e = prepare_device())", "prepare_device()"), \
        "swr_context_create prepares every device it opens"


def test_the_constants_stand_where_the_table_says():
    check_constants_stand(sources())


def test_every_size_lies_on_the_side_the_table_says():
    check_sides(sources())


def test_every_kernel_with_more_than_64_kb_of_lds_is_prepared():
    check_prepared(sources())


def test_the_scenes_have_the_extents_of_their_rows(oracle):
    """From the oracle's own projection: the pairs are one pixel below and at the bounds, and the long triangles reach at_least."""
    for name, key, axis in (("WIDE", "small_x", 0), ("TALL", "small_y", 1), ("X16K", "dense_x", 0)):
        s = TS.scene(name)
        ext = TS.extents(oracle, s.vertices, s.indices, LT.IDENT, *TS.TARGETS[name])[axis]
        r = TS.BY_KEY[key]
        pair = s.pair2 if name == "TALL" else s.pair
        assert tuple(ext[list(pair)]) == (r.below, r.above), f"{name}: {ext[list(pair)]}"
        assert tuple(ext[list(s.pair)]) == ((32767, 32768) if name != "X16K" else (16383, 16384))
        assert ext.max() >= r.at_least and (ext >= r.above).sum() >= (10 if name != "X16K" else 8)
        assert s.indices.size // 3 == TS.SMALL_TRIANGLES + TS.LONG_TRIANGLES


def _cases():
    """{node id relative to the file: the decorators' text} of the GPU tests of tests/test_large_targets.py."""
    path = os.path.join(ROOT, "tests", "test_large_targets.py")
    text = open(path).read()
    out = {}
    for n in ast.parse(text).body:
        if isinstance(n, ast.FunctionDef) and n.name.startswith("test_"):
            decos = [ast.get_source_segment(text, d) for d in n.decorator_list]
            assert "gpu" in decos, f"{n.name} is not marked gpu"
            params = [d for d in decos if d.startswith("pytest.mark.parametrize")]
            if not params:
                out[n.name] = ""
            for p in params:
                if "TILE_CASES" in p:
                    out.update({f"{n.name}[{t}-{kind}]": p for t, kind in LT.TILE_CASES})
                for name in re.findall(r'"([A-Z0-9_]+)"', p):
                    out[f"{n.name}[{name}]"] = p
    return out


def test_every_row_is_used_by_a_collected_gpu_case():
    cases = _cases()
    used = set()
    for case, keys in LT.CROSSES.items():
        assert case in cases, f"{case} is not collected"
        for key in keys:
            assert TS.BY_KEY[key].case == TS.T + case, f"{key} names {TS.BY_KEY[key].case}, CROSSES has it under {case}"
            used.add(key)
    for r in TS.ROWS:
        assert r.key in used or (not r.case and r.mutation.startswith("not crossed")), f"{r.key}: no case crosses it and the row does not say why"
        assert r.mutation, r.key
    source = open(os.path.join(ROOT, "tests", "test_large_targets.py")).read()
    for name in TS.TARGETS:
        assert f'"{name}"' in source, f"no case draws on {name}"


def test_every_mutation_of_the_table_is_in_the_record():
    record = open(os.path.join(ROOT, "profiles", "large_targets", "mutations.txt")).read()
    for r in TS.ROWS:
        if not r.mutation.startswith(("none", "not crossed")):
            assert r.mutation in record, f"{r.key}: `{r.mutation}` is not in profiles/large_targets/mutations.txt"


# ---- the checks see what they are there for -------------------------------------------------------------------------------------------
EDITS = [
    (KRN, "p.use_lds = p.lds_bytes <= 136 * 1024 &&", "p.use_lds = p.lds_bytes <= 144 * 1024 &&"),
    (KRN, "> 150 * 1024) p.use_lds = false", "> 140 * 1024) p.use_lds = false"),
    (KRN, "(int64_t)maxx - (int64_t)minx < 32768)", "(int64_t)maxx - (int64_t)minx < 65536)"),
    (KRN, "(int64_t)s2y - (int64_t)s0y < 32768 - TILE_H)", "(int64_t)s2y - (int64_t)s0y < 32768)"),
    (KRN, "maxx - minx >= 16384 ||", "maxx - minx >= 32768 ||"),
    (KRN, "const int per = (n + 1023) / 1024;", "const int per = (n + 511) / 512;"),
    (KRN, "(size_t)((b.ntiles + 1) / 2) * 4 + (size_t)(b.per + 1) * 4", "(size_t)b.ntiles * 4 + (size_t)(b.per + 1) * 4"),
    (KRN, "f.plan.lds_bytes + 4 * 256, s,", "f.plan.lds_bytes + 4 * 512, s,"),
    (KRN, "    return whole_lds(k_fill_lds<256>);", "    return hipSuccess;"),
    (KRN, "    for (int v = 0; v < 16; v++)", "    for (int v = 0; v < 8; v++)"),
    (KRN, "    if ((e = whole_lds(k_setup_hist<256, true>)) != hipSuccess) return e;\n", ""),
    (API, "width > 65535 || height > 65535", "width > 32768 || height > 32768"),
]


@pytest.mark.parametrize("k", range(len(EDITS)))
def test_an_edited_constant_fails_a_check(k):
    file, old, new = EDITS[k]
    srcs = sources()
    assert srcs[file].count(old) == 1, f"`{old}` stands {srcs[file].count(old)} times in {file}"
    check_constants_stand(srcs), check_sides(srcs), check_prepared(srcs)
    srcs[file] = srcs[file].replace(old, new)
    failed = []
    for check in (check_constants_stand, check_sides, check_prepared):
        try:
            check(srcs)
        except AssertionError as e:
            failed.append(f"{check.__name__}: {e}")
    print(f"`{old}` -> `{new}`:\n  " + "\n  ".join(failed))
    assert failed, f"no check fails when `{old}` becomes `{new}`"
