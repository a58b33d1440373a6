"""The table of capped grids cannot rot (CPU): the entries of tests/grid_caps.py are exactly the capped launch sites of
software-renderer_amd/csrc/*.hip, their thresholds follow from the constants in the sources, the tests they name exist, and the shapes
those tests draw cross the thresholds."""
import ast
import glob
import os
import re

import grid_caps as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "software-renderer_amd", "csrc")


def sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}


def _code(src):
    """The source without its comments (their length kept, so that offsets stay)."""
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), src)


def _close(text, at, open_="(", close=")"):
    """The index behind the bracket that closes the one opened at text[at]."""
    depth = 0
    for i in range(at, len(text)):
        depth += {open_: 1, close: -1}.get(text[i], 0)
        if depth == 0:
            return i + 1
    raise ValueError("unbalanced")


def _args(text):
    """The top-level arguments of a call's argument text (parentheses nest; a template-id with a comma is always parenthesised)."""
    out, depth, cur = [], 0, ""
    for ch in text:
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
            continue
        depth += {"(": 1, ")": -1, "{": 1, "}": -1, "[": 1, "]": -1}.get(ch, 0)
        cur += ch
    return out + [cur.strip()]


def constants(srcs=None):
    """Every `constexpr int NAME = <int or NAME>;` and `#define NAME <int>` of the sources and swr_internal.h."""
    text = "\n".join((srcs or sources()).values()) + open(os.path.join(CSRC, "swr_internal.h")).read()
    c = {m.group(1): int(m.group(2)) for m in re.finditer(r"#\s*define\s+(\w+)\s+(\d+)\b", text)}
    pending = re.findall(r"constexpr\s+(?:int|uint32_t|unsigned)\s+(\w+)\s*=\s*([^;]+);", text)
    for _ in range(3):
        for name, expr in pending:
            try:
                c[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(c)))
            except Exception:
                pass
    return c


def _cap_values(expr):
    """The integers a std::min (or a literal) caps a grid at: the arguments of std::min that are a literal or a ternary of two."""
    vals = []
    for m in re.finditer(r"std::min(?:<[^>]*>)?\(", expr):
        for a in _args(expr[m.end():_close(expr, m.end() - 1) - 1]):
            if re.fullmatch(r"\d+u?", a):
                vals.append(int(a.rstrip("u")))
            t = re.fullmatch(r"\w+ \? (\d+)u? : (\d+)u?", a)
            if t:
                vals += [int(t.group(1)), int(t.group(2))]
    return tuple(sorted(vals))


def _function_at(code, at):
    """(name, text up to `at`) of the function a launch sits in: the last line before it that starts in column 0 with a declarator."""
    head = None
    for m in re.finditer(r"^(?![#}\s])[^\n;]*?\b(\w+)\([^\n;]*$", code[:at], flags=re.M):
        head = m
    assert head is not None
    return head.group(1), code[head.start():at]


def _strided(code, kernel):
    """Does the kernel's body stride by its grid?"""
    m = re.search(r"\bvoid\s+%s\(" % re.escape(kernel), code)
    assert m, kernel
    brace = code.index("{", _close(code, code.index("(", m.start())))
    return "gridDim.x" in code[brace:_close(code, brace, "{", "}")]


def capped_sites(srcs=None):
    """[(file, wrapper, kernel, caps, block)] of every launch whose grid is capped."""
    srcs = srcs or sources()
    consts = constants(srcs)
    out = []
    for name, src in srcs.items():
        code = _code(src)
        for m in re.finditer(r"\b(hipLaunchKernelGGL|launch_on)\(", code):
            args = _args(code[m.end():_close(code, m.end() - 1) - 1])
            if m.group(1) == "launch_on":
                args = args[1:]
            if len(args) < 3 or not re.search(r"\bk_\w+", args[0]):
                continue
            kernel = re.search(r"\bk_\w+", args[0]).group(0)
            grid, block = args[1], args[2]
            wrapper, body = _function_at(code, m.start())
            caps = ()
            lit = re.fullmatch(r"dim3\((\d+)\)", grid)
            if lit:
                if int(lit.group(1)) >= 1 and _strided(code, kernel):
                    caps = (int(lit.group(1)),)
            elif "std::min" in grid:
                caps = _cap_values(grid)
            else:
                var = re.fullmatch(r"(?:dim3\()?(?:\(\w+\))?(\w+)\)?", grid)
                if var:
                    v = var.group(1)
                    for d in re.finditer(r"\b%s\b\s*(?:=|\()([^;]*);" % v, body):
                        caps += _cap_values(d.group(1))
                    caps += tuple(int(x) for x in re.findall(r"if \(%s > (\d+)\)" % v, body))
            if not caps:
                continue
            b = re.fullmatch(r"dim3\((\w+)\)", block)
            b = b.group(1) if b else re.search(r"\b%s\((\w+)\)" % re.escape(block), body).group(1)
            out.append((name, wrapper, kernel, tuple(sorted(set(caps))), int(b) if b.isdigit() else consts[b]))
    return out


def _key(c):
    return (c.file, c.wrapper, re.match(r"k_\w+", c.kernel).group(0), tuple(c.caps), c.block)


def test_every_capped_launch_has_an_entry():
    found = set(capped_sites())
    want = {_key(c) for c in G.CAPS if c.rule != "fold"}
    assert found == want, f"capped launches without an entry: {sorted(found - want)}; entries without a launch: {sorted(want - found)}"
    assert len(found) == 17


def test_thresholds_follow_from_the_constants():
    k = constants()
    assert (k["SKIN_THREADS"], k["SKIN_DQ_THREADS"], k["DELTA_THREADS"], k["SWR_TUNE_SKIN_LDS"]) == (256, 256, 256, 1)
    for c in G.CAPS + G.SCANS:
        if c.rule == "cap":
            assert c.cap in c.caps and c.threshold == c.cap * c.block + 1, c
        elif c.rule == "fold":
            assert (c.cap, c.block) == (k["ITEM_BOUNDS_SLOTS"], k["ITEM_BOUNDS_CHUNK"]) and c.threshold == c.cap * c.block + 1, c
            assert (G.ITEM_SLOTS, G.ITEM_CHUNK) == (c.cap, c.block)
        else:
            assert c.rule == "waves" and c.threshold == k["COUNT_WAVES"] + 1 and c.block == k["COUNT_THREADS"], c
    skin = next(c for c in G.CAPS if c.kernel.startswith("k_skin_vertices<"))
    assert skin.cap == (1024 if k["SWR_TUNE_SKIN_LDS"] else 65536)
    # the sizes the shapes are built from
    assert G.SHAPES["validate_oneshot"]["units"] == 3 * G.oneshot_first_chunk(G.ONESHOT_TRIS) and "{70, 100}" in sources()["swr_api.hip"]
    scan = sources()["swr_clip.hip"]
    assert "hipLaunchKernelGGL(k_clip_scan, dim3(1), dim3(1024)" in scan and "(nb + 1023) / 1024" in scan and k["CLIP_THREADS"] == 256


def _tests_of(path):
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    return {n.name: n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def test_every_entry_names_a_test_whose_shape_crosses_the_threshold():
    for c in G.CAPS + G.SCANS:
        path, _, rest = c.test.partition("::")
        name, _, param = rest.partition("[")
        text = open(os.path.join(ROOT, path)).read()
        fn = _tests_of(path).get(name)
        assert fn is not None, f"{c.kernel}: no test {c.test}"
        src = ast.get_source_segment(text, fn)
        marks = ast.get_source_segment(text, fn.decorator_list[0]) if fn.decorator_list else ""
        assert "gpu" in marks or "pytestmark = pytest.mark.gpu" in text or "gpu_ctx" in src, f"{c.test} is not a GPU test"
        if param:
            ids = param.rstrip("]").split("-")
            decos = " ".join(ast.get_source_segment(text, d) for d in fn.decorator_list)
            assert all(re.search(r"[\"']%s[\"']" % re.escape(i), decos) for i in ids), f"{c.test}: no such case"
        units = G.SHAPES[c.shape]["units"]
        assert units >= c.threshold, f"{c.kernel}: {c.test} reaches {units} {c.unit}, the second trip starts at {c.threshold}"
        if path == "tests/test_grid_caps.py":
            assert not c.evidence and 'G.SHAPES["%s"]' % c.shape in src, f"{c.test} does not take its size from SHAPES[{c.shape!r}]"
        else:
            assert c.evidence and c.evidence in text, f"{c.test}: {c.evidence!r} is gone"


def test_the_smallest_crossing_sizes():
    """Where the size was this table's to choose it is the smallest that crosses with the last workgroup partly filled."""
    s = G.SHAPES
    assert s["skin"]["units"] == 1024 * 256 + 257
    assert s["band"]["units"] - 1280 * 13 < 4096 * 256 < s["band"]["row"] * 1280 + 1280 and s["band"]["units"] % 256 == 0
    assert s["validate"]["units"] == 4096 * 256 + 5 and (s["validate"]["units"] - 3) <= 4096 * 256 + 2
    assert 3 * G.oneshot_first_chunk(G.ONESHOT_TRIS - 64) <= 4096 * 256 < s["validate_oneshot"]["units"]
    for key in ("delta_words", "delta_quads"):          # one tile row less no longer crosses
        d = s[key]
        per_row = d["width"] // (4 if key == "delta_quads" else 1)
        last = d["height"] % 32 or 32
        assert d["units"] == per_row * (d["height"] - d["y0"]) > 4096 * 256 >= per_row * (d["height"] - d["y0"] - last)
    assert (s["delta_words"]["width"] % 4, s["delta_quads"]["width"] % 4) == (2, 0)


# ---- the parser sees what it is there for ----------------------------------------------------------------------------------------------
def test_the_parser_sees_a_new_capped_launch_and_a_changed_constant():
    srcs = sources()
    base = set(capped_sites(srcs))
    grown = dict(srcs)
    at = srcs["swr_morph.hip"].index("    const dim3 grid((unsigned)((nv + MORPH_THREADS - 1) / MORPH_THREADS)), block(MORPH_THREADS);")
    line = "    const dim3 grid((unsigned)std::min<int64_t>((nv + MORPH_THREADS - 1) / MORPH_THREADS, 8192)), block(MORPH_THREADS);\n"
    grown["swr_morph.hip"] = srcs["swr_morph.hip"][:at] + line + srcs["swr_morph.hip"][srcs["swr_morph.hip"].index("\n", at) + 1:]
    new = set(capped_sites(grown)) - base
    assert {(f, w, k, c) for f, w, k, c, _ in new} == {("swr_morph.hip", "launch_morph_vertices", "k_morph_vertices", (8192,))}, new
    # an `if (blocks > N)` and a literal grid in front of a strided kernel
    grown = dict(srcs)
    grown["swr_delta.hip"] = srcs["swr_delta.hip"].replace(
        "    hipLaunchKernelGGL((k_delta_tiles<HAVE_BASE, VEC, false>), grid, block, 0, s, a);",
        "    unsigned blocks = grid.x;\n    if (blocks > 512) blocks = 512;\n"
        "    hipLaunchKernelGGL((k_delta_tiles<HAVE_BASE, VEC, false>), dim3(blocks), block, 0, s, a);")
    assert {(k, c) for _, _, k, c, _ in set(capped_sites(grown)) - base} == {("k_delta_tiles", (512,))}
    grown = dict(srcs)
    grown["swr_kernels.hip"] = srcs["swr_kernels.hip"].replace(
        "    hipLaunchKernelGGL(k_texture_to_float, dim3(2048), dim3(256), 0, s, bgra, n, out);",
        "    hipLaunchKernelGGL(k_texture_to_float, dim3(1024), dim3(256), 0, s, bgra, n, out);")
    moved = set(capped_sites(grown))
    assert ("swr_kernels.hip", "launch_texture_to_float", "k_texture_to_float", (1024,), 256) in moved - base and len(base - moved) == 1
    # a changed constant moves a threshold: the table's number is then stale
    grown = dict(srcs)
    grown["swr_skin.hip"] = srcs["swr_skin.hip"].replace("constexpr int SKIN_THREADS = 256;", "constexpr int SKIN_THREADS = 128;")
    assert ("swr_skin.hip", "launch_skin_vertices", "k_skin_vertices", (1024, 65536), 128) in set(capped_sites(grown)) - base
    assert constants(grown)["SKIN_THREADS"] == 128
