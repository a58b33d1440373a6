"""The host layer frees nothing by hand (CPU, reads the source text): in software-renderer_amd/csrc/swr_api.hip the HIP calls that give a
resource back occur only inside the owner types, whose destructors make them, and the names the host layer has retired stay retired."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = os.path.join(ROOT, "software-renderer_amd")
API = os.path.join(PRODUCT, "csrc", "swr_api.hip")
OWNERS = ("DevBuf", "HostBuf", "Pinned", "Event", "Stream")
RELEASES = {"hipFree(": ("DevBuf",), "hipHostFree(": ("HostBuf", "Pinned"), "hipEventDestroy(": ("Event",), "hipStreamDestroy(": ("Stream",)}


def _code(src):
    return re.sub(r"//[^\n]*", "", src)


def _block_end(text, at):
    """The index behind the brace that closes the one opened at text[at]."""
    depth = 0
    for i in range(at, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return i + 1
    raise ValueError("unbalanced braces")


def _owners(code):
    """name -> (start, end) of the definition of every owner type."""
    spans = {}
    for name in OWNERS:
        m = re.search(r"\bstruct %s \{" % name, code)
        assert m, "owner type %s is gone" % name
        spans[name] = (m.start(), _block_end(code, m.end() - 1))
    return spans


def test_resources_are_released_only_by_the_owner_types():
    code = _code(open(API).read())
    spans = _owners(code)
    for call, owners in RELEASES.items():
        sites = [m.start() for m in re.finditer(re.escape(call), code)]
        inside = {o: [s for s in sites if spans[o][0] <= s < spans[o][1]] for o in owners}
        for o in owners:
            assert inside[o], "%s does not call %s" % (o, call[:-1])
        stray = [s for s in sites if not any(s in v for v in inside.values())]
        assert not stray, "%s outside %s, line %s" % (call[:-1], " / ".join(owners), [code.count("\n", 0, s) + 1 for s in stray])


def test_owner_types_cannot_be_copied():
    code = _code(open(API).read())
    for name, (a, b) in _owners(code).items():
        body = code[a:b]
        assert "~%s()" % name in body
        assert re.search(r"%s\(const %s&\) = delete" % (name, name), body) or re.search(r"%s\(%s&& o\)" % (name, name), body), name


@pytest.mark.parametrize("word", ["group_tg", "group_has_target", "STANDIN", "SWR_HOST_TEST_"])
def test_retired_names_stay_retired(word):
    hits = []
    for folder, _, files in os.walk(PRODUCT):
        if os.path.basename(folder) in ("build", "lib", "__pycache__"):
            continue
        for f in files:
            if f.endswith((".so", ".o", ".pyc")):
                continue
            with open(os.path.join(folder, f), errors="replace") as fh:
                if word in fh.read():
                    hits.append(os.path.relpath(os.path.join(folder, f), ROOT))
    assert not hits, hits
