"""The arithmetic rules several kernels must agree on bit for bit have one definition each, in software-renderer_amd/csrc/swr_rules.hip.h
(DESIGN.md §27).  CPU, reads the source text: fails when a second definition comes back — a retired name, or the telltale spelling of a
rule outside the header."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "software-renderer_amd", "csrc")
RULES = "swr_rules.hip.h"
RETIRED = ["ib_orderable", "ib_from_orderable", "ordered_bits", "from_ordered_bits", "IB_COORD_LIMIT", "ib_find"]
TELLTALES = {
    "the monotone float <-> uint map": ">> 31) | 0x80000000",
    "the 2^30 coordinate limit": "1073741824",
    "the box poison": "0x7FC00000u",
}


def sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*")))}


def test_the_retired_names_are_gone():
    for name, text in sources().items():
        for word in RETIRED:
            assert not re.search(r"\b%s\b" % word, text), f"{name} spells {word} again: the rule lives in {RULES}"
        assert not re.search(r"#\s*define\s+COORD_LIMIT\b", text), f"{name} defines COORD_LIMIT as a macro: it is a constexpr float of {RULES}"


@pytest.mark.parametrize("rule", list(TELLTALES))
def test_a_rule_is_spelled_in_the_header_only(rule):
    srcs = sources()
    assert TELLTALES[rule] in srcs[RULES], f"{rule}: {TELLTALES[rule]!r} is not in {RULES}"
    again = [name for name, text in srcs.items() if name != RULES and TELLTALES[rule] in text]
    assert not again, f"{rule} is spelled out again in {again}: include {RULES} instead"


def test_only_kernel_files_include_the_header():
    users = {name for name, text in sources().items() if '#include "%s"' % RULES in text}
    assert users and all(name.endswith(".hip") for name in users) and "swr_api.hip" not in users, users
