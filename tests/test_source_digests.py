"""The generated headers keep their text, and the table of function blocks matches the headers it names.

A generated header is part of the cache key of every code object built from it, so generator code that is reorganised
must leave every header byte for byte as it was: ``tests/golden/native_source_sha256.json`` holds
sha256(native_source()) of the models ``build()`` and the GPU tests compile (tools/make_golden_source_digests.py).
"""
import glob
import json
import os
import re

from sunode_amd.symode.codegen import MATH_BLOCKS, math_block_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_generated_header_keeps_its_text(golden_dir):
    from tools.make_golden_source_digests import digests, names
    with open(os.path.join(golden_dir, "native_source_sha256.json")) as fh:
        want = json.load(fh)
    assert sorted(want) == sorted(names())
    got = digests()
    assert [name for name in sorted(want) if got[name] != want[name]] == []


def test_every_math_header_is_one_block():
    headers = sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "sunode_amd", "csrc", "sa_math*.h")))
    assert sorted(block.header for block in MATH_BLOCKS) == headers
    assert len({block.name for block in MATH_BLOCKS}) == len(MATH_BLOCKS)


def test_every_call_of_a_block_is_defined_in_its_header():
    """``SA_FN double sa_<call>(`` at the start of a line -- or a block's own ``SAM_<BLOCK>_FN``, which is SA_FN on the host
    (csrc/sa_math_bessel.h: noinline on the device)."""
    for block in MATH_BLOCKS:
        text = math_block_text(block.name)
        for call in block.calls:
            assert re.search(r"^SA(M_[A-Z]+)?_FN double sa_%s\(" % call, text, re.M), (block.name, call)
        for _, call in block.printers:
            assert call in block.calls, (block.name, call)
