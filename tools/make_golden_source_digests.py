"""Writes tests/golden/native_source_sha256.json: {model: sha256(native_source())}.

The generated header is part of every code object's cache key, so a change of generator code that is meant to leave the
headers alone is checked against this file (tests/test_source_digests.py).  Regenerate it only in a change that is
meant to alter generated text, on the commit BEFORE that change is judged.

    python tools/make_golden_source_digests.py [--check]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "native_source_sha256.json")
#: models outside STANDARD_PROBLEMS that build() or the GPU tests compile
EXTRA = ("network8", "pivoting", "huge_pivots", "lv12", "rn12_4", "rnb7_9")


def names():
    from __graft_entry__ import STANDARD_PROBLEMS
    return list(STANDARD_PROBLEMS) + list(EXTRA)


def digests():
    from tools.problem_cache import make_problem
    return {name: hashlib.sha256(make_problem(name).native_source().encode()).hexdigest() for name in names()}


if __name__ == "__main__":
    got = digests()
    if "--check" in sys.argv:
        with open(PATH) as fh:
            want = json.load(fh)
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        print("differ: %s" % bad if bad else "%d digests match" % len(got))
        sys.exit(1 if bad else 0)
    with open(PATH, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s (%d models)" % (PATH, len(got)))
