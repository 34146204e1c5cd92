"""The build's dependency table (__graft_entry__.HIP_HEADERS: source -> headers) against the sources' own
#include lines: an object is rebuilt only when its source or a listed header is newer, so a header
missing from the table would leave a stale object behind.  Reads files only."""
import os
import re

import __graft_entry__ as g

INCLUDE = os.path.join(g.ROOT, "include")
QUOTED = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _closure(path, seen):
    for name in QUOTED.findall(open(path).read()):
        inc = os.path.normpath(os.path.join(os.path.dirname(path), name))
        assert os.path.dirname(inc) in (g.CSRC, INCLUDE), f"{path} includes {name}: outside csrc/ and include/"
        assert os.path.isfile(inc), f"{path} includes {name}: no such file"
        if inc not in seen:
            seen.add(inc)
            _closure(inc, seen)
    return seen


def test_header_table_matches_the_includes():
    for src, headers in g.HIP_HEADERS.items():
        found = _closure(os.path.join(g.CSRC, src), set())
        found.discard(os.path.join(INCLUDE, "pob.h"))  # every object depends on it: build_lib adds it itself
        assert sorted(os.path.relpath(p, g.CSRC) for p in found) == sorted(headers), src


def test_every_source_is_built():
    on_disk = {f for f in os.listdir(g.CSRC) if f.endswith((".hip", ".cpp")) and f != "pob_py.cpp"}
    assert on_disk == set(g.HIP_SOURCES)
