"""CPU: the inventory of preprocessor build switches in the native sources.

Every identifier that a conditional directive tests (#if, #ifdef, #ifndef, #elif, defined(..))
in po-brax_amd/csrc/* and include/pob.h -- include guards and compiler-provided names apart --
must be one of the switches that INTEGRATION.md's "Build switches" table documents, and every
switch of the table must still be tested somewhere.  A tunable is a plain #define beside the
comment that records its measurement: no `#ifndef NAME` / `#define NAME value` pair may make one
overridable from the compile line, where only the default would ever be built and tested."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = sorted(glob.glob(os.path.join(ROOT, "po-brax_amd", "csrc", "*"))) + [os.path.join(ROOT, "include", "pob.h")]

_DIRECTIVE = re.compile(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b(.*)$")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$")
_IDENT = re.compile(r"[A-Za-z_]\w*")


def _logical_lines(path):
    """The file's lines with backslash continuations joined and comments removed."""
    with open(path, encoding="utf-8") as f:
        text = f.read().replace("\\\n", " ")
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return [re.sub(r"//.*", "", line) for line in text.split("\n")]


def _scan(path):
    """(tested names, include guards, overridable names) of one source."""
    lines = _logical_lines(path)
    tested, guards, overridable = set(), set(), set()
    for i, line in enumerate(lines):
        m = _DIRECTIVE.match(line)
        if not m:
            continue
        names = {n for n in _IDENT.findall(m.group(2)) if n != "defined"}
        tested |= names
        if m.group(1) == "ifndef" and len(names) == 1:
            (name,) = names
            nxt = next((x for x in lines[i + 1:] if x.strip()), "")
            d = _DEFINE.match(nxt)
            if d and d.group(1) == name:
                # `#define NAME` with no value right after: an include guard; with one: an override
                (overridable if d.group(2).strip() else guards).add(name)
    return tested, guards, overridable


def _documented():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        text = f.read()
    m = re.search(r"^## [^\n]*Build switches[^\n]*\n(.*?)(?=^## |\Z)", text, flags=re.S | re.M)
    assert m, "INTEGRATION.md has no 'Build switches' section"
    rows = [r for r in m.group(1).split("\n") if r.startswith("|") and not set(r) <= set("|-: ")]
    names = [re.match(r"\|\s*`(\w+)`", r) for r in rows[1:]]  # (rows[0]: the table's header)
    assert names and all(names), "every row of the table starts with a switch name in backticks"
    return {n.group(1) for n in names}


def test_build_switches_match_the_documented_table():
    assert len(SOURCES) > 5
    tested, guards, overridable = set(), set(), set()
    for path in SOURCES:
        t, g, o = _scan(path)
        tested |= t
        guards |= g
        overridable |= o
    switches = {n for n in tested - guards if not n.startswith("__")}  # (compiler-provided: __cplusplus, ..)
    assert switches == _documented()
    assert not overridable, overridable  # (POB_..., QK and their like: none, whatever the prefix)
