"""The library's environment switches are the ones INTEGRATION.md documents, and no others: every
DDSHE_* name passed to getenv under csrc/ appears in the "Environment switches" table and every table
row is read by the code; no #if / #ifdef / #ifndef on a DDSHE_* macro compiles a variant in or out
(include guards apart). A new switch has to be added to the table, with the test that flips it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc")


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".cpp", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def _table_names():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## Environment switches"):]
    nxt = sec.find("\n## ", 1)
    sec = sec if nxt < 0 else sec[:nxt]
    return {m.group(1) for m in re.finditer(r"^\| `(DDSHE_[A-Z0-9_]+)` \|", sec, re.M)}


def test_getenv_names_equal_the_integration_table():
    read = set()
    for name, src in _sources():
        calls = re.findall(r"\bgetenv\(\s*([^)]*?)\s*\)", src)
        for arg in calls:
            m = re.fullmatch(r'"(DDSHE_[A-Z0-9_]+)"', arg)
            assert m, f"{name}: getenv({arg}) does not name a DDSHE_* switch literally"
            read.add(m.group(1))
    table = _table_names()
    assert table, "no rows found in the Environment switches table"
    assert read == table, (sorted(read - table), sorted(table - read))


def test_no_ddshe_preprocessor_variants():
    found = []
    for name, src in _sources():
        lines = src.split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*DDSHE_\w+.*)", line)
            if not m:
                continue
            guard = re.fullmatch(r"\s*(DDSHE_\w+)\s*", m.group(2)) if m.group(1) == "ifndef" else None
            if guard and i + 1 < len(lines) and re.match(r"\s*#\s*define\s+" + guard.group(1) + r"\s*$", lines[i + 1]):
                continue  # include guard
            found.append((name, i + 1, line.strip()))
    assert not found, found
