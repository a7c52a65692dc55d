"""DESIGN.md section 6b is the table of the run-time PALACE_AMD_* names: it lists every one the sources contain and no other."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"PALACE_AMD_[A-Z0-9_]+")


def _source_names():
    names = set()
    for top in ("palace_amd", "include"):
        for path, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f == "Makefile" or os.path.splitext(f)[1] in (".py", ".hip", ".hpp", ".h"):
                    with open(os.path.join(path, f), encoding="utf-8") as fh:
                        names.update(NAME.findall(fh.read()))
    return names


def test_switch_table_matches_sources():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        design = fh.read()
    start = design.index("\n## 6b. ")
    table = set(NAME.findall(design[start:design.index("\n## ", start + 1)]))
    sources = _source_names()
    assert "PALACE_AMD_LIB" in sources, "the source scan found nothing"
    assert sources - table == set(), "read by the sources, missing in DESIGN.md 6b"
    assert table - sources == set(), "in DESIGN.md 6b, in no source file"
