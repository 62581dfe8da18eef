"""The build's dependency rule: an object is rebuilt when its own source or any
header is newer, which is the whole truth only while every quoted include in
csrc/ names a header (csrc/*.hpp or include/rudp.h) and no .hip includes a
.hip.  CPU-only: nothing is compiled here.
"""
import itertools
import re

from conftest import PKG, REPO
from rudp import _build

CSRC = PKG / "csrc"
INCLUDE_LINE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', flags=re.M)


def quoted_includes():
    """(file, included name) for every #include "..." line in csrc/."""
    files = sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".hpp", ".cpp", ".h"))
    assert files
    return [(p, name) for p in files for name in INCLUDE_LINE.findall(p.read_text())]


def test_stale_truth_table():
    old, mid, new = 100.0, 200.0, 300.0
    # forced, or no object yet: always rebuilt
    for src, hdr, obj in itertools.product((old, mid, new), (old, mid, new), (None, old, mid, new)):
        assert _build._stale(src, hdr, obj, True)
        assert _build._stale(src, hdr, None, False)
    # the object is at least as new as both: kept
    assert not _build._stale(old, old, mid, False)
    assert not _build._stale(old, mid, mid, False)
    assert not _build._stale(mid, old, mid, False)
    assert not _build._stale(mid, mid, mid, False)
    assert not _build._stale(old, mid, new, False)
    # the source alone, a header alone, or both are newer: rebuilt
    assert _build._stale(new, old, mid, False)
    assert _build._stale(old, new, mid, False)
    assert _build._stale(new, new, mid, False)
    # and in full: stale exactly when the object is older than the newer of the two
    for src, hdr, obj in itertools.product((old, mid, new), repeat=3):
        assert _build._stale(src, hdr, obj, False) == (obj < max(src, hdr))


def test_no_source_includes_a_hip_file():
    found = [(p.name, name) for p, name in quoted_includes() if name.endswith(".hip")]
    assert found == []


def test_every_quoted_include_is_a_header_the_build_watches():
    watched = {p.resolve() for p in CSRC.glob("*.hpp")} | {(REPO / "include" / "rudp.h").resolve()}
    assert watched == {p.resolve() for p in list(_build.CSRC.glob("*.hpp")) + list(_build.INCLUDE.glob("*.h"))}
    includes = quoted_includes()
    assert len(includes) > 20  # (the scan sees the sources)
    for p, name in includes:
        # as the compiler resolves it: beside the including file, then -I include/
        hits = [c.resolve() for c in (p.parent / name, _build.INCLUDE / name) if c.exists()]
        assert hits and hits[0] in watched, (p.name, name)
