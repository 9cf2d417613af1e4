"""The index's host layer as one text: the index_* translation units ragmi._build.SOURCES
lists, concatenated in that order. The tests that assert on how the host layer is written read
it through here, so they hold a property of the sources, not of a file name."""
import os


def index_host_source():
    from ragmi import _build
    units = [s for s in _build.SOURCES if s.startswith("index_")]
    assert units, "no index unit in _build.SOURCES"
    return "".join(open(os.path.join(_build.CSRC, s)).read() for s in units)
