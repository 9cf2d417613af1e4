"""CPU tests of the int8 prescan's control surface (include/ragmi.h "int8 prescan"): the routing
rule (mode x dim x storage x k x count) as the header states it and the library
applies it (RAG_PRESCAN_ROUTES, compiled here into a small host program), the agreement of
the header, the ctypes table and the Python constants, and the argument checks that need no
device."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ragmi.h")
NEW = {"rag_index_set_prescan": 2, "rag_index_prescan": 1, "rag_index_prescan_bounds": 6}


@pytest.fixture(scope="module")
def lib():
    from ragmi import _build, _lib
    _build.build()
    return _lib.load()


def _header_int(name):
    text = open(HEADER).read()
    m = re.search(rf"#define {name}\s+(\d+)", text) or re.search(rf"\b{name}\s*=\s*(\d+)", text)
    assert m, name
    return int(m.group(1))


def test_header_table_and_python_constants_agree(lib):
    from ragmi import _lib, index
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} not declared"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
        res, args = _lib.INDEX_API[name]
        assert res is ctypes.c_int and len(args) == n_args
        assert hasattr(lib, name)
    assert (index.PRESCAN_OFF, index.PRESCAN_AUTO, index.PRESCAN_ALWAYS) == tuple(
        _header_int(n) for n in ("RAG_PRESCAN_OFF", "RAG_PRESCAN_AUTO", "RAG_PRESCAN_ALWAYS"))
    assert index.PRESCAN_MIN_ROWS == _header_int("RAG_PRESCAN_MIN_ROWS")
    # below half a million rows a step is launch-bound: the copy buys nothing there
    assert index.PRESCAN_MIN_ROWS >= 500_000
    assert hasattr(index.FlatIndex, "set_prescan")


def test_argument_checks_need_no_device(lib):
    assert lib.rag_index_set_prescan(None, 1) == -1 and b"NULL" in lib.rag_last_error()
    assert lib.rag_index_prescan(None) == -1
    fake = ctypes.c_void_p(16)
    assert lib.rag_index_prescan_bounds(None, fake, 1, fake, 1, fake) == -1
    assert b"NULL" in lib.rag_last_error()


def test_routing_rule(tmp_path):
    """mode x dim x storage x k x count -> int8 prescan or not (filtered passes route alike)"""
    thr = _header_int("RAG_PRESCAN_MIN_ROWS")
    cases = [  # mode, dim, storage, k, count, expected
        (1, 384, 0, 15, thr, 1), (1, 384, 0, 15, thr - 1, 0), (1, 384, 0, 15, 100_000, 0),
        (1, 384, 0, 15, 10_000_000, 1), (1, 384, 0, 1, 10_000_000, 1),
        (1, 384, 0, 32, thr, 1), (1, 384, 0, 33, 10_000_000, 0),
        (1, 384, 0, 4096, 10_000_000, 0), (1, 1024, 0, 15, 10_000_000, 0),
        (1, 384, 1, 15, 10_000_000, 0), (0, 384, 0, 15, 10_000_000, 0),
        (2, 384, 0, 15, 0, 1), (2, 384, 0, 1, 3000, 1), (2, 384, 0, 33, 3000, 0),
        (2, 1024, 0, 15, 3000, 0), (2, 384, 1, 15, 3000, 0), (0, 384, 0, 15, 3000, 0),
    ]
    rows = "\n".join(
        f'  printf("%d\\n", (int)RAG_PRESCAN_ROUTES({m}, {d}, {s}, {k}, (int64_t){c}));'
        for m, d, s, k, c, _ in cases)
    src = tmp_path / "routes.c"
    src.write_text('#include <stdio.h>\n#include "ragmi.h"\nint main(void) {\n' + rows +
                   "\n  return 0;\n}\n")
    exe = tmp_path / "routes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [c[-1] for c in cases]
    # and the library routes by this very macro
    from _index_src import index_host_source
    assert ("RAG_PRESCAN_ROUTES(h->prescan, h->dim, h->storage, k, h->count)"
            in index_host_source())
