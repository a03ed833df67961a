"""CPU-only tests of the tiled top-K (csrc/topk_tiled.hip: paths_topk_tiled / paths_topk_rows_tiled): the C surface, every refusal
(validation precedes any launch, so none needs a GPU) and the choice of entry point by level size (paths_amd.utils.topk_entry).
No kernel runs here."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED_MAX = 65535
A = 4096                                        # an aligned non-null address: never dereferenced, every call below is refused


def test_header_declares_both_entries_with_their_twins_types():
    from paths_amd import _lib
    with open(os.path.join(ROOT, "include", "paths_hip.h")) as f:
        header = f.read()
    assert re.search(r"^#define PATHS_TOPK_TILED_MAX 65535$", header, flags=re.M)
    for name, twin, nargs in (("paths_topk_tiled", "paths_topk", 10), ("paths_topk_rows_tiled", "paths_topk_rows", 15)):
        assert re.search(r"^int %s\(" % name, header, flags=re.M), f"{name} is not declared in include/paths_hip.h"
        assert name in _lib.DECLARATIONS
        res, args = _lib.DECLARATIONS[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert (res, args) == _lib.DECLARATIONS[twin] and args == _lib.SIGNATURES[twin]
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "paths_topk_tiled") and hasattr(raw, "paths_topk_rows_tiled")
    assert _lib.ABI_VERSION == 3 and lib.paths_abi_version() == 3


def test_the_new_entries_live_outside_select_hip():
    """select.hip's entry points are pinned to a fixed map of direct tests (test_cpu_select_reference); these have their own file
    and their own direct test (tests/test_gpu_topk_tiled.py::test_tiled_topk_equals_the_numpy_contract)."""
    import importlib
    with open(os.path.join(ROOT, "paths_amd", "csrc", "select.hip")) as f:
        assert "_tiled" not in f.read()
    with open(os.path.join(ROOT, "paths_amd", "csrc", "topk_tiled.hip")) as f:
        src = f.read()
    assert re.findall(r"^int (paths_\w+)\(", src[src.index('extern "C" {'):], flags=re.M) == ["paths_topk_tiled", "paths_topk_rows_tiled"]
    assert callable(getattr(importlib.import_module("tests.test_gpu_topk_tiled"), "test_tiled_topk_equals_the_numpy_contract"))


# (n_max, keep, ldk, B) that both entries refuse, and the argument the message names
REFUSED = (((0, 1, 1, 1), b"n_max (0)"), ((TILED_MAX + 1, 512, 512, 1), b"n_max (65536)"), ((100, 0, 100, 1), b"keep (0)"),
           ((100, -2, 100, 1), b"keep (-2)"), ((100, 50, 49, 1), b"ldk (49)"), ((100, -1, 99, 1), b"ldk (99)"),
           ((100, 200, 99, 1), b"ldk (99)"), ((100, 50, TILED_MAX + 1, 1), b"ldk (65536)"), ((100, 50, 50, 0), b"B (0)"),
           ((100, 50, 50, -1), b"B (-1)"))
# changes to a valid paths_topk_rows_tiled argument list (index -> value) that are refused
ROWS_OK = [A, 100, A, 1, 100, 50, A, 50, A, A, 12, 100, A, A, None]
ROWS_REFUSED = (({9: None}, b"row_base"), ({12: None}, b"kept_rows"), ({13: None}, b"zero_row"), ({10: 0}, b"row_ld (0)"),
                ({11: 99}, b"slide_rows (99)"))


def refusals():
    """(entry point, argument list, word of the message) of every refusal, for this file and for the GPU test that shows that a
    refused call writes nothing (device pointers are put in place of A there)."""
    for (n_max, keep, ldk, B), word in REFUSED:
        head = [A, max(n_max, 1), A, B, n_max, keep, A, ldk, A]
        yield "paths_topk_tiled", head + [None], word
        yield "paths_topk_rows_tiled", head + [A, 12, max(n_max, 1), A, A, None], word
    for change, word in ROWS_REFUSED:
        yield "paths_topk_rows_tiled", [change.get(i, v) for i, v in enumerate(ROWS_OK)], word
    yield "paths_topk_tiled", [A, 99, A, 1, 100, 50, A, 50, A, None], b"ld (99)"
    for at in (0, 2, 6, 8):
        yield "paths_topk_tiled", [None if i == at else v for i, v in enumerate([A, 100, A, 1, 100, 50, A, 50, A, None])], b"null pointer"


def test_invalid_arguments_are_reported_not_launched():
    """Host-side validation happens before any launch, so this is safe without a GPU."""
    import pytest
    from paths_amd import _lib
    lib = _lib.load()
    n = 0
    for name, args, word in refusals():
        assert getattr(lib, name)(*args) == -1, (name, args)
        msg = lib.paths_last_error()
        assert word in msg and name[len("paths_"):].encode() + b":" in msg, (name, args, msg)
        n += 1
    assert n == 2 * len(REFUSED) + len(ROWS_REFUSED) + 5
    with pytest.raises(_lib.PathsHipError, match=r"paths_topk_tiled failed \(-1\): topk_tiled: n_max \(65536\) must be in \[1, 65535\]"):
        _lib.call("paths_topk_tiled", A, 65536, A, 1, 65536, 512, A, 512, A, None)


def test_topk_entry_switches_at_the_lds_limit():
    from paths_amd import utils as putils
    assert putils.TOPK_LDS_MAX == 8192
    for N in (1, 2048, 8192):
        assert putils.topk_entry(N, False) == "paths_topk" and putils.topk_entry(N, True) == "paths_topk_rows"
    for N in (8193, 20000, TILED_MAX, TILED_MAX + 1):         # (above the cap the C entry refuses, as it did before)
        assert putils.topk_entry(N, False) == "paths_topk_tiled" and putils.topk_entry(N, True) == "paths_topk_rows_tiled"
