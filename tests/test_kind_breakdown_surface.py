"""CPU checks of the kind breakdown's surface: the header's declaration, the library's export, the ctypes
table and the Python keywords (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import REPO


def test_header_declares_the_entry():
    text = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mr_windows_kind_breakdown\s*\(([^;]*)\)\s*;", code)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 20 and args[-1].startswith("int32_t* status") and args[18].startswith("int64_t* kb_tot")
    assert "no reference counterpart" in text[text.index("kind breakdown"):].lower()


def test_library_exports_the_entry():
    from microrank_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libmicrorank_hip.so not built (run __graft_entry__.build())"
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mr_windows_kind_breakdown")


def test_signature():
    from microrank_amd import _lib
    from microrank_amd._lib import P, i32p, i64p

    vpp = C.POINTER(C.c_void_p)
    assert _lib.SIGNATURES["mr_windows_kind_breakdown"] == (
        C.c_int, [P, C.c_int32, C.POINTER(P), i64p, i64p, vpp, vpp, i32p, i32p, C.c_int32, C.c_int32, i32p, i32p, i32p, i32p,
                  i32p, i32p, i32p, i64p, i32p])


def _params(fn):
    return inspect.signature(fn).parameters


def _positional(fn):
    return [p.name for p in _params(fn).values() if p.kind != p.KEYWORD_ONLY]


def test_keywords_are_keyword_only_with_defaults():
    from microrank_amd import online_rca as o

    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream.__init__, o.sweep_rank):
        p = _params(fn)["kind_breakdown"]
        assert p.kind == p.KEYWORD_ONLY and p.default is None, fn.__name__
    p = _params(o.windows_kind_breakdown)["m"]
    assert p.kind == p.KEYWORD_ONLY and p.default == 8
    assert _positional(o.windows_kind_breakdown) == ["ctx", "windows", "ops"]
    # the positional names of the existing entries are what they were
    assert _positional(o.rca_window) == ["data", "start_time", "end_time", "slo"]
    assert _positional(o.rank_windows) == ["ctx", "windows"]
    assert _positional(o.windows_latency) == ["ctx", "windows", "ops"]
    assert _positional(o.online_anomaly_detect_RCA) == ["data", "slo", "operation_list"]
    assert _positional(o.RCAStream.__init__) == ["self", "slo", "operation_list"]
    assert _positional(o.sweep_rank) == ["plan", "events", "precision", "iters", "exemplars", "exemplar_kinds"]
    assert "kind_breakdown" not in _params(o.rank_windows)   # rank_windows keeps its tuples


@pytest.mark.parametrize("m", [0, 33, -1, 2.5, "8", True, None])
def test_bad_m_raises_before_any_device_work(m):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_kind_breakdown(None, [], [], m=m)
    if m is None:   # (for the keyword None means "not asked")
        return
    with pytest.raises(ValueError):
        o.rca_window(None, None, None, None, kind_breakdown=m)
    with pytest.raises(ValueError):
        o.RCAStream(None, None, ctx=object(), device_append=False, kind_breakdown=m)
    with pytest.raises(ValueError):
        o.online_anomaly_detect_RCA(None, None, None, kind_breakdown=m)
    with pytest.raises(ValueError):
        o.sweep_rank({}, [], kind_breakdown=m)


def test_bad_op_lists_raise_before_any_device_work():
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_kind_breakdown(None, [], [[1]])                     # len(ops) != len(windows)
    with pytest.raises(ValueError):
        o.windows_kind_breakdown(None, [object()], [list(range(65))])  # more than 64 ops in a window
    assert o.windows_kind_breakdown(None, [], []) == []
