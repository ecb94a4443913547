"""CPU checks of the latency evidence's surface: the header's declarations, the library's exports, the
ctypes table and the Python keywords (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "microrank_hip.h")).read()


def test_header_declares_entries_and_constants():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+mr_op_latency\s*\(", code)
    assert re.search(r"\bint\s+mr_windows_latency\s*\(", code)
    assert re.search(r"enum\s*\{\s*MR_LAT_DURATION\s*=\s*0\s*,\s*MR_LAT_SELF\s*=\s*1\s*\}", code)


def test_library_exports_entries():
    from microrank_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libmicrorank_hip.so not built (run __graft_entry__.build())"
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mr_op_latency") and hasattr(lib, "mr_windows_latency")


def test_signatures():
    from microrank_amd import _lib
    from microrank_amd._lib import P, f64p, i32p, i64p, u8p

    vpp = C.POINTER(C.c_void_p)
    assert _lib.SIGNATURES["mr_op_latency"] == (
        C.c_int, [P, P, C.c_int64, C.c_int64, u8p, i32p, C.c_int32, C.c_int, f64p, C.c_int32, C.c_int, f64p, i64p])
    assert _lib.SIGNATURES["mr_windows_latency"] == (
        C.c_int, [P, C.c_int32, C.POINTER(P), i64p, i64p, vpp, vpp, i32p, i32p, C.c_int32, C.c_int, f64p, C.c_int32,
                  C.c_int, f64p, i64p, i32p])
    assert (_lib.MR_LAT_DURATION, _lib.MR_LAT_SELF) == (0, 1)


def _params(fn):
    return inspect.signature(fn).parameters


def _positional(fn):
    return [p.name for p in _params(fn).values() if p.kind != p.KEYWORD_ONLY]


def test_keywords_are_keyword_only_with_defaults():
    from microrank_amd import online_rca as o

    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream.__init__, o.sweep_rank):
        ps = _params(fn)
        for name, default in (("latency", None), ("latency_what", "self")):
            assert ps[name].kind == ps[name].KEYWORD_ONLY, (fn.__name__, name)
            assert ps[name].default == default, (fn.__name__, name)
    for fn in (o.op_latency, o.windows_latency):
        ps = _params(fn)
        for name, default in (("q", (0.5, 0.99)), ("what", "self"), ("method", "linear")):
            assert ps[name].kind == ps[name].KEYWORD_ONLY and ps[name].default == default, (fn.__name__, name)
    for name in ("ctx", "table", "dev"):
        assert _params(o.op_latency)[name].kind == inspect.Parameter.KEYWORD_ONLY
        assert _params(o.op_latency)[name].default is None
    assert _positional(o.op_latency) == ["data", "start_time", "end_time", "slo", "ops"]
    assert _positional(o.windows_latency) == ["ctx", "windows", "ops"]
    # the positional names of the existing entries are what they were
    assert _positional(o.rca_window) == ["data", "start_time", "end_time", "slo"]
    assert _positional(o.rank_windows) == ["ctx", "windows"]
    assert _positional(o.online_anomaly_detect_RCA) == ["data", "slo", "operation_list"]
    assert _positional(o.RCAStream.__init__) == ["self", "slo", "operation_list"]
    assert "latency" not in _params(o.rank_windows)   # rank_windows keeps its tuples


@pytest.mark.parametrize("kw", [{"q": 1.5}, {"q": -0.1}, {"q": float("nan")}, {"q": []}, {"q": [0.5] * 17},
                                {"q": "median"}, {"what": "total"}, {"what": 1}, {"method": "nearest"}])
def test_bad_arguments_raise_before_any_device_work(kw):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.op_latency(None, None, None, None, ["x"], **kw)
    with pytest.raises(ValueError):
        o.windows_latency(None, [], [], **kw)
    lat = {"latency": kw["q"]} if "q" in kw else {"latency": 0.5, "latency_what": kw["what"]} if "what" in kw else None
    if lat is not None:
        with pytest.raises(ValueError):
            o.rca_window(None, None, None, None, **lat)
        with pytest.raises(ValueError):
            o.RCAStream(None, None, ctx=object(), device_append=False, **lat)
