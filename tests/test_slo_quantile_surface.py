"""CPU checks of the percentile-SLO surface: the header declares mr_slo_quantiles, the built
library exports it, the ctypes table has it, and the Python drop-ins take the new keyword-only
arguments without changing their positional names."""
import inspect
import os
import re

import pytest

from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "microrank_hip.h")).read()


def test_header_declares_quantiles():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+mr_slo_quantiles\s*\(", text)
    for name, value in (("MR_Q_LINEAR", 0), ("MR_Q_LOWER", 1), ("MR_Q_HIGHER", 2)):
        assert re.search(rf"\b{name}\s*=\s*{value}\b", text), name


def test_library_exports_quantiles():
    from microrank_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmicrorank_hip.so not built (run __graft_entry__.build())")
    import ctypes

    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mr_slo_quantiles")


def test_signature_table_and_constants():
    from microrank_amd import _lib

    res, args = _lib.SIGNATURES["mr_slo_quantiles"]
    C = _lib.C
    assert res is C.c_int
    assert args == [_lib.P, _lib.P, C.c_int64, C.c_int64, _lib.f64p, C.c_int32, C.c_int, _lib.f64p, _lib.i64p]
    assert (_lib.MR_Q_LINEAR, _lib.MR_Q_LOWER, _lib.MR_Q_HIGHER) == (0, 1, 2)


def _kinds(fn):
    return {p.name: p.kind for p in inspect.signature(fn).parameters.values()}


def test_python_surface_keyword_only_additions():
    from microrank_amd import anormaly_detector, preprocess_data

    for fn in (preprocess_data.get_operation_slo, anormaly_detector.get_slo):
        sig = inspect.signature(fn)
        for name in ("quantile", "method"):
            assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, name)
        assert sig.parameters["quantile"].default is None
        assert sig.parameters["method"].default == "linear"
    pos = lambda fn: [p.name for p in inspect.signature(fn).parameters.values() if p.kind != p.KEYWORD_ONLY]
    assert pos(preprocess_data.get_operation_slo) == ["service_operation_list", "span_df"]
    assert pos(anormaly_detector.get_slo) == ["span_df", "start_time", "end_time"]
    assert pos(preprocess_data.get_operation_quantiles) == ["service_operation_list", "span_df", "q"]
    kinds = _kinds(preprocess_data.get_operation_quantiles)
    for name in ("method", "window", "ctx"):
        assert kinds[name] is inspect.Parameter.KEYWORD_ONLY, name


@pytest.mark.parametrize("q", [-0.1, 1.5, float("nan"), [0.5, 2.0], [], "p99"])
def test_bad_q_raises_before_any_device_work(q):
    """A bad q is a ValueError from the argument check itself (no table, no context needed)."""
    from microrank_amd.preprocess_data import get_operation_quantiles

    with pytest.raises(ValueError):
        get_operation_quantiles([], None, q)


def test_bad_method_raises_before_any_device_work():
    from microrank_amd.preprocess_data import get_operation_quantiles, get_operation_slo

    with pytest.raises(ValueError):
        get_operation_quantiles([], None, 0.5, method="nearest")
    with pytest.raises(ValueError):
        get_operation_slo([], None, quantile=0.5, method="midpoint")
    with pytest.raises(ValueError):
        get_operation_slo([], None, quantile=[0.5, 0.9])
