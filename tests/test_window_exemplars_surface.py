"""CPU checks of the window-batch exemplar surface: the header declares mr_windows_batch_exemplars as
mr_windows_batch_ex's arguments plus four, the ctypes table binds it, and rank_windows, the driver and
RCAStream reject a bad `exemplars` before any library call (no device needed)."""
import inspect
import os
import re

import pytest

from conftest import REPO

BAD_M = [0, 33, True, "3"]


class _NoDevice:
    """Stands where a context or a frame would: any use of it is an error of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the argument check touched the device object (.{name})")


@pytest.fixture
def no_library(monkeypatch):
    from microrank_amd import _lib

    def load(*a, **k):
        raise AssertionError("the argument check loaded the library")

    monkeypatch.setattr(_lib, "load", load)


def _args(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared"
    return [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]


def test_header_declares_the_entry():
    raw = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert _args(text, "mr_windows_batch_exemplars") == _args(text, "mr_windows_batch_ex") + ["ex_m", "ex_trace", "ex_score",
                                                                                              "ex_n"]
    comment = raw[:raw.index("int mr_windows_batch_exemplars")].rsplit("/*", 1)[1]
    for word in ("1..32", "top_max + 6", "-1 padded", "0.0 padded", "MR_ERR_ARG", "coverage", "trace code ascending"):
        assert word in comment, word


def test_signature_table_and_exports():
    from microrank_amd import _lib

    C = _lib.C
    base = _lib.SIGNATURES["mr_windows_batch_ex"]
    assert _lib.SIGNATURES["mr_windows_batch_exemplars"] == (C.c_int, base[1] + [C.c_int32, _lib.i32p, _lib.f64p, _lib.i32p])
    if os.path.exists(_lib.LIB_PATH):
        assert "mr_windows_batch_exemplars" in _lib.exported_symbols()


def test_python_surface():
    from microrank_amd import online_rca

    for fn in (online_rca.rank_windows, online_rca.sweep_rank, online_rca.online_anomaly_detect_RCA,
               online_rca.RCAStream.__init__):
        assert inspect.signature(fn).parameters["exemplars"].default is None, fn


@pytest.mark.parametrize("m", BAD_M)
def test_rank_windows_rejects_exemplars(m, no_library):
    from microrank_amd.online_rca import rank_windows

    with pytest.raises(ValueError, match="m must be"):
        rank_windows(None, [], exemplars=m)
    with pytest.raises(ValueError, match="m must be"):
        rank_windows(_NoDevice(), [(_NoDevice(), 0, 1, _NoDevice(), _NoDevice())], exemplars=m)


@pytest.mark.parametrize("m", BAD_M)
def test_driver_rejects_exemplars(m, no_library):
    from microrank_amd.online_rca import RCAStream, online_anomaly_detect_RCA

    with pytest.raises(ValueError, match="m must be"):
        online_anomaly_detect_RCA(_NoDevice(), {}, [], exemplars=m)
    with pytest.raises(ValueError, match="m must be"):
        RCAStream({}, [], ctx=_NoDevice(), exemplars=m)
