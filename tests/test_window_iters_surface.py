"""CPU checks of the window entries' iteration surface: the header declares mr_windows_batch_ex and
mr_rca_window_ex as their plain entries' arguments plus five, the ctypes table binds them alike, the
built library exports them, and the Python entries reject bad keywords before the library is loaded
(no device needed)."""
import inspect
import os
import re

import pytest

from conftest import REPO

EXTRA = ["iters", "tol", "check_every", "iters_done", "resid"]


def _header_args(name):
    raw = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("plain", ["mr_windows_batch", "mr_rca_window"])
def test_header_declares_ex_entries(plain):
    base, ex = _header_args(plain), _header_args(plain + "_ex")
    assert ex[:len(base)] == base   # every argument of the plain entry, in its order
    assert [a.split()[-1].lstrip("*") for a in ex[len(base):]] == EXTRA
    assert ex[len(base):] == ["int iters", "double tol", "int check_every", "int32_t* iters_done", "double* resid"]


def test_header_comments():
    raw = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    comment = raw[:raw.index("int mr_windows_batch_ex")].rsplit("/*", 1)[1]
    for word in ("pagerank.py:117", "README.md:37", "25, 0.0, 1, NULL", "iters_done", "bitwise", "k_resid", "MR_ERR_ARG",
                 "MR_FP32"):
        assert word in comment, word
    comment = raw[:raw.index("int mr_rca_window_ex")].rsplit("/*", 1)[1]
    assert "25, 0.0, 1, NULL, NULL" in comment
    conv = raw[:raw.index("int mr_pagerank_converge")].rsplit("/*", 1)[1]
    assert "mr_windows_batch_ex" in conv and "mr_rca_window_ex" in conv
    assert "no convergence form" not in conv


def test_signature_table():
    from microrank_amd import _lib

    C = _lib.C
    tail = [C.c_int, C.c_double, C.c_int, _lib.i32p, _lib.f64p]
    for plain in ("mr_windows_batch", "mr_rca_window"):
        res, args = _lib.SIGNATURES[plain + "_ex"]
        assert res is C.c_int
        assert args == _lib.SIGNATURES[plain][1] + tail
        assert len(args) == len(_header_args(plain + "_ex"))


def test_library_exports_ex_entries():
    from microrank_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmicrorank_hip.so not built (run __graft_entry__.build())")
    assert {"mr_windows_batch_ex", "mr_rca_window_ex"} <= _lib.exported_symbols()


def test_python_defaults_are_the_references():
    from microrank_amd import online_rca

    for fn in (online_rca.rank_windows, online_rca.rca_window):
        sig = inspect.signature(fn)
        for name, default in (("iters", 25), ("tol", None), ("check_every", 5), ("info", None)):
            assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, name)
            assert sig.parameters[name].default == default, (fn.__name__, name)
    for fn in (online_rca.online_anomaly_detect_RCA, online_rca.RCAStream.__init__):
        p = inspect.signature(fn).parameters["iters"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 25
    for fn in (online_rca.sweep_rank, online_rca._window_loop):
        assert inspect.signature(fn).parameters["iters"].default == 25


class _NoDevice:
    """Stands where a context or a table would: any use of it is an error of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the argument check touched the device object (.{name})")


BAD = [dict(iters=0), dict(iters=2.5), dict(iters=True), dict(tol=-1.0), dict(tol=float("nan")), dict(tol="1e-9"),
       dict(check_every=0), dict(tol=1e-9, check_every=0)]


@pytest.mark.parametrize("kw", BAD + [dict(info={}), dict(info=())],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_rank_windows_rejects_before_any_library_call(kw, monkeypatch):
    from microrank_amd import _lib, online_rca

    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    with pytest.raises(ValueError):
        online_rca.rank_windows(_NoDevice(), [(_NoDevice(), 0, 1, None, None)], **kw)


@pytest.mark.parametrize("kw", BAD + [dict(info=[]), dict(info=())],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_rca_window_rejects_before_any_library_call(kw, monkeypatch):
    from microrank_amd import _lib, online_rca

    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))
    with pytest.raises(ValueError):
        online_rca.rca_window(_NoDevice(), 0, 1, {}, ctx=_NoDevice(), table=_NoDevice(), dev=_NoDevice(), **kw)


def test_error_wording_is_check_converge_args():
    from microrank_amd import online_rca
    from microrank_amd.graph import check_converge_args

    for kw, args in ((dict(iters=0), (0.0, 0, 5)), (dict(tol=-1.0), (-1.0, 25, 5)), (dict(check_every=0), (0.0, 25, 0))):
        with pytest.raises(ValueError) as want:
            check_converge_args(*args)
        with pytest.raises(ValueError) as got:
            online_rca.rank_windows(_NoDevice(), [], **kw)
        assert str(got.value) == str(want.value)


@pytest.mark.parametrize("iters", [0, -3, 2.5])
def test_drivers_reject_a_bad_count(iters):
    from microrank_amd import online_rca

    with pytest.raises(ValueError):
        online_rca.online_anomaly_detect_RCA(_NoDevice(), {}, [], iters=iters)
    with pytest.raises(ValueError):
        online_rca.RCAStream({}, [], ctx=_NoDevice(), iters=iters)
