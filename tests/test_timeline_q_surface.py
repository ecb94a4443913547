"""CPU checks of the timeline quantiles' surface: the header's declaration, the library's export, the ctypes
table, the drivers' keywords timeline_q / timeline_what, the request's parameters and the timeline_q.csv writer
(no GPU needed; the library is not loaded where the test says so)."""
import csv
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

BAD_Q = [1.5, -0.1, float("nan"), [], [0.5] * 17, "median"]


@pytest.fixture
def no_library(monkeypatch):
    from microrank_amd import _lib

    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))


def test_header_declares_the_entry():
    text = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mr_windows_timeline_q\s*\(([^;]*)\)\s*;", code)
    plain = re.search(r"\bint\s+mr_windows_timeline\s*\(([^;]*)\)\s*;", code)
    assert m and plain
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    old = [" ".join(a.split()) for a in plain.group(1).split(",")]
    # mr_windows_timeline's arguments, q / n_q / method ahead of the outputs, tl_q behind tl_out
    assert args[:14] == old[:14] and args[14:17] == ["const double* q", "int32_t n_q", "int method"]
    assert args[17:21] == old[14:18] and args[21] == "double* tl_q" and args[22] == old[18] and len(args) == 23
    doc = re.sub(r"[\s*]+", " ", text[text.index("mr_windows_timeline with latency quantiles"):
                                      text.index("int mr_windows_timeline_q")])
    for word in ("np.quantile", "1..16", "[0, 1]", "MR_Q_LINEAR", "word for word", "0.0 where the count is 0",
                 "outside buckets get no quantiles", "ONE sort", "value range too wide", "MR_ERR_STATE", "same bits"):
        assert word in doc, word


def test_library_exports_the_entry_and_signature():
    from microrank_amd import _lib
    from microrank_amd._lib import P, f64p, i32p, i64p

    assert os.path.exists(_lib.LIB_PATH), "libmicrorank_hip.so not built (run __graft_entry__.build())"
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mr_windows_timeline_q")
    vpp = C.POINTER(C.c_void_p)
    assert _lib.SIGNATURES["mr_windows_timeline_q"] == (
        C.c_int, [P, C.c_int32, C.POINTER(P), i64p, i64p, vpp, vpp, i32p, i32p, C.c_int32, C.c_int, i64p, i64p, C.c_int32,
                  f64p, C.c_int32, C.c_int, i64p, i64p, i64p, i64p, f64p, i32p])


def test_keywords_are_keyword_only_with_defaults():
    from microrank_amd import evidence
    from microrank_amd import online_rca as o

    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream.__init__, o.sweep_rank, evidence.evidence_request):
        ps = inspect.signature(fn).parameters
        assert ps["timeline_q"].kind == ps["timeline_q"].KEYWORD_ONLY and ps["timeline_q"].default is None, fn.__name__
        assert ps["timeline_what"].kind == ps["timeline_what"].KEYWORD_ONLY and ps["timeline_what"].default == "self"
    for fn, lead in ((o.windows_timeline_q, ["ctx", "windows", "ops"]),
                     (o.window_timeline_q, ["data", "start_time", "end_time", "slo", "ops"])):
        ps = inspect.signature(fn).parameters
        assert [p.name for p in ps.values() if p.kind != p.KEYWORD_ONLY] == lead
        assert ps["q"].default == (0.5, 0.99) and ps["method"].default == "linear" and ps["buckets"].default == 30
        assert ps["what"].default == "self"
    assert o.windows_timeline_q is evidence.windows_timeline_q and o.window_timeline_q is evidence.window_timeline_q
    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream, o.sweep_rank, o.windows_timeline_q):
        assert "timeline_q" in fn.__doc__, fn.__name__


@pytest.mark.parametrize("q", BAD_Q, ids=lambda q: repr(q)[:12])
def test_bad_q_raises_before_the_library_is_loaded(q, no_library):
    from microrank_amd import evidence
    from microrank_amd import online_rca as o

    kw = {"timeline": 8, "timeline_q": q}
    with pytest.raises(ValueError):
        evidence.evidence_request(**kw)
    with pytest.raises(ValueError):
        o.sweep_rank({}, [], **kw)
    with pytest.raises(ValueError):
        o.rca_window(None, None, None, None, **kw)
    with pytest.raises(ValueError):
        o.online_anomaly_detect_RCA(None, None, None, **kw)
    with pytest.raises(ValueError):
        o.RCAStream(None, None, ctx=object(), device_append=False, **kw)
    with pytest.raises(ValueError):
        o.windows_timeline_q(None, [], [], q=q)
    with pytest.raises(ValueError):
        o.window_timeline_q(None, None, None, None, [], q=q)


@pytest.mark.parametrize("kw", [{"timeline_q": 0.5}, {"timeline_q": (0.5, 0.99), "latency": 0.5},
                                {"timeline": 8, "timeline_what": "total"}, {"timeline": 8, "timeline_what": 1},
                                {"timeline": 8, "timeline_q": 0.5, "timeline_what": None}, {"timeline_what": "p99"},
                                {"timeline": 0, "timeline_q": 0.5}, {"timeline": True, "timeline_what": "duration"}],
                         ids=lambda kw: ",".join(f"{k}={v!r}"[:22] for k, v in kw.items()))
def test_bad_combinations_raise_before_the_library_is_loaded(kw, no_library):
    """timeline_q without timeline (as exemplar_kinds without exemplars), a bad timeline_what, bad buckets beside
    the new keywords."""
    from microrank_amd import evidence
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        evidence.evidence_request(**kw)
    with pytest.raises(ValueError):
        o.sweep_rank({}, [], **kw)
    with pytest.raises(ValueError):
        o.rca_window(None, None, None, None, **kw)
    with pytest.raises(ValueError):
        o.online_anomaly_detect_RCA(None, None, None, **kw)
    with pytest.raises(ValueError):
        o.RCAStream(None, None, ctx=object(), device_append=False, **kw)


def test_bad_method_and_what_of_the_forms(no_library):
    from microrank_amd import online_rca as o

    for kw in ({"method": "nearest"}, {"method": 0}, {"what": "total"}, {"buckets": 0}, {"buckets": 513}):
        with pytest.raises(ValueError):
            o.windows_timeline_q(None, [], [], **kw)
        with pytest.raises(ValueError):
            o.window_timeline_q(None, None, None, None, [], **kw)
    assert o.windows_timeline_q(None, [], []) == []


def test_request_parameters(no_library):
    from microrank_amd import evidence

    tl = evidence.KINDS[3]
    assert tl.keyword == "timeline" and len(evidence.KINDS) == 5
    plain = evidence.evidence_request(timeline=8)
    assert [dict(p) for _, p in plain.kinds] == [{"buckets": 8}]          # without the keywords: what it was
    assert tl.batch_for(plain.kinds[0][1]) is evidence.windows_timeline
    assert tl.window_for(plain.kinds[0][1]) is evidence.window_timeline
    same = evidence.evidence_request(timeline=8, timeline_what="self")
    assert [dict(p) for _, p in same.kinds] == [{"buckets": 8}]
    r = evidence.evidence_request(timeline=np.int64(8), timeline_q=(0.5, 0.99))
    (kind, params), = r.kinds
    assert kind is tl and sorted(params) == ["buckets", "q"] and params["buckets"] == 8 and type(params["buckets"]) is int
    assert params["q"].dtype == np.float64 and params["q"].tolist() == [0.5, 0.99]
    assert tl.batch_for(params) is evidence.windows_timeline_q and tl.window_for(params) is evidence.window_timeline_q
    with pytest.raises(TypeError):
        params["q"] = None                                               # the request is read-only
    with pytest.raises(ValueError):
        params["q"][0] = 0.1                                             # ... and so is its vector
    one = evidence.evidence_request(timeline=8, timeline_q=0.9, timeline_what="duration")
    p = dict(one.kinds[0][1])
    assert p.pop("q").tolist() == [0.9] and p == {"buckets": 8, "what": "duration"}
    what = evidence.evidence_request(timeline=8, timeline_what="duration")
    assert [dict(p) for _, p in what.kinds] == [{"buckets": 8, "what": "duration"}]
    assert tl.batch_for(what.kinds[0][1]) is evidence.windows_timeline
    # latency's "q" does not send latency to other forms, and the kinds beside timeline are what they were
    both = evidence.evidence_request(latency=(0.5,), timeline=4, timeline_q=0.5, replicas=3)
    assert [k.key for k, _ in both.kinds] == ["latency", "timeline", "replicas"]
    lat = both.kinds[0]
    assert lat[0].batch_for(lat[1]) is evidence.windows_latency and lat[0].window_for(lat[1]) is evidence.op_latency
    assert evidence.evidence_request() is evidence.NOTHING


ROWS = {
    # key: start [B], cnt / sum / max [B][normal, abnormal], out [side][before, after]
    -1: {"start": [1000, 1500], "cnt": [[4, 1], [0, 2]], "sum": [[2_000_000, 700_000], [0, 9_000_000]],
         "max": [[900_000, 700_000], [0, 5_000_000]], "out": [[0, 0], [0, 0]]},
    "front": {"start": [1000, 1500], "cnt": [[7, 0], [2, 3]], "sum": [[-7000, 0], [3000, 9_000_000]],
              "max": [[-500, 0], [2000, 5_000_000]], "out": [[0, 0], [0, 0]]},
    "cart": {"start": [1000, 1500], "cnt": [[0, 1], [0, 0]], "sum": [[0, 123_456], [0, 0]],
             "max": [[0, 123_456], [0, 0]], "out": [[0, 0], [1, 0]]},
    "unranked": {"start": [1000, 1500], "cnt": [[1, 1], [1, 1]], "sum": [[1, 1], [1, 1]], "max": [[1, 1], [1, 1]],
                 "out": [[0, 0], [0, 0]]},
}
# quantile [B][normal, abnormal][q] for q = (0.5, 0.99), raw units
QUANT = {
    -1: [[[450_000.0, 899_000.5], [700_000.0, 700_000.0]], [[0.0, 0.0], [4_500_000.0, 4_990_000.0]]],
    "front": [[[-1000.0, -500.2], [0.0, 0.0]], [[1500.0, 1990.0], [3_000_000.0, 4_960_000.06]]],
    "cart": [[[0.0, 0.0], [123_456.0, 123_456.0]], [[0.0, 0.0], [0.0, 0.0]]],
    "unranked": [[[1.0, 1.0], [1.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]]],
}


def test_timeline_q_csv_writer(tmp_path, monkeypatch):
    from microrank_amd import online_rca as o

    (tmp_path / "plain").mkdir()
    (tmp_path / "q").mkdir()
    monkeypatch.chdir(tmp_path / "plain")
    o._write_timeline(["front", "gone", "cart"], [0.5, 0.7, 0.9], ROWS)
    assert os.listdir(".") == ["timeline.csv"]                           # rows without quantiles: today's one file
    plain = open("timeline.csv", "rb").read()
    monkeypatch.chdir(tmp_path / "q")
    rows = {k: dict(v, q=[0.5, 0.99], quantile=QUANT[k]) for k, v in ROWS.items()}
    # result.csv's order is by score: cart (0.9) before front (0.5); `gone` has no rows
    o._write_timeline(["front", "gone", "cart"], [0.5, 0.7, 0.9], rows)
    assert sorted(os.listdir(".")) == ["timeline.csv", "timeline_q.csv"]
    assert open("timeline.csv", "rb").read() == plain                    # timeline.csv exactly as without them
    got = list(csv.reader(open("timeline_q.csv")))
    assert got[0] == ["result", "rank", "bucket", "start", "side", "spans", "q", "value"]
    assert got[1:] == [
        ["*", "0", "0", "1000", "normal", "4", "0.5", "450.0"], ["*", "0", "0", "1000", "normal", "4", "0.99", "899.0005"],
        ["*", "0", "0", "1000", "abnormal", "1", "0.5", "700.0"], ["*", "0", "0", "1000", "abnormal", "1", "0.99", "700.0"],
        ["*", "0", "1", "1500", "normal", "0", "0.5", "0.0"], ["*", "0", "1", "1500", "normal", "0", "0.99", "0.0"],
        ["*", "0", "1", "1500", "abnormal", "2", "0.5", "4500.0"], ["*", "0", "1", "1500", "abnormal", "2", "0.99", "4990.0"],
        ["cart", "1", "0", "1000", "normal", "0", "0.5", "0.0"], ["cart", "1", "0", "1000", "normal", "0", "0.99", "0.0"],
        ["cart", "1", "0", "1000", "abnormal", "1", "0.5", "123.456"], ["cart", "1", "0", "1000", "abnormal", "1", "0.99", "123.456"],
        ["cart", "1", "1", "1500", "normal", "0", "0.5", "0.0"], ["cart", "1", "1", "1500", "normal", "0", "0.99", "0.0"],
        ["cart", "1", "1", "1500", "abnormal", "0", "0.5", "0.0"], ["cart", "1", "1", "1500", "abnormal", "0", "0.99", "0.0"],
        ["front", "3", "0", "1000", "normal", "7", "0.5", "-1.0"], ["front", "3", "0", "1000", "normal", "7", "0.99", "-0.5002"],
        ["front", "3", "0", "1000", "abnormal", "0", "0.5", "0.0"], ["front", "3", "0", "1000", "abnormal", "0", "0.99", "0.0"],
        ["front", "3", "1", "1500", "normal", "2", "0.5", "1.5"], ["front", "3", "1", "1500", "normal", "2", "0.99", "1.99"],
        ["front", "3", "1", "1500", "abnormal", "3", "0.5", "3000.0"], ["front", "3", "1", "1500", "abnormal", "3", "0.99", "4960.0001"],
    ]


def test_timeline_row_passes_the_quantile_keys_as_lists():
    from microrank_amd import evidence

    slot = {"start": np.array([5, 9], np.int64), "cnt": np.array([[1, 0], [2, 3]], np.int64), "q": np.array([0.5]),
            "quantile": np.array([[[7.0], [0.0]], [[1.5], [2.0]]])}
    row = evidence._timeline_row(None, slot)
    assert row == {"start": [5, 9], "cnt": [[1, 0], [2, 3]], "q": [0.5], "quantile": [[[7.0], [0.0]], [[1.5], [2.0]]]}
    assert type(row["quantile"][0][0][0]) is float and type(row["start"][0]) is int


def test_gitignore_and_documents():
    ignored = open(os.path.join(REPO, ".gitignore")).read().split()
    assert "/timeline_q.csv" in ignored
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "timeline_q" in readme and "mr_windows_timeline_q" in readme
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "mr_windows_timeline_q" in design and "k_tlq_select" in design
