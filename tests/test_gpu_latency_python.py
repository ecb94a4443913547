"""GPU checks of the Python surface of the latency evidence (online_rca.op_latency, rca_window's and
the driver's ``latency`` keyword) on the committed case `pods_dup_broken`, against pandas and numpy on
the DataFrame itself."""
import contextlib
import csv
import io
import os

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden, regen_window

pytestmark = pytest.mark.gpu

QS = [0.5, 0.99]


@pytest.fixture(scope="module")
def case():
    c = load_golden("pods_dup_broken.json")
    ndf, adf = regen_window(c)
    slo = {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in c["slo"].items()}
    return c, adf, slo


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _pandas_latency(df, ops, abnormal, normal, start, end, what):
    """{op: {...}} as op_latency gives it, from the DataFrame: self time through a merge on
    ParentSpanId == spanID (every row of the frame, traceID ignored), the sides from the detector's
    lists, the rows of the detector's inclusive window."""
    from microrank_amd.spans import op_display

    d = df.reset_index(drop=True)
    kids = d.loc[d["ParentSpanId"].notna(), ["ParentSpanId", "duration"]].groupby("ParentSpanId")["duration"].sum()
    m = d[["spanID"]].merge(kids.rename("csum"), how="left", left_on="spanID", right_index=True)
    value = d["duration"].to_numpy(np.int64) - m["csum"].fillna(0).to_numpy(np.int64) if what == "self" else \
        d["duration"].to_numpy(np.int64)
    op = op_display(d["serviceName"].to_numpy(dtype=object), d["operationName"].to_numpy(dtype=object))
    podop = np.array([f"{a}_{b}" for a, b in zip(d["podName"], op)], dtype=object)
    inside = ((d["startTime"] >= start) & (d["endTime"] <= end)).to_numpy()
    sides = {"normal": d["traceID"].isin(set(normal)).to_numpy(), "abnormal": d["traceID"].isin(set(abnormal)).to_numpy()}
    res = {}
    for name in ops:
        row = {}
        for side, msk in sides.items():
            a = value[inside & msk & (podop == name)]
            row["n_" + side] = int(a.size)
            row[side] = [float(x) for x in np.round(np.quantile(a, QS) / 1000.0, 4)] if a.size else [0.0] * len(QS)
        res[name] = row
    return res


def _same(got, exp):
    assert list(got) == list(exp)
    for name in exp:
        for side in ("normal", "abnormal"):
            assert got[name]["n_" + side] == exp[name]["n_" + side], (name, side)
            assert [float(v).hex() for v in got[name][side]] == [float(v).hex() for v in exp[name][side]], (name, side)
            assert all(isinstance(v, np.float64) for v in got[name][side])


def test_op_latency_and_rca_window(case):
    from microrank_amd.anormaly_detector import system_anomaly_detect
    from microrank_amd.online_rca import op_latency, rca_window

    c, adf, slo = case
    start, end = pd.Timestamp(c["detect"]["start_ns"]), pd.Timestamp(c["detect"]["end_ns"])
    flag, abnormal, normal = _quiet(system_anomaly_detect, adf, start_time=start, end_time=end, slo=slo,
                                    operation_list=c["operation_list"])
    assert flag is True and abnormal and normal
    plain = rca_window(adf, start, end, slo)
    top = plain["top"]
    assert top
    for what in ("self", "duration"):
        got = op_latency(adf, start, end, slo, top, q=QS, what=what)
        exp = _pandas_latency(adf, top, abnormal, normal, start, end, what)
        _same(got, exp)
        assert any(r["n_abnormal"] > 0 and r["n_normal"] > 0 for r in got.values())
    with_lat = rca_window(adf, start, end, slo, latency=QS)
    _same(with_lat.pop("latency"), op_latency(adf, start, end, slo, top, q=QS))
    assert with_lat == plain                      # every other key is what it was
    scalar = rca_window(adf, start, end, slo, latency=0.5, latency_what="duration")["latency"]
    full = op_latency(adf, start, end, slo, top, q=[0.5], what="duration")
    _same(scalar, full)
    with pytest.raises(ValueError):
        op_latency(adf, start, end, slo, ["no-such-pod_op"])


def _drive(df, slo, ops, **kw):
    from microrank_amd import online_rca

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        online_rca.online_anomaly_detect_RCA(df.copy(), slo, ops, **kw)
    return buf.getvalue()


@pytest.mark.parametrize("path", ["sweep", "window_loop"])
def test_driver_writes_latency_csv(case, path, tmp_path, monkeypatch):
    from microrank_amd import synth
    from microrank_amd.online_rca import op_latency

    c, adf, slo = case
    if path == "window_loop":   # times that vary within a trace: the driver goes window by window
        p = dict(c["params"])
        _, adf = synth.window_dataframes(p.pop("n_ops"), p.pop("n_traces"), p.pop("seed"), **dict(p, span_times=True))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    monkeypatch.chdir(tmp_path / "a")
    out_plain = _drive(adf, slo, c["operation_list"])
    assert os.path.exists("result.csv") and not os.path.exists("latency.csv")   # without the keyword: no file
    monkeypatch.chdir(tmp_path / "b")
    out_lat = _drive(adf, slo, c["operation_list"], latency=QS)
    assert out_lat == out_plain
    assert open("result.csv", "rb").read() == open(tmp_path / "a" / "result.csv", "rb").read()
    ranked = [r["result"] for r in csv.DictReader(open("result.csv"))]
    rows = list(csv.reader(open("latency.csv")))
    assert rows[0] == ["result", "rank", "side", "spans", "q", "value"]
    # the data holds one 5-minute window of traffic: the one trigger is the driver's first window
    start = adf["startTime"].min()
    exp = op_latency(adf, start, start + pd.Timedelta(minutes=5), slo, ranked, q=QS)
    want = []
    for rank, name in enumerate(ranked, start=1):
        for side in ("normal", "abnormal"):
            for qj, v in zip(QS, exp[name][side]):
                want.append([name, str(rank), side, str(exp[name]["n_" + side]), repr(float(qj)), repr(float(v))])
    assert rows[1:] == want
    assert any(int(r[3]) > 0 for r in rows[1:])
