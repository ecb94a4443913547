"""Every evidence keyword in ONE call against each keyword alone, on every driver path: the sweep path, the
stream, the window-by-window loop, rca_window and sweep_rank over several windows.  A kind must get its own
parameters, its own lead op and its own window's rows whatever else is asked.  All comparisons are exact:
two runs of one path give identical answers (tests/test_gpu_window_exemplar_kinds.py compares files so)."""
import contextlib
import io
import os

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden, regen_window

pytestmark = pytest.mark.gpu

SINGLES = [dict(exemplars=3, exemplar_kinds=True), dict(latency=(0.5, 0.99)), dict(kind_breakdown=4), dict(call_edges=4),
           dict(timeline=8), dict(replicas=4)]
ALL = {k: v for kw in SINGLES for k, v in kw.items()}
KEYS = ["exemplars", "latency", "kinds", "calls", "timeline", "replicas"]   # rca_window's keys; KEY.csv the files
FILES = [k + ".csv" for k in KEYS]


def _slo(case):
    return {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in case["slo"].items()}


@pytest.fixture(scope="module")
def golden():
    c = load_golden("pods_dup_broken.json")
    _, adf = regen_window(c)
    return c, adf, _slo(c)


def _in_dir(path, fn):
    """fn() with ``path`` (created) as the working directory: (its stdout, {file name: bytes} left there)."""
    cwd = os.getcwd()
    os.makedirs(path)
    os.chdir(path)
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            fn()
        return buf.getvalue(), {f: open(f, "rb").read() for f in sorted(os.listdir("."))}
    finally:
        os.chdir(cwd)


def _drive(path, golden, **kw):
    from microrank_amd import online_rca

    c, adf, slo = golden
    return _in_dir(path, lambda: online_rca.online_anomaly_detect_RCA(adf.copy(), slo, c["operation_list"], **kw))


def _check_all_against_singles(base, golden):
    """The driver with every keyword: the plain run's stdout and result.csv, exactly the six evidence files, each
    byte-equal to the file of the run with its keyword alone.  Returns the files."""
    out_plain, plain = _drive(base / "plain", golden)
    assert sorted(plain) == ["result.csv"] and "normal_list" in out_plain
    out_all, files = _drive(base / "all", golden, **ALL)
    assert out_all == out_plain
    assert sorted(files) == sorted(FILES + ["result.csv"]) and files["result.csv"] == plain["result.csv"]
    for i, (kw, name) in enumerate(zip(SINGLES, FILES)):
        out_one, one = _drive(base / f"single{i}", golden, **kw)
        assert out_one == out_plain and sorted(one) == sorted([name, "result.csv"]), kw
        assert one[name] == files[name], name
        assert len(one[name].splitlines()) > 1, name     # (a header alone would compare equal too)
    return files


@pytest.fixture(scope="module")
def sweep_files(golden, tmp_path_factory):
    return _check_all_against_singles(tmp_path_factory.mktemp("sweep"), golden)


def test_sweep_path_all_at_once_equals_each_alone(sweep_files):
    assert sorted(sweep_files) == sorted(FILES + ["result.csv"])


def test_stream_writes_the_drivers_files(golden, sweep_files, tmp_path):
    from microrank_amd.online_rca import RCAStream

    c, adf, slo = golden

    def run():
        s = RCAStream(slo, c["operation_list"], **ALL)
        s.push(adf.copy())
        s.close()

    _, files = _in_dir(tmp_path / "stream", run)
    assert files == sweep_files


def test_window_loop_all_at_once_equals_each_alone(golden, tmp_path, monkeypatch):
    from microrank_amd import online_rca

    monkeypatch.setattr(online_rca, "_sweep_plan", lambda *a, **k: None)   # window by window: the one-window forms
    _check_all_against_singles(tmp_path, golden)


def test_rca_window_all_at_once_equals_each_alone(golden):
    from microrank_amd.online_rca import rca_window

    c, adf, slo = golden
    start, end = pd.Timestamp(c["detect"]["start_ns"]), pd.Timestamp(c["detect"]["end_ns"])
    plain = rca_window(adf, start, end, slo)
    assert plain["top"]
    both = rca_window(adf, start, end, slo, **ALL)
    assert list(both) == list(plain) + KEYS
    assert {k: v for k, v in both.items() if k not in KEYS} == plain
    for kw, key in zip(SINGLES, KEYS):
        one = rca_window(adf, start, end, slo, **kw)
        assert list(one) == list(plain) + [key], kw
        np.testing.assert_equal(both[key], one[key])
        assert one[key], key


def test_sweep_rank_gives_each_kind_its_own_windows_rows():
    """Four triggered windows in one batch: every kind's plan entry of every window, asked with the others, is
    what the kind alone leaves there -- no kind is handed another window's rows or another kind's lead op."""
    from microrank_amd import online_rca, synth

    case = load_golden("stream.json")
    _, adf = synth.stream_dataframes(**case["params"])
    plan = online_rca._sweep_plan(adf, _slo(case), adf["startTime"].min(), adf["endTime"].max(), pd.Timedelta(minutes=5),
                                  pd.Timedelta(minutes=4), None)
    events = online_rca.sweep_chain(plan)
    todo = [e[1] for e in events if e[0] == "window" and e[4]]
    assert len(todo) == 4
    together = dict(plan)
    ranked = online_rca.sweep_rank(together, events, **ALL)
    assert list(ranked) == todo and sorted(set(together) - set(plan)) == sorted(KEYS[1:])
    for kw, key in zip(SINGLES, KEYS):
        alone = dict(plan)
        got = online_rca.sweep_rank(alone, events, **kw)
        assert sorted(set(alone) - set(plan)) == ([] if key == "exemplars" else [key]), kw
        for m in todo:
            np.testing.assert_equal(got[m], ranked[m] if key == "exemplars" else ranked[m][:6])
            if key == "exemplars":
                assert len(got[m]) == 7 and got[m][6]
                continue
            a, b = alone[key], together[key]
            if key == "latency":      # (q, {m: ...})
                np.testing.assert_equal(a[0], b[0])
                a, b = a[1], b[1]
            assert list(a) == list(b) == todo
            np.testing.assert_equal(a[m], b[m])
            assert list(a[m])[0] == {"kinds": None, "timeline": -1}.get(key, int(ranked[m][0][0])), (key, m)
    # (the windows differ, so a mix-up would show: each has its own traces per bucket)
    assert len({together["timeline"][m][-1]["cnt"].tobytes() for m in todo}) == len(todo)
