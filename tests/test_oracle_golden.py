"""Pin the oracle (oracle/oracle.py) to the reference's own outputs (tests/golden/*.json).

The fixtures were produced by importing /root/reference in the dev container
(tests/golden/make_golden.py).  Tolerances: graph structure, counts, key orders and
top lists exact; trace_pagerank weights 1e-12 relative (the reference's dense
OpenBLAS dgemv sums in an order no sparse code reproduces bit for bit); spectrum,
SLO and detector bit-exact (same IEEE operation sequence).
"""
import math

import numpy as np
import pandas as pd
import pytest

import oracle as orc
from conftest import load_golden, regen_window, unhex
from microrank_amd.spans import SpanTable

SPAN_CASES = ["c1", "pods_dup_broken", "ops200", "span_times"]


def check_pr(got, exp, rtol=1e-12):
    w, num = got
    assert list(w.keys()) == exp["keys"]
    assert list(num.keys()) == exp["num_keys"]
    assert [int(v) for v in num.values()] == exp["num"]
    gw = np.array([float(v) for v in w.values()])
    ew = unhex(exp["weight"])
    np.testing.assert_allclose(gw, ew, rtol=rtol, atol=0)


@pytest.mark.parametrize("case", ["fig3", "multiset_selfloop", "pr_subset", "single", "asym_incidence"])
@pytest.mark.parametrize("anomaly", [False, True])
def test_dict_cases(case, anomaly):
    d = load_golden("dict_cases.json")[case]
    inp = d["input"]
    exp = d[f"anomaly={anomaly}"]
    args = (inp["operation_operation"], inp["operation_trace"], inp["trace_operation"], inp["pr_trace"])
    if "error" in exp:
        with pytest.raises(getattr(__builtins__, exp["error"], Exception) if isinstance(__builtins__, dict)
                           else Exception):
            orc.trace_pagerank(*args, anomaly)
        return
    check_pr(orc.trace_pagerank(*args, anomaly), exp)


@pytest.mark.parametrize("anomaly", [False, True])
def test_dict_general(anomaly):
    """The general dict form at 300 ops / 1500 traces (gpu_util.general_graph: P_rs != P_sr, a
    pr_trace subset with its own lengths, traces without ops, list multiplicities) against the
    reference's own output on the recorded dicts.  1e-10: the reference's dense dgemv sums 1500
    terms in another order (measured 5e-15); keys, counts and zeros exact."""
    from gpu_util import general_golden_dicts

    fix = load_golden("dict_general.json")
    exp = fix[f"anomaly={anomaly}"]
    got = orc.trace_pagerank(*general_golden_dicts(fix), anomaly)
    check_pr(got, exp, rtol=1e-10)
    gw, ew = np.array([float(v) for v in got[0].values()]), unhex(exp["weight"])
    np.testing.assert_array_equal(gw == 0, ew == 0)


def test_dict_general_fixture_is_a_general_graph():
    """The recorded dicts (stored, not re-derived from the seed) have the properties the fixture is
    there for, and graph_dicts inverts graph_from_dicts on them."""
    from gpu_util import general_golden_dicts, graph_dicts

    dicts = general_golden_dicts(load_golden("dict_general.json"))
    g = orc.graph_from_dicts(*dicts)
    assert (g.N, g.T) == (300, 1500)
    assert not (np.array_equal(g.rs_t, g.sr_t) and np.array_equal(g.rs_o, g.sr_o))
    assert g.pr_idx.size < g.T and (np.diff(g.pr_idx) < 0).any()
    assert (g.len_t == 0).any() and (g.len_t > np.bincount(g.sr_t, minlength=g.T)).any()
    assert (g.len_o > np.bincount(g.rs_o, minlength=g.N)).any() and (g.nchild > np.bincount(g.ss_p, minlength=g.N)).any()
    again = graph_dicts(g)
    assert all(a == b and list(a) == list(b) for a, b in zip(again, dicts))


def test_host_graph_from_dicts_equals_oracle_conversion():
    """The product's dict -> index conversion (graph.host_graph_from_dicts) against the oracle's
    (graph_from_dicts -> host_graph_from_oracle), field for field, on the general dicts (explicit
    rs_* and pr_*) and on their rs == sr / pr_trace-is-operation_trace form (both None)."""
    from gpu_util import general_golden_dicts, general_graph, graph_dicts, host_graph_from_oracle
    from microrank_amd.graph import host_graph_from_dicts

    general = general_golden_dicts(load_golden("dict_general.json"))
    plain = graph_dicts(general_graph(300, 200, seed=5, rs_drop=0, rs_add=0, pr_frac=None, empty_frac=0))
    for dicts, explicit in ((general, True), (plain, False)):
        got = host_graph_from_dicts(*dicts)
        exp = host_graph_from_oracle(orc.graph_from_dicts(*dicts))
        assert got.nodes == exp.nodes and got.traces == exp.traces
        for f in ("sr_off", "sr_ops", "rs_off", "rs_ops", "len_t", "len_o", "ss_off", "ss_par", "nchild", "pr_trace",
                  "pr_len"):
            a, b = getattr(got, f), getattr(exp, f)
            if f.startswith(("rs_", "pr_")):
                assert (a is not None) == (b is not None) == explicit, f
            if b is not None:
                assert a.dtype == b.dtype, f
                np.testing.assert_array_equal(a, b, err_msg=f)


def test_paper_example_survey_values():
    # anomaly weights of the Fig. 3 dicts through the reference
    d = load_golden("dict_cases.json")["fig3"]
    w = unhex(d["anomaly=True"]["weight"])
    np.testing.assert_allclose(w, [0.65681832483573, 0.21988528611506, 0.21988528611506, 0.66330495471105],
                               rtol=1e-12)


def _spans(df):
    return SpanTable.from_dataframe(df)


@pytest.mark.parametrize("name", SPAN_CASES)
def test_span_graph_matches_reference(name):
    case = load_golden(f"{name}.json")
    _, adf = regen_window(case)
    st = _spans(adf)
    tnames = list(st.trace_names)
    ti = {n: i for i, n in enumerate(tnames)}
    for key, lst in (("graph_swapped_normal", case["detect"]["abnormal"]),
                     ("graph_swapped_anomaly", case["detect"]["normal"])):
        exp = case[key]
        sel = np.zeros(len(tnames), dtype=bool)
        sel[lst] = True
        sg = orc.span_graph(st.trace, st.podop, st.span, st.parent, sel)
        nodes = [st.podop_names[c] for c in sg.node_podop]
        assert nodes == exp["nodes"]
        # children multisets
        oo = exp["operation_operation"]
        N = len(nodes)
        exp_nchild = np.zeros(N, dtype=np.int64)
        exp_pairs = set()
        pos = 0
        for k, ln in zip(oo["keys"], oo["len"]):
            exp_nchild[k] = ln
            for c in oo["vals"][pos:pos + ln]:
                exp_pairs.add((c, k))
            pos += ln
        assert oo["keys"] == list(range(N))
        np.testing.assert_array_equal(sg.nchild, exp_nchild)
        assert set(zip(sg.ss_c.tolist(), sg.ss_p.tolist())) == exp_pairs
        # operation_trace: sorted trace keys, list lengths, distinct op sets
        ot = exp["operation_trace"]
        assert list(sg.trace_codes) == ot["keys"]
        np.testing.assert_array_equal(sg.len_t, ot["len"])
        exp_sr = set()
        pos = 0
        for t_i, (k, ln) in enumerate(zip(ot["keys"], ot["len"])):
            for o in ot["vals"][pos:pos + ln]:
                exp_sr.add((t_i, o))
            pos += ln
        assert set(zip(sg.sr_t.tolist(), sg.sr_o.tolist())) == exp_sr
        to = exp["trace_operation"]
        len_o = dict(zip(to["keys"], to["len"]))
        assert [len_o[i] for i in range(N)] == sg.len_o.tolist()
        assert exp["pr_trace_is_operation_trace"]


@pytest.mark.parametrize("name", SPAN_CASES)
def test_span_pagerank_matches_reference(name):
    case = load_golden(f"{name}.json")
    _, adf = regen_window(case)
    st = _spans(adf)
    for lst_key, anomaly, exp_key in (("abnormal", False, "pr_normal"), ("normal", True, "pr_anomaly"),
                                      ("abnormal", True, "pr_abn_true"), ("normal", False, "pr_nor_false")):
        sel = np.zeros(st.n_traces, dtype=bool)
        sel[case["detect"][lst_key]] = True
        sg = orc.span_graph(st.trace, st.podop, st.span, st.parent, sel)
        g = sg.as_graph()
        g.nodes = [st.podop_names[c] for c in sg.node_podop]
        kind = orc.trace_kinds(g)
        v = orc.preference(g, kind, anomaly)
        s = orc.power_iteration(g, v)
        check_pr(orc.weights(g, s), case[exp_key])


@pytest.mark.parametrize("name", SPAN_CASES)
def test_spectrum_matches_reference(name):
    case = load_golden(f"{name}.json")
    a = case["pr_anomaly"]
    n = case["pr_normal"]
    a_w = dict(zip(a["keys"], unhex(a["weight"])))
    n_w = dict(zip(n["keys"], unhex(n["weight"])))
    a_n = dict(zip(a["num_keys"], a["num"]))
    n_n = dict(zip(n["num_keys"], n["num"]))
    A = len(case["detect"]["normal"])     # T1: the driver's anomaly list is the detector's normal list
    Nn = len(case["detect"]["abnormal"])
    for m, exp in case["spectrum"].items():
        top, score, lines = orc.spectrum(a_w, n_w, A, Nn, 5, n_n, a_n, m)
        assert top == exp["top"]
        assert [float(x).hex() for x in score] == exp["score"]
        assert "".join(l + "\n" for l in lines) == exp["stdout"]


def test_spectrum_edge_cases():
    d = load_golden("dict_cases.json")["spectrum_edges"]
    i = d["input"]
    for m, exp in d["out"].items():
        if "error" in exp:
            with pytest.raises(ZeroDivisionError):
                orc.spectrum(i["a_w"], i["n_w"], i["A"], i["N"], 5, i["n_n"], i["a_n"], m)
            continue
        top, score, lines = orc.spectrum(i["a_w"], i["n_w"], i["A"], i["N"], 5, i["n_n"], i["a_n"], m)
        assert top == exp["top"]
        assert [float(x).hex() for x in score] == exp["score"]


def test_spectrum_synth_matches_reference():
    """oracle.spectrum against the reference's own results on the generated spectrum inputs
    (tests/spectrum_cases.py: tie groups of hundreds, -0.0 and inf scores, Python / numpy typed
    weights, a zero division raised by the union's last node), bit for bit: names, score hex and
    score types of the top 11 of every method, ZeroDivisionError where the reference raised.  The
    fixture holds results only; the inputs are rebuilt from its seed.  From here the oracle is the
    reference of the GPU spectrum tests at every other size."""
    import spectrum_cases as sc

    fix = load_golden("spectrum_synth.json")
    assert fix["seed"] == sc.SEED and tuple(fix["no_neg_zero"]) == sc.NO_NEG_ZERO
    assert sorted({c["n"] for c in fix["cases"]}) == [1, 2, 3, 65, 1025, 4097]
    assert len(fix["cases"]) == 18
    for c in fix["cases"]:
        assert set(c["out"]) == set(sc.METHODS)
        for m, exp in c["out"].items():
            case = sc.case_for(m, c["n"], fix["seed"], c["typed"])
            if "error" in exp:
                assert exp["error"] == "ZeroDivisionError"
                with pytest.raises(ZeroDivisionError):
                    sc.run_oracle(case, m, 5)
                continue
            top, score, _ = sc.run_oracle(case, m, 5)
            where = (c["n"], c["typed"], m)
            assert top == exp["top"], where
            assert [float(s).hex() for s in score] == exp["score"], where
            assert ["np.float64" if isinstance(s, np.float64) else type(s).__name__ for s in score] == exp["type"], where


def test_spectrum_cases_have_their_edges():
    """The generator's own promises (spectrum_cases.expected's assertions: the three node kinds in
    an order of their own, no NaN for any method, inf and -0.0 scores, the typed variants) at the
    smallest sizes and around the one-block sort's limit; tie groups of hundreds and a -0.0 inside
    the +0.0 scores at 4096 and 4097."""
    import spectrum_cases as sc

    for n in (1, 2, 3, 5, 64, 65, 4097):
        for typed in ("np", "mixed", "zd_last"):
            sc.expected(n, typed)
    kinds = set()
    for n in (1, 2, 3):
        a, nr = sc.spectrum_case(n)[:2]
        kinds |= {(k in a, k in nr) for k in sc.union(sc.spectrum_case(n))}
    assert kinds == {(True, False), (True, True), (False, True)}
    for n in (4096, 4097):   # either side of the switch between the two sorts
        e = sc.expected(n, "np")
        assert sc.largest_tie_group(e["dstar2"][1]) >= 200
        z = [bool(np.signbit(float(s))) for s in e["jaccard"][1] if float(s) == 0.0]
        assert 0 < z.index(True) < len(z) - 1   # the -0.0 ties with the +0.0 scores: between them, by position


@pytest.mark.parametrize("name", SPAN_CASES)
def test_slo_and_detector_match_reference(name):
    case = load_golden(f"{name}.json")
    ndf, adf = regen_window(case)
    nst = _spans(ndf)
    slo = orc.operation_slo(nst.svcop, nst.duration, nst.svcop_names, case["operation_list"])
    assert list(slo.keys()) == list(case["slo"].keys())
    for k, v in slo.items():
        assert [float(v[0]).hex(), float(v[1]).hex()] == case["slo"][k]
    ast = _spans(adf)
    a3 = {}
    for code, name_ in enumerate(ast.svcop_names):
        if name_ in slo:
            a3[code] = slo[name_][0] + 3 * slo[name_][1]
    flag, ab, no = orc.detect(ast.trace, ast.svcop, ast.duration, ast.tstart, ast.tend,
                              case["detect"]["start_ns"], case["detect"]["end_ns"], a3)
    assert ab == case["detect"]["abnormal"]
    assert no == case["detect"]["normal"]
    assert flag == case["detect"]["flag"]


def test_edge_spans():
    e = load_golden("edges.json")
    df = pd.read_parquet(f"{__import__('conftest').GOLDEN}/edges_spans.parquet")
    st = _spans(df)
    slo_list = e["operation_list"][:-1]
    slo = orc.operation_slo(st.svcop, st.duration, st.svcop_names, slo_list)
    assert {k: [float(v[0]).hex(), float(v[1]).hex()] for k, v in slo.items()} == e["slo"]
    a3 = {c: slo[n][0] + 3 * slo[n][1] for c, n in enumerate(st.svcop_names) if n in slo}
    t0 = int(df.startTime.min().value)
    flag, ab, no = orc.detect(st.trace, st.svcop, st.duration, st.tstart, st.tend, t0,
                              t0 + 5 * 60 * 10**9, a3)
    assert [st.trace_names[t] for t in ab] == e["detect"]["abnormal"]
    assert [st.trace_names[t] for t in no] == e["detect"]["normal"]
    all_tr = sorted(df.traceID.unique())
    for key, lst in (("all", all_tr), ("subset", all_tr[::2] + ["not-a-trace"])):
        sel = np.isin(np.array(st.trace_names, dtype=object), lst)
        sg = orc.span_graph(st.trace, st.podop, st.span, st.parent, sel)
        exp = e[f"graph_{key}"]
        nodes = [st.podop_names[c] for c in sg.node_podop]
        assert nodes == list(exp["operation_operation"].keys())
        for p, ch in exp["operation_operation"].items():
            pi = nodes.index(p)
            assert sg.nchild[pi] == len(ch)
            assert {(nodes.index(c), pi) for c in ch} == {(c, p_) for c, p_ in zip(sg.ss_c, sg.ss_p) if p_ == pi}
        for flag_ in (False, True):
            g = sg.as_graph()
            g.nodes = nodes
            w = orc.weights(g, orc.power_iteration(g, orc.preference(g, orc.trace_kinds(g), flag_)))
            check_pr(w, e[f"pr_{key}_{flag_}"])


def test_slo_large_ops_numpy_buffering():
    """Ops larger than numpy's 8192-element reduction buffer: np.std sums the buffers
    sequentially (oracle.numpy_reduce_sum); plain pairwise summation over the whole op differs
    in the last bits for some of them."""
    from microrank_amd import synth

    case = load_golden("slo_large.json")
    df = synth.slo_frame(case["seed"], tuple(case["sizes"]))
    assert synth.frame_digest(df) == case["digest"]
    st = _spans(df)
    slo = orc.operation_slo(st.svcop, st.duration, st.svcop_names, case["operation_list"])
    assert {k: [float(v[0]).hex(), float(v[1]).hex()] for k, v in slo.items()} == case["slo"]
    assert list(slo) == sorted(case["slo"])


@pytest.mark.parametrize("name", ["stream", "stream_gap"])
def test_driver_sweep_matches_reference(name):
    """The oracle's window chain (online_rca.py:161-216) reproduces every detector line of the
    reference driver over a multi-window stream, and where it ends (T2)."""
    from microrank_amd import synth

    case = load_golden(f"{name}.json")
    ndf, adf = synth.stream_dataframes(**case["params"])
    assert synth.frame_digest(ndf) == case["input_digest"]["normal"], "generator drifted (normal)"
    assert synth.frame_digest(adf) == case["input_digest"]["abnormal"], "generator drifted (abnormal)"
    ast = _spans(adf)
    slo = {k: (float.fromhex(a), float.fromhex(b)) for k, (a, b) in case["slo"].items()}
    a3 = {c: slo[n][0] + 3 * slo[n][1] for c, n in enumerate(ast.svcop_names) if n in slo}
    events, empty = orc.driver_sweep(ast.trace, ast.svcop, ast.duration, ast.tstart, ast.tend, a3)
    lines = []
    for _t, flag, ab, no, _ranked in events:
        lines += [f"anormaly_trace {len(ab)}", f"total_trace {len(ab) + len(no)}"]
        if flag:
            lines += [f"anomaly_list {len(no)}", f"normal_list {len(ab)}"]
    if empty:
        lines.append("Error: Current span list is empty")
    exp = [ln.rstrip() for ln in case["driver_stdout"].splitlines()
           if ln.startswith(("anormaly_trace", "total_trace", "anomaly_list", "normal_list", "Error"))]
    assert lines == exp
    assert empty == (case["driver_error"] == "TypeError")


def test_read_traces_csv_equals_pandas(tmp_path):
    """f2: the OTel export (collect_data.py:35-46) read through pyarrow (Arrow-backed strings) holds
    what pandas' read_csv + rename + to_datetime (online_rca.py:221-248) holds, and factorises
    to the same codes."""
    import pandas as pd

    from microrank_amd import synth
    from microrank_amd.spans import OTEL_RENAME, SpanTable, read_traces_csv

    case = load_golden("pods_dup_broken.json")
    _, adf = regen_window(case)
    inv = {v: k for k, v in OTEL_RENAME.items()}
    p = tmp_path / "traces.csv"
    adf.rename(columns=inv).to_csv(p, index=False)
    ref = pd.read_csv(p).rename(columns=OTEL_RENAME)
    ref["startTime"] = pd.to_datetime(ref["startTime"])
    ref["endTime"] = pd.to_datetime(ref["endTime"])
    got = read_traces_csv(p)
    assert list(got.columns) == list(ref.columns)
    for c in ref.columns:
        a, b = got[c].to_numpy(dtype=object), ref[c].to_numpy(dtype=object)
        same = [(pd.isna(x) and pd.isna(y)) if (pd.isna(x) or pd.isna(y)) else x == y for x, y in zip(a, b)]
        assert all(same), c
    h1, h2 = SpanTable.from_dataframe(ref), SpanTable.from_dataframe(got)
    for c in ("trace", "podop", "svcop", "span", "parent", "duration", "tstart", "tend"):
        assert np.array_equal(getattr(h1, c), getattr(h2, c)), c
    assert synth.frame_digest(adf) == case["input_digest"]["abnormal"]
