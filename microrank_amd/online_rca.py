"""Drop-in for the reference module ``online_rca`` (online_rca.py).

* ``calculate_spectrum_without_delay_list`` -- the weighted spectrum scores and the stable
  top list (online_rca.py:33-152), computed on the GPU (K3, csrc/mr_spectrum.hip); printing,
  argument names and return types as in the reference.
* ``online_anomaly_detect_RCA`` -- the sliding-window driver (online_rca.py:155-216), line for
  line the same control flow, with every ranking step on the GPU.
* ``rca_window`` -- one whole window (detect -> 2 graphs -> 2 PageRanks -> spectrum) in a
  single C-ABI call with every intermediate resident in HBM (used by bench.py).

The evidence kinds beside a ranking (latency, trace kinds, call edges, timeline, replicas) live in
``evidence.py``; the drivers here check their keywords into one request (``evidence_request``) and loop
over its kinds.  The kinds' entries and writers are re-exported under their names here.
"""
from __future__ import annotations

import csv
import ctypes as C
import math
import time

import numpy as np
import pandas as pd

from . import _lib
from . import evidence as ev   # (the drivers read ev.KINDS when they are called)
from ._lib import SPECTRUM_METHODS, ptr
from .anormaly_detector import slo_arrays, system_anomaly_detect, trace_list_partition  # noqa: F401
from .evidence import (NOTHING, _detect_state, _latency_ms, _ranked, _write_calls, _write_endpoints,  # noqa: F401
                       _write_kinds, _write_latency, _write_replicas, _write_timeline, evidence_request, op_latency,
                       window_calls, window_endpoints, window_kinds, window_replicas, window_timeline, window_timeline_q,
                       windows_call_edges, windows_endpoints, windows_kind_breakdown, windows_latency, windows_replicas,
                       windows_timeline, windows_timeline_q)
from .graph import check_converge_args, check_exemplar_kinds, check_exemplar_m, check_exemplar_ops
from .pagerank import ITERATIONS, trace_pagerank
from .preprocess_data import (PagerankGraph, SpanStream, _quantile_args, get_operation_duration_data, get_operation_slo,  # noqa: F401
                              get_pagerank_graph, get_service_operation_list, get_span, span_table)
from .spans import to_ns


def timestamp(datetime):
    """online_rca.py:26-30."""
    return int(time.mktime(time.strptime(str(datetime), "%Y-%m-%d %H:%M:%S"))) * 1000


def _is_np(v) -> bool:
    return isinstance(v, np.generic)


def calculate_spectrum_without_delay_list(anomaly_result, normal_result, anomaly_list_len, normal_list_len, top_max,
                                          normal_num_list, anomaly_num_list, spectrum_method, *, ctx=None):
    """online_rca.calculate_spectrum_without_delay_list on MI355X."""
    nodes = list(anomaly_result)
    nodes += [k for k in normal_result if k not in anomaly_result]
    n = len(nodes)
    has_a = np.zeros(n, np.uint8)
    has_n = np.zeros(n, np.uint8)
    a_w = np.zeros(n, np.float64)
    n_w = np.zeros(n, np.float64)
    a_num = np.zeros(n, np.int64)
    n_num = np.zeros(n, np.int64)
    kinds = []   # (a numpy-typed, n numpy-typed) per node, for the result type
    for i, node in enumerate(nodes):
        ta = tn = False
        if node in anomaly_result:
            w = anomaly_result[node]
            a_w[i] = w
            a_num[i] = anomaly_num_list[node]          # KeyError as in the reference (:49)
            ta = _is_np(w)
            has_a[i] = 1 | (2 if ta else 0)
        if node in normal_result:
            w = normal_result[node]
            n_w[i] = w
            n_num[i] = normal_num_list[node]
            tn = _is_np(w)
            has_n[i] = 1 | (2 if tn else 0)
        kinds.append((ta, tn))
    try:
        method = SPECTRUM_METHODS.index(spectrum_method)
    except ValueError:
        return [], []                                  # no branch matched: empty result (:77-142)
    if n == 0:
        return [], []
    ctx = ctx or _lib.default_context()
    k = max(0, min(n, top_max + 6))
    idx = np.zeros(max(k, 1), np.int32)
    sc = np.zeros(max(k, 1), np.float64)
    n_out, zd = C.c_int32(), C.c_int32()
    ctx.check(_lib.load().mr_spectrum(ctx.h, n, ptr(has_a, C.c_uint8), ptr(a_w, C.c_double), ptr(a_num, C.c_int64),
                                      ptr(has_n, C.c_uint8), ptr(n_w, C.c_double), ptr(n_num, C.c_int64),
                                      int(anomaly_list_len), int(normal_list_len), method, k, ptr(idx, C.c_int32),
                                      ptr(sc, C.c_double), C.byref(n_out), C.byref(zd)), "mr_spectrum")
    if zd.value:
        raise ZeroDivisionError("float division by zero")
    top_list, score_list = [], []
    for j in range(n_out.value):
        i = int(idx[j])
        ta, tn = kinds[i]
        ha, hn = bool(has_a[i] & 1), bool(has_n[i] & 1)
        if spectrum_method == "ochiai":          # ef / math.sqrt(...): the type of ef decides
            res_np = ta if ha else False
        else:
            res_np = (ta or (tn and hn)) if ha else tn
        s = np.float64(sc[j]) if res_np else float(sc[j])
        top_list.append(nodes[i])
        score_list.append(s)
        print("%-50s: %.8f" % (nodes[i], s))
    return top_list, score_list


def _write_result(top_list, score_list):
    with open("result.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["level", "result", "rank", "confidence"])
        for rank, (service, score) in enumerate(_ranked(top_list, score_list), start=1):
            w.writerow(["span", service, rank, float(score)])


def _write_exemplars(top_list, score_list, rows, kinds=False):
    """exemplars.csv beside result.csv: for each op of result.csv, in its order, the traces to open
    (rows: {op: [(trace, score), ...]}, best first).  kinds: the rows hold (trace, score, count), one
    trace per trace kind, and the file a 5th column ``traces``: the traces of that kind in the window."""
    with open("exemplars.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "trace", "score"] + (["traces"] if kinds else []))
        for service, _ in _ranked(top_list, score_list):
            for rank, row in enumerate(rows.get(service, []), start=1):
                w.writerow([service, rank, row[0], float(row[1])] + ([int(row[2])] if kinds else []))


def sweep_plan(ctx, table, dev, a3, ok, t_begin: int, t_end: int, step_normal: int, step_abnormal: int):
    """SURVEY 8(f) f3 on a resident span table: the detector counts of every window start the
    driver's chain can reach (online_rca.py:161-216: starts t_begin + m * grain while < t_end,
    grain = gcd of the two steps) from ONE device pass (mr_detect_sweep).  None when the table's
    window times vary within a trace (the per-window loop applies then)."""
    grain = math.gcd(step_normal, step_normal + step_abnormal)
    n_win = -(-(t_end - t_begin) // grain)
    if n_win <= 0 or n_win > 1 << 24:
        return None
    na, nn, rows = np.zeros(n_win, np.int32), np.zeros(n_win, np.int32), np.zeros(n_win, np.int64)
    rc = _lib.load().mr_detect_sweep(ctx.h, dev.h, t_begin, grain, step_normal, n_win, ptr(a3, C.c_double),
                                     ptr(ok, C.c_uint8), None, ptr(na, C.c_int32), ptr(nn, C.c_int32),
                                     ptr(rows, C.c_int64))
    if rc == _lib.MR_ERR_STATE:
        return None
    ctx.check(rc, "mr_detect_sweep")
    return dict(ctx=ctx, table=table, dev=dev, a3=a3, ok=ok, t_begin=t_begin, grain=grain,
                step_n=step_normal // grain, step_a=step_abnormal // grain, n_win=n_win, na=na, nn=nn, rows=rows)


def sweep_chain(plan):
    """Walk the driver's window chain over the sweep's counts -- only the counts decide the next
    start: ("window", m, n_abnormal, n_normal, ranked) per visited window, ("empty", m) where the
    reference's detector returns False (T2) and the chain stops."""
    events, m = [], 0
    while m < plan["n_win"]:
        if plan["rows"][m] == 0:
            events.append(("empty", m))
            break
        na, nn = int(plan["na"][m]), int(plan["nn"][m])
        ranked = na > 0 and nn > 0
        events.append(("window", m, na, nn, ranked))
        m += plan["step_n"] + (plan["step_a"] if ranked else 0)
    plan["next_m"] = m   # where the chain goes on (RCAStream)
    return events


def sweep_rank(plan, events, precision="fp64", iters=ITERATIONS, exemplars=None, exemplar_kinds=False, *, latency=None,
               latency_what="self", kind_breakdown=None, call_edges=None, timeline=None, replicas=None, timeline_q=None,
               timeline_what="self", kind_by="kind"):
    """Every ranked window of the chain in ONE mr_windows_batch_ex call: {m: (codes, scores, ...)}.
    exemplars, exemplar_kinds: rank_windows' keywords (a 7th element per window).
    The evidence keywords are online_anomaly_detect_RCA's: each asked kind makes ONE batch call over the
    triggered windows' top lists and leaves its answer in the plan for the replay (no key without the keyword):
    latency: plan["latency"] = (q, {m: windows_latency's dict});
    kind_breakdown: plan["kinds"] = {m: windows_kind_breakdown's dict}, the whole window (None) first;
    call_edges: plan["calls"] = {m: windows_call_edges' dict};
    timeline: plan["timeline"] = {m: windows_timeline's dict}, the window's own traces (-1) first -- with
    timeline_q its slots carry "q" and "quantile" too, and timeline_what chooses their value;
    kind_by="endpoint" (with kind_breakdown): plan["endpoints"] = {m: windows_endpoints' dict}, the whole window
    (None) first, in place of plan["kinds"];
    replicas: plan["replicas"] = {m: windows_replicas' dict}."""
    return _sweep_rank(plan, events, precision, iters,
                       evidence_request(exemplars=exemplars, exemplar_kinds=exemplar_kinds, latency=latency,
                                        latency_what=latency_what, kind_breakdown=kind_breakdown, call_edges=call_edges,
                                        timeline=timeline, replicas=replicas, timeline_q=timeline_q,
                                        timeline_what=timeline_what, kind_by=kind_by))


def _sweep_rank(plan, events, precision, iters, evidence):
    """sweep_rank for a checked request."""
    for kind in ev.KINDS:
        for key in kind.keys:
            plan.pop(key, None)
    todo = [e[1] for e in events if e[0] == "window" and e[4]]
    width = plan["step_n"] * plan["grain"]
    if not todo:
        return {}
    wins = [(plan["dev"], plan["t_begin"] + mm * plan["grain"], plan["t_begin"] + mm * plan["grain"] + width,
             plan["a3"], plan["ok"]) for mm in todo]
    ranked = rank_windows(plan["ctx"], wins, precision=precision, iters=iters, exemplars=evidence.exemplars,
                          exemplar_kinds=evidence.exemplar_kinds)
    for kind, params in evidence.kinds:
        answer = kind.batch_for(params)(plan["ctx"], wins, [list(kind.lead) + r[0].tolist() for r in ranked],
                                        **kind.kwargs(params))
        plan[kind.key_for(params)] = kind.plan_value(params, dict(zip(todo, answer)))
    return dict(zip(todo, ranked))


def _sweep_plan(data, slo, start, end, window_normal, window_abnormal, ctx):
    """The driver's sweep plan for a DataFrame (None: not applicable -- no datetime window columns,
    an empty frame, or times that vary within a trace)."""
    if len(data) == 0 or not all(np.issubdtype(data[c].dtype, np.datetime64) for c in ("startTime", "endTime")):
        return None
    if pd.isna(start) or pd.isna(end) or not start < end:
        return None
    ctx = ctx or _lib.default_context()
    table, dev = span_table(data, ctx)
    return _sweep_plan_dev(table, dev, slo, start, end, window_normal, window_abnormal, ctx)


def _sweep_plan_dev(table, dev, slo, start, end, window_normal, window_abnormal, ctx):
    """_sweep_plan over a resident device table (RCAStream's appended one)."""
    if pd.isna(start) or pd.isna(end) or not start < end:
        return None
    a3, ok = slo_arrays(table, slo)
    return sweep_plan(ctx, table, dev, a3, ok, int(pd.Timestamp(start).value), int(pd.Timestamp(end).value),
                      int(window_normal.value), int(window_abnormal.value))


def _sweep_run(plan, iters, evidence):
    """The chain, one batched ranking of its triggered windows, then the driver's output replayed
    in window order; an empty window raises the reference's TypeError (T2) after the output of
    the windows before it."""
    events = sweep_chain(plan)
    _sweep_emit(plan, events, _sweep_rank(plan, events, "fp64", iters, evidence), evidence)


def _sweep_emit(plan, events, results, evidence):
    """The driver's output for the chain's events, in window order: the prints, result.csv and, from what
    sweep_rank left in ``results`` and in the plan, the file of everything ``evidence`` asks."""
    names = plan["table"].podop_names
    for e in events:
        if e[0] == "empty":
            print("Error: Current span list is empty ")
            anomaly_flag, normal_list, abnormal_list = False   # noqa: F841 -- TypeError, as the reference (T2)
        _, mm, na, nn, ranked = e
        print("anormaly_trace", na)                       # anormaly_detector.py:74-76
        print("total_trace", na + nn)
        print()
        if not na:
            continue
        print("anomaly_list", nn)                         # T1: the driver's abnormal_list is the
        print("normal_list", na)                          # detector's normal list
        print("total", na + nn)
        if not ranked:
            continue
        codes, scores, r_na, r_nn, _edges, status = results[mm][:6]
        if status != _lib.MR_OK or (r_na, r_nn) != (na, nn):
            raise RuntimeError(f"window {mm}: batch ranking disagrees with the sweep (status {status})")
        top_list = [names[c] for c in codes] if names is not None else codes.tolist()
        score_list = [np.float64(x) for x in scores]    # dstar2 over np.float64 weights
        for node, sc in zip(top_list, score_list):
            print("%-50s: %.8f" % (node, sc))             # online_rca.py:151
        print(top_list, score_list)
        _write_result(top_list, score_list)
        if evidence.exemplars is not None:   # (the batch's answer, trace names where the table has them)
            tnames = plan["table"].trace_names
            rows = {(names[c] if names is not None else c): [(tnames[r[0]] if tnames is not None else r[0],) + tuple(r[1:])
                                                             for r in lst]
                    for c, lst in results[mm][6].items()}
            _write_exemplars(top_list, score_list, rows, evidence.exemplar_kinds)
        for kind, params in evidence.kinds:   # (the batch's answer, by name)
            kind.file(top_list, score_list,
                      kind.names(plan["table"], kind.answers(plan[kind.key_for(params)])[mm], params), params)


def online_anomaly_detect_RCA(data, slo, operation_list, *, ctx=None, iters=ITERATIONS, exemplars=None,
                              exemplar_kinds=False, latency=None, latency_what="self", kind_breakdown=None,
                              call_edges=None, timeline=None, replicas=None, timeline_q=None, timeline_what="self",
                              kind_by="kind"):
    """online_rca.online_anomaly_detect_RCA (online_rca.py:155-216): 5-minute windows, a triggered
    window advances by 9 minutes; the detector's lists are unpacked swapped (T1), an empty
    window makes the unpacking raise TypeError (T2); result.csv is rewritten per trigger.

    With trace-level window times (the renamed TraceStart/TraceEnd, online_rca.py:229-230) the
    whole sweep runs as one device detector pass, one batched ranking of the triggered windows
    and a replay of the output (f3, :func:`_sweep_run`); otherwise window by window.

    iters: the PageRank iterations of every window (the reference's 25, pagerank.py:117; its README
    asks for more on a large system).

    exemplars: an integer m (1..32): every trigger also rewrites ``exemplars.csv`` beside result.csv
    (columns result, rank, trace, score): for each op of result.csv the m abnormal traces of the
    window to open first.  On the sweep path from the batch's own answer (rank_windows), window by
    window from window_exemplars.  stdout and result.csv do not change; without it no file is written.

    exemplar_kinds (with exemplars): one trace per trace kind (traces of the window with the same
    pod-ops and span count), each kind by its best trace; exemplars.csv gains a 5th column ``traces``,
    the number of abnormal traces of the window of that kind.  Without it the file is unchanged.

    latency: a q (a float in [0, 1] or a sequence of them): every trigger also rewrites ``latency.csv``
    beside result.csv (columns result, rank, side, spans, q, value): for each op of result.csv, in its
    order, the q-quantiles of the op's spans on the window's normal and then abnormal traces (one row
    per q; ``spans`` the op's rows on that side; value in the SLO's unit and rounding).  latency_what:
    "self" (a span's duration minus its children's: what separates a cause from its callers) or
    "duration".  On the sweep path from ONE windows_latency call over the triggered windows, window by
    window from op_latency.  stdout and result.csv do not change; without it no file is written.

    kind_breakdown: an integer m (1..32): every trigger also rewrites ``kinds.csv`` beside result.csv
    (columns result, rank, trace, n_abnormal, n_normal, spans, ops): which trace kinds (traces with the
    same pod-ops and span count) the anomaly hits -- first the whole window's m kinds with the most
    abnormal traces (``result`` = ``*``), then for each op of result.csv, in its order, the m such kinds
    among those that pass through the op; ``trace`` names a trace of the kind to open, n_abnormal /
    n_normal its traces on each side of the detector's partition, spans / ops a member's rows and
    distinct pod-ops.  From ONE windows_kind_breakdown call over the triggered windows on the sweep
    path, a call per window otherwise; tables whose window times vary within a trace are not covered
    (the call raises).  stdout and result.csv do not change; without it no file is written.

    kind_by (with kind_breakdown): "kind" (the default: kinds.csv as above) or "endpoint": every trigger rewrites
    ``endpoints.csv`` instead (columns result, rank, endpoint, traces_abnormal, traces_normal, mean_abnormal,
    mean_normal, max_abnormal, max_normal, live; kinds.csv is not written): which user-facing endpoints are hit --
    first the whole window's m endpoints with the most abnormal traces (``result`` = ``*``, rank 0), then for each
    op of result.csv, in its order, the m such endpoints among the traces that hold a span of the op, each trace
    once.  A trace's endpoint is the pod-op of its longest root span (``(none)`` without one); mean / max are of
    endTime - startTime (the SLO's unit and rounding); ``live`` the slot's endpoints with a trace.  From ONE
    windows_endpoints call over the triggered windows on the sweep path, a call per window otherwise.  Any other
    value, or "endpoint" without kind_breakdown, is a ValueError.

    call_edges: an integer m (1..32): every trigger also rewrites ``calls.csv`` beside result.csv
    (columns result, rank, direction, peer, calls_abnormal, calls_normal, mean_abnormal, mean_normal,
    max_abnormal, max_normal): for each op of result.csv, in its order, its m callers and then its m
    callees with the most calls on the abnormal traces -- the calls of the edge on each side of the
    detector's partition, and the mean and the largest duration of the called span (the SLO's unit and
    rounding, as latency.csv; a mean of no calls is 0.0).  From ONE windows_call_edges call over the
    triggered windows on the sweep path, a call per window otherwise.  stdout and result.csv do not
    change; without it no file is written.

    timeline: an integer B (1..512): every trigger also rewrites ``timeline.csv`` beside result.csv
    (columns result, rank, bucket, start, count_abnormal, count_normal, mean_abnormal, mean_normal,
    max_abnormal, max_normal): the window cut into B time buckets by trace start (``start`` the bucket's
    first ns) -- first the window's own traces (``result`` = ``*``, rank 0: how many normal and abnormal
    traces start in the bucket, the mean and the largest endTime - startTime), then for each op of
    result.csv, in its order, the op's spans on each side of the detector's partition with the mean and
    the largest self time (the SLO's unit and rounding, as calls.csv; a mean of no rows is 0.0).  From
    ONE windows_timeline call over the triggered windows on the sweep path, a call per window otherwise;
    tables whose window times vary within a trace are not covered (the call raises).  stdout and
    result.csv do not change; without it no file is written.

    timeline_q (with timeline): a q as latency's: every trigger also rewrites ``timeline_q.csv`` beside
    timeline.csv (columns result, rank, bucket, start, side, spans, q, value): the ``*`` block first, then each
    op of result.csv, in its order; per bucket the normal and then the abnormal side, one row per q -- ``spans``
    the bucket's count on that side, ``value`` the q-quantile of those spans' values (np.quantile, linear; the
    SLO's unit and rounding; 0.0 for no spans): a percentile SLO laid over the timeline.  timeline.csv does not
    change.  timeline_what: "self" or "duration", the value of an op's span in both files (the ``*`` block is
    endTime - startTime either way).  timeline_q without timeline is a ValueError.

    replicas: an integer m (1..32): every trigger also rewrites ``replicas.csv`` beside result.csv
    (columns result, rank, pod, is_result, count_abnormal, count_normal, mean_abnormal, mean_normal,
    max_abnormal, max_normal, live, replicas): is it the pod, or the operation?  For each op of result.csv,
    in its order, the m pod-ops of the same service-op (the op itself among them, ``is_result`` 1) with the
    most spans on the abnormal traces -- their spans on each side of the detector's partition with the mean
    and the largest self time (the SLO's unit and rounding, as calls.csv; a mean of no rows is 0.0) --
    then the replicas with a span in the window (``live``) and those the table knows (``replicas``).  From
    ONE windows_replicas call over the triggered windows on the sweep path, a call per window otherwise.
    stdout and result.csv do not change; without it no file is written."""
    check_converge_args(0.0, iters, 1)
    evidence = evidence_request(exemplars=exemplars, exemplar_kinds=exemplar_kinds, latency=latency,
                                latency_what=latency_what, kind_breakdown=kind_breakdown, call_edges=call_edges,
                                timeline=timeline, replicas=replicas, timeline_q=timeline_q, timeline_what=timeline_what,
                                kind_by=kind_by)
    window_normal = pd.Timedelta(minutes=5)
    window_abnormal = pd.Timedelta(minutes=4)
    start = data["startTime"].min()
    end = data["endTime"].max()
    plan = _sweep_plan(data, slo, start, end, window_normal, window_abnormal, ctx)
    if plan is not None:
        return _sweep_run(plan, iters, evidence)
    _window_loop(data, slo, operation_list, start, end, iters, evidence)


def _window_loop(data, slo, operation_list, current_time, end, iters=ITERATIONS, evidence=None):
    """online_rca.py:164-216 window by window from current_time while it is before end; returns
    where the chain goes on.  evidence: an evidence_request's answer (None: nothing beside result.csv); each
    trigger rewrites the file of everything it asks, from the one-window forms."""
    evidence = evidence or NOTHING
    window_normal = pd.Timedelta(minutes=5)
    window_abnormal = pd.Timedelta(minutes=4)
    while current_time < end:
        start_time = current_time
        end_time = current_time + window_normal
        anomaly_flag, normal_list, abnormal_list = system_anomaly_detect(
            data, start_time=start_time, end_time=end_time, slo=slo, operation_list=operation_list)
        if anomaly_flag:
            print("anomaly_list", len(abnormal_list))
            print("normal_list", len(normal_list))
            print("total", len(normal_list) + len(abnormal_list))
            if not abnormal_list or not normal_list:
                current_time += window_normal
                continue
            n_graph = get_pagerank_graph(normal_list, data)
            normal_trace_result, normal_num_list = trace_pagerank(*n_graph, False, iters=iters)
            a_graph = get_pagerank_graph(abnormal_list, data)
            anomaly_trace_result, anomaly_num_list = trace_pagerank(*a_graph, True, iters=iters)
            top_list, score_list = calculate_spectrum_without_delay_list(
                anomaly_result=anomaly_trace_result, normal_result=normal_trace_result,
                anomaly_list_len=len(abnormal_list), normal_list_len=len(normal_list), top_max=5,
                anomaly_num_list=anomaly_num_list, normal_num_list=normal_num_list, spectrum_method="dstar2")
            print(top_list, score_list)
            _write_result(top_list, score_list)
            if evidence.exemplars is not None:
                rows = window_exemplars(data, start_time, end_time, slo, top_list, m=evidence.exemplars, iters=iters,
                                        distinct_kinds=evidence.exemplar_kinds) if top_list else {}
                _write_exemplars(top_list, score_list, rows, evidence.exemplar_kinds)
            for kind, params in evidence.kinds:
                kind.file(top_list, score_list,
                          kind.window_for(params)(data, start_time, end_time, slo, top_list, **kind.kwargs(params)), params)
            current_time += window_abnormal
        current_time += window_normal
    return current_time


class RCAStream:
    """SURVEY 8(f) f3, online: online_anomaly_detect_RCA (online_rca.py:161-216) over spans that
    arrive in chunks.  Each chunk holds whole traces and chunks come in trace-start order (the
    OTel export's TraceStart order); push() ranks every window of the driver's chain that the data
    seen so far completes (a window [t, t + 5 min] is complete once a trace starting after t + 5 min
    has arrived), close() the rest up to the last endTime, as the offline driver would.  The
    output -- prints, result.csv, the T2 TypeError -- equals the offline driver's on the
    concatenated chunks.  Spans of traces that start before the chain's next window are dropped,
    so the resident table stays a few windows long; each push re-ingests that table on the device
    (mr_spans_ingest) and runs the chain's new windows as one sweep + one batched ranking.
    iters: the PageRank iterations of every window, as online_anomaly_detect_RCA's.  The evidence keywords
    are its keywords too, each file rewritten at every trigger: exemplars, exemplar_kinds (exemplars.csv);
    latency, latency_what (latency.csv); kind_breakdown (kinds.csv; with kind_by="endpoint" endpoints.csv); call_edges (calls.csv); timeline
    (timeline.csv), timeline_q (timeline_q.csv), timeline_what; replicas (replicas.csv).  They are kept
    checked, as one request, in ``evidence``."""

    WINDOW = pd.Timedelta(minutes=5)
    STEP_ABNORMAL = pd.Timedelta(minutes=4)

    def __init__(self, slo, operation_list, *, ctx=None, device_append=True, iters=ITERATIONS, exemplars=None,
                 exemplar_kinds=False, latency=None, latency_what="self", kind_breakdown=None, call_edges=None,
                 timeline=None, replicas=None, timeline_q=None, timeline_what="self", kind_by="kind"):
        check_converge_args(0.0, iters, 1)
        self.evidence = evidence_request(exemplars=exemplars, exemplar_kinds=exemplar_kinds, latency=latency,
                                         latency_what=latency_what, kind_breakdown=kind_breakdown,
                                         call_edges=call_edges, timeline=timeline, replicas=replicas,
                                         timeline_q=timeline_q, timeline_what=timeline_what, kind_by=kind_by)
        self.slo, self.operation_list, self.iters = slo, operation_list, iters
        self.ctx = ctx or _lib.default_context()
        self.data = None          # retained spans as a DataFrame (host mode only)
        self.cur = None           # the chain's next window start (pd.Timestamp)
        self.watermark = None     # largest trace start seen
        self.end = None           # largest trace end seen (the offline driver's loop bound)
        self.dead = False         # an empty window ended the driver (T2)
        # device mode (default): the resident table lives in HBM and grows by mr_spans_append, so
        # a push costs O(chunk) on the host and across PCIe; the chunk frames are kept (by
        # reference) only for the per-window fallback.  Host mode: pd.concat + a full re-ingest.
        self._stream = SpanStream(self.ctx) if device_append else None
        self._frames = []         # (chunk, its largest trace start) of the device mode
        self._empty = None        # a zero-row frame with the chunks' columns

    def push(self, chunk: pd.DataFrame):
        if self.dead:
            raise RuntimeError("RCAStream: the driver ended at an empty window")
        if len(chunk) == 0:
            return
        lo, hi, e = chunk["startTime"].min(), chunk["startTime"].max(), chunk["endTime"].max()
        if self.cur is None:
            self.cur = lo
        elif self.watermark is not None and lo < self.watermark:
            raise ValueError("RCAStream.push: chunks must arrive in trace-start order")
        self.watermark = hi if self.watermark is None else max(self.watermark, hi)
        self.end = e if self.end is None else max(self.end, e)
        arrays = SpanStream.accepts(chunk) if self._stream is not None else None
        if arrays is not None:
            self._stream.append(chunk, int(pd.Timestamp(self.cur).value), arrays)
            self._frames.append((chunk, hi))
            self._empty = chunk.iloc[:0]
        else:
            if self._stream is not None:   # a chunk the device append cannot take: host mode from here
                self.data = self._frame()
                self._stream.close()
                self._stream, self._frames = None, []
            self.data = chunk if self.data is None else pd.concat([self.data, chunk], ignore_index=True)
        # complete windows: start + 5 min < watermark
        self._advance(self.watermark - self.WINDOW, final=False)

    def close(self):
        if self.dead or (self.data is None if self._stream is None else self._stream.dev is None):
            return
        self._advance(self.end, final=True)

    def _frame(self):
        """The resident spans as a DataFrame (device mode: from the kept chunk frames)."""
        if self._stream is None:
            return self.data
        if not self._frames:
            return self._empty
        df = pd.concat([f for f, _ in self._frames], ignore_index=True) if len(self._frames) > 1 else self._frames[0][0]
        keep = df["startTime"] >= self.cur
        return df if keep.all() else df[keep].reset_index(drop=True)

    def _advance(self, limit, final):
        if not self.cur < limit:
            return
        try:
            if self._stream is not None:
                plan = _sweep_plan_dev(self._stream.table, self._stream.dev, self.slo, self.cur, limit, self.WINDOW,
                                       self.STEP_ABNORMAL, self.ctx)
            else:
                plan = _sweep_plan(self.data, self.slo, self.cur, limit, self.WINDOW, self.STEP_ABNORMAL, self.ctx)
            if plan is None:   # window times vary within a trace: window by window
                data = self._frame()
                if final:
                    self.cur = _window_loop(data, self.slo, self.operation_list, self.cur, limit, self.iters, self.evidence)
                else:
                    self.cur = self._loop_complete(data, limit)
            else:
                events = sweep_chain(plan)
                _sweep_emit(plan, events, _sweep_rank(plan, events, "fp64", self.iters, self.evidence), self.evidence)
                self.cur = self.cur + pd.Timedelta(plan["next_m"] * plan["grain"], unit="ns")
        except TypeError:
            self.dead = True
            raise
        if self._stream is not None:   # frames whose every trace started before the next window go
            self._frames = [(f, h) for f, h in self._frames if h >= self.cur]
            return
        keep = self.data["startTime"] >= self.cur   # traces before the next window leave the table
        if not keep.all():
            self.data = self.data[keep].reset_index(drop=True)

    def _loop_complete(self, data, limit):
        """The window loop for per-span times, one window at a time while its start is before limit."""
        cur = self.cur
        while cur < limit:
            cur = _window_loop(data, self.slo, self.operation_list, cur, cur + pd.Timedelta(1, unit="ns"), self.iters,
                               self.evidence)
        return cur


def _iter_args(iters, tol, check_every, info, info_type):
    """The window entries' iters / tol / check_every / info keywords, checked before any library
    call (graph.check_converge_args' rules; iters plays max_iters).  Returns tol as the C ABI's
    double (None: 0.0, a fixed count)."""
    check_converge_args(0.0 if tol is None else tol, iters, check_every)
    if info is not None and not isinstance(info, info_type):
        raise ValueError(f"info must be a {info_type.__name__} (or None)")
    return 0.0 if tol is None else float(tol)


def _window_report(iters_done, resid, i):
    return {"iters": int(iters_done[i]), "resid_normal": float(resid[2 * i]), "resid_anomaly": float(resid[2 * i + 1])}


def window_exemplars(data, start_time, end_time, slo, ops, *, m=5, iters=ITERATIONS, precision="fp64", ctx=None,
                     table=None, dev=None, distinct_kinds=False):
    """The traces to open for the ops a window's ranking names: for each pod-op of ``ops`` (names, or
    pod-op codes) the m abnormal traces of the window that matter most to the ranking among those the
    op occurs in -- {pod-op: [(traceID, score), ...]}, score descending.  Composed from entries that
    exist: mr_detect -> the abnormal traces' mask -> mr_graph_build -> mr_pagerank_ex (anomaly = 0:
    the flag the window path gives the graph of the detector's abnormal traces, T1) ->
    mr_graph_exemplars (DeviceGraph.exemplars).  An op absent from that graph maps to []; an empty
    window, or one without abnormal traces, returns {}.  distinct_kinds: one trace per trace kind of
    that graph (DeviceGraph.exemplars' keyword): (traceID, score, traces of that kind)."""
    m = check_exemplar_m(m)
    ops = check_exemplar_ops(ops)
    distinct_kinds = check_exemplar_kinds(distinct_kinds, m)
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
        raise ValueError(f"iters must be an integer >= 0, not {iters!r}")
    ctx = ctx or _lib.default_context()
    if table is None or dev is None:
        table, dev = span_table(data, ctx)
    state = _detect_state(ctx, table, dev, slo, start_time, end_time)
    mask = None if state is None else state == 2
    if mask is None or not mask.any():
        return {}
    pg = PagerankGraph(ctx, table, dev, mask)
    g = pg.device_graph()
    try:
        g.pagerank(False, iters=int(iters), precision=precision)
        node_of = {int(c): i for i, c in enumerate(pg.node_podop)}
        names = table.podop_names
        code_of = {n: c for c, n in enumerate(names)} if names is not None else {}
        idx = []
        for op in ops:
            code = int(op) if isinstance(op, (int, np.integer)) and not isinstance(op, bool) else code_of.get(op)
            idx.append(node_of.get(code, -1))
        have = [i for i in idx if i >= 0]
        out = {op: [] for op in ops}
        if have:
            tr, sc, cnt, *mult = g.exemplars_raw(have, m, distinct_kinds)
            tnames = table.trace_names
            j = 0
            for op, i in zip(ops, idx):
                if i < 0:
                    continue
                out[op] = [(tnames[int(pg.trace_code[t])] if tnames is not None else int(pg.trace_code[t]), np.float64(s))
                           for t, s in zip(tr[j, :cnt[j]], sc[j, :cnt[j]])]
                if distinct_kinds:
                    out[op] = [r + (int(c),) for r, c in zip(out[op], mult[0][j, :cnt[j]])]
                j += 1
        return out
    finally:
        g.close()


def rca_window(data, start_time, end_time, slo, *, top_max=5, spectrum_method="dstar2", precision="fp64", ctx=None,
               table=None, dev=None, iters=ITERATIONS, tol=None, check_every=5, info=None, exemplars=None,
               exemplar_kinds=False, latency=None, latency_what="self", kind_breakdown=None, call_edges=None,
               timeline=None, replicas=None, timeline_q=None, timeline_what="self", kind_by="kind"):
    """One RCA window entirely on the device (mr_rca_window_ex).  Returns a dict with the top list
    (pod-op names), scores, the detector counts and the edges traversed by the two PageRanks.

    iters: the PageRank iterations of both graphs (the reference's 25).  tol: stop at the first check
    (every check_every iterations, and at iters, now the maximum) where both graphs'
    max|s_k - s_{k-1}| is <= tol.  A dict passed as info receives ``iters`` (iterations run; 0 when
    nothing was ranked), ``resid_normal`` and ``resid_anomaly``: the last iteration's residual of the
    graph ranked as normal (the detector's abnormal traces, T1) and of the one ranked as anomaly.

    exemplars: an integer m adds the key ``"exemplars"``: window_exemplars for the ops of the top
    list, with this call's iters (with tol, the iterations the report says were run).  Every other
    key is what the call returns without the keyword.  exemplar_kinds (with exemplars): window_exemplars'
    distinct_kinds -- one trace per trace kind, as (traceID, score, traces of that kind).

    The other evidence keywords are online_anomaly_detect_RCA's; each adds one key for the ops of the top list
    and leaves every other key what it is:
    latency (with latency_what): ``"latency"``, op_latency's dict;
    kind_breakdown: ``"kinds"``, window_kinds' dict -- the whole window (key None), then the ops; with
    kind_by="endpoint" the key is ``"endpoints"`` instead, window_endpoints' dict in the same order;
    call_edges: ``"calls"``, window_calls' dict;
    timeline: ``"timeline"``, window_timeline's dict -- the window's own traces (key -1), then the ops; with
    timeline_q (a q as latency's) every slot carries ``"q"`` and ``"quantile"`` ([bucket][side][q], raw duration
    units) too, and timeline_what ("self" or "duration") chooses the value of an op's span;
    replicas: ``"replicas"``, window_replicas' dict."""
    tol = _iter_args(iters, tol, check_every, info, dict)
    evidence = evidence_request(exemplars=exemplars, exemplar_kinds=exemplar_kinds, latency=latency,
                                latency_what=latency_what, kind_breakdown=kind_breakdown, call_edges=call_edges,
                                timeline=timeline, replicas=replicas, timeline_q=timeline_q, timeline_what=timeline_what,
                                kind_by=kind_by)
    exemplars = evidence.exemplars
    ctx = ctx or _lib.default_context()
    if table is None or dev is None:
        table, dev = span_table(data, ctx)
    a3, ok = slo_arrays(table, slo)
    k = max(top_max + 6, 1)
    codes = np.zeros(k, np.int32)
    scores = np.zeros(k, np.float64)
    n_out, na, nn, edges = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    iters_done, resid = np.zeros(1, np.int32), np.zeros(2, np.float64)
    want = info is not None or (exemplars is not None and tol > 0.0)   # (with tol: the count for the exemplars)
    method = SPECTRUM_METHODS.index(spectrum_method)
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    ctx.check(_lib.load().mr_rca_window_ex(ctx.h, dev.h, to_ns(start_time), to_ns(end_time), ptr(a3, C.c_double),
                                           ptr(ok, C.c_uint8), method, top_max, prec, ptr(codes, C.c_int32),
                                           ptr(scores, C.c_double), C.byref(n_out), C.byref(edges), C.byref(na),
                                           C.byref(nn), int(iters), tol, int(check_every),
                                           ptr(iters_done if want else None, C.c_int32),
                                           ptr(resid if want else None, C.c_double)), "mr_rca_window_ex")
    if info is not None:
        info.update(_window_report(iters_done, resid, 0))
    m = n_out.value
    names = table.podop_names
    res = {"top": [names[c] for c in codes[:m]] if names is not None else codes[:m].tolist(),
           "score": scores[:m].tolist(), "n_abnormal": na.value, "n_normal": nn.value, "edges": edges.value}
    if exemplars is not None:
        k_run = int(iters_done[0]) if tol > 0.0 else int(iters)
        res["exemplars"] = window_exemplars(data, start_time, end_time, slo, res["top"], m=exemplars, iters=k_run,
                                            precision=precision, ctx=ctx, table=table, dev=dev,
                                            distinct_kinds=evidence.exemplar_kinds) if m else {}
    for kind, params in evidence.kinds:
        res[kind.key_for(params)] = kind.window_for(params)(data, start_time, end_time, slo, res["top"], ctx=ctx,
                                                            table=table, dev=dev, **kind.kwargs(params))
    return res


def _exemplar_rows(n, k, m, codes, n_out, ex_t, ex_s, ex_c, ex_m=None):
    """mr_windows_batch_exemplars' arrays as one {pod-op code: [(trace code, np.float64 score), ...]}
    per window (whole-array conversions: a Python-level loop per score costs more than the device side).
    ex_m (mr_windows_batch_exemplars_ex's class sizes): triples (trace code, score, class size)."""
    cod, cnt, no, tl, sl = codes.tolist(), ex_c.tolist(), n_out.tolist(), ex_t.tolist(), list(ex_s)
    ml = ex_m.tolist() if ex_m is not None else None
    out = []
    for i in range(n):
        rows = {}
        for j in range(i * k, i * k + no[i]):
            b = j * m
            if ml is not None:
                rows[cod[j]] = list(zip(tl[b:b + cnt[j]], sl[b:b + cnt[j]], ml[b:b + cnt[j]]))
                continue
            rows[cod[j]] = list(zip(tl[b:b + cnt[j]], sl[b:b + cnt[j]]))
        out.append(rows)
    return out


def rank_windows(ctx, windows, *, top_max=5, spectrum_method="dstar2", precision="fp64", iters=ITERATIONS, tol=None,
                 check_every=5, info=None, exemplars=None, exemplar_kinds=False):
    """C3: many RCA windows in one call (mr_windows_batch_ex).  ``windows``: a list of
    (DeviceSpans, t0_ns, t1_ns, a3, a3_valid) (the SLO arrays over the table's service-op
    codes).  Returns per window (top pod-op codes, scores, n_abnormal, n_normal, edges, status);
    status MR_ERR_VALUE marks an empty window (the reference raises TypeError there, T2).

    iters, tol, check_every as rca_window's; with tol the windows whose PageRanks share launches (a
    group) stop together, and the groups are ranked one after the other instead of pipelined.  A
    list passed as info is extended by one rca_window report per window, in order.  Each window's
    result is bit for bit that of a fixed-count call with its reported ``iters``.

    exemplars: an integer m (1..32) makes each window's tuple carry a 7th element, read on the device
    from what the window's ranking left (mr_windows_batch_exemplars): {pod-op code: [(trace code,
    np.float64 score), ...]} for the codes of its top list, in top-list order -- for each the m
    abnormal traces of the window that matter most to the ranking among those the pod-op occurs in,
    score descending; [] for a pod-op that occurs only in the window's normal traces.  Without the
    keyword the tuples stay 6 long, through mr_windows_batch_ex.

    exemplar_kinds (with exemplars; mr_windows_batch_exemplars_ex, MR_EX_DISTINCT_KINDS): one trace per
    trace kind of the window's graph of abnormal traces, each kind by its best trace, and the 7th
    element holds triples (trace code, score, traces of that kind in that graph)."""
    tol = _iter_args(iters, tol, check_every, info, list)
    exemplar_kinds = check_exemplar_kinds(exemplar_kinds, exemplars)
    if exemplars is not None:
        exemplars = check_exemplar_m(exemplars)
    n = len(windows)
    k = max(top_max + 6, 1)
    keep = [np.ascontiguousarray(w[3], np.float64) for w in windows] + \
           [np.ascontiguousarray(w[4], np.uint8) for w in windows]
    spans = (_lib.P * max(n, 1))(*[w[0].h for w in windows])
    t0 = np.array([int(w[1]) for w in windows], np.int64)
    t1 = np.array([int(w[2]) for w in windows], np.int64)
    a3 = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in keep[:n]])
    ok = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in keep[n:]])
    codes = np.zeros(max(n, 1) * k, np.int32)
    scores = np.zeros(max(n, 1) * k, np.float64)
    n_out, edges, na, nn, status = (np.zeros(max(n, 1), t) for t in (np.int32, np.int64, np.int32, np.int32, np.int32))
    iters_done, resid = np.zeros(max(n, 1), np.int32), np.zeros(2 * max(n, 1), np.float64)
    want = info is not None
    method = SPECTRUM_METHODS.index(spectrum_method)
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    args = (ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok, method, top_max, prec, ptr(codes, C.c_int32),
            ptr(scores, C.c_double), ptr(n_out, C.c_int32), ptr(edges, C.c_int64), ptr(na, C.c_int32), ptr(nn, C.c_int32),
            ptr(status, C.c_int32), int(iters), tol, int(check_every), ptr(iters_done if want else None, C.c_int32),
            ptr(resid if want else None, C.c_double))
    if exemplars is None:
        ctx.check(_lib.load().mr_windows_batch_ex(*args), "mr_windows_batch_ex")
    else:
        m = exemplars
        ex_t = np.full(max(n, 1) * k * m, -1, np.int32)
        ex_s = np.zeros(max(n, 1) * k * m, np.float64)
        ex_c = np.zeros(max(n, 1) * k, np.int32)
        ex_mu = np.zeros(max(n, 1) * k * m, np.int32) if exemplar_kinds else None
        if exemplar_kinds:
            ctx.check(_lib.load().mr_windows_batch_exemplars_ex(*args, m, ptr(ex_t, C.c_int32), ptr(ex_s, C.c_double),
                                                                ptr(ex_c, C.c_int32), _lib.MR_EX_DISTINCT_KINDS,
                                                                ptr(ex_mu, C.c_int32)), "mr_windows_batch_exemplars_ex")
        else:
            ctx.check(_lib.load().mr_windows_batch_exemplars(*args, m, ptr(ex_t, C.c_int32), ptr(ex_s, C.c_double),
                                                             ptr(ex_c, C.c_int32)), "mr_windows_batch_exemplars")
    if want:
        info.extend(_window_report(iters_done, resid, i) for i in range(n))
    out = [(codes[i * k:i * k + n_out[i]].copy(), scores[i * k:i * k + n_out[i]].copy(), int(na[i]), int(nn[i]),
            int(edges[i]), int(status[i])) for i in range(n)]
    if exemplars is None:
        return out
    return [res + (rows,) for res, rows in zip(out, _exemplar_rows(n, k, m, codes, n_out, ex_t, ex_s, ex_c, ex_mu))]
