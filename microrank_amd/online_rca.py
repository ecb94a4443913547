"""Drop-in for the reference module ``online_rca`` (online_rca.py).

* ``calculate_spectrum_without_delay_list`` -- the weighted spectrum scores and the stable
  top list (online_rca.py:33-152), computed on the GPU (K3, csrc/mr_spectrum.hip); printing,
  argument names and return types as in the reference.
* ``online_anomaly_detect_RCA`` -- the sliding-window driver (online_rca.py:155-216), line for
  line the same control flow, with every ranking step on the GPU.
* ``rca_window`` -- one whole window (detect -> 2 graphs -> 2 PageRanks -> spectrum) in a
  single C-ABI call with every intermediate resident in HBM (used by bench.py).
"""
from __future__ import annotations

import csv
import ctypes as C
import math
import time

import numpy as np
import pandas as pd

from . import _lib
from ._lib import SPECTRUM_METHODS, ptr
from .anormaly_detector import slo_arrays, system_anomaly_detect, trace_list_partition  # noqa: F401
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
    ranked = sorted(zip(top_list, score_list), key=lambda x: x[1], reverse=True)
    with open("result.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["level", "result", "rank", "confidence"])
        for rank, (service, score) in enumerate(ranked, start=1):
            w.writerow(["span", service, rank, float(score)])


def _write_exemplars(top_list, score_list, rows, kinds=False):
    """exemplars.csv beside result.csv: for each op of result.csv, in its order, the traces to open
    (rows: {op: [(trace, score), ...]}, best first).  kinds: the rows hold (trace, score, count), one
    trace per trace kind, and the file a 5th column ``traces``: the traces of that kind in the window."""
    ranked = sorted(zip(top_list, score_list), key=lambda x: x[1], reverse=True)
    with open("exemplars.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "trace", "score"] + (["traces"] if kinds else []))
        for service, _ in ranked:
            for rank, row in enumerate(rows.get(service, []), start=1):
                w.writerow([service, rank, row[0], float(row[1])] + ([int(row[2])] if kinds else []))


def _write_latency(top_list, score_list, rows, qv):
    """latency.csv beside result.csv: for each op of result.csv, in its order, the quantiles of the
    op's span values on the normal and then the abnormal traces of the window, one row per q (rows:
    op_latency's dict; ``spans`` the rows of the op on that side)."""
    ranked = sorted(zip(top_list, score_list), key=lambda x: x[1], reverse=True)
    with open("latency.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "side", "spans", "q", "value"])
        for rank, (service, _) in enumerate(ranked, start=1):
            row = rows.get(service)
            if row is None:
                continue
            for side in ("normal", "abnormal"):
                for qj, v in zip(qv, row[side]):
                    w.writerow([service, rank, side, int(row["n_" + side]), float(qj), float(v)])


def _write_kinds(top_list, score_list, rows):
    """kinds.csv beside result.csv: the whole window's block first (``result`` = ``*``), then for each op
    of result.csv, in its order, the op's trace kinds in answer order (rows: window_kinds' dict)."""
    ranked = sorted(zip(top_list, score_list), key=lambda x: x[1], reverse=True)
    with open("kinds.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "trace", "n_abnormal", "n_normal", "spans", "ops"])
        for label, key in [("*", None)] + [(service, service) for service, _ in ranked]:
            if key not in rows:
                continue
            for rank, e in enumerate(rows[key][0], start=1):
                w.writerow([label, rank, e[0], int(e[1]), int(e[2]), int(e[3]), int(e[4])])


def _write_calls(top_list, score_list, rows):
    """calls.csv beside result.csv: for each op of result.csv, in its order, its callers and then its
    callees in answer order (rows: window_calls' dict).  A mean is dsum / calls in float64 (0.0 for no
    calls); means and maxima in the SLO's unit and rounding, as latency.csv's values."""
    ranked = sorted(zip(top_list, score_list), key=lambda x: x[1], reverse=True)
    with open("calls.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "direction", "peer", "calls_abnormal", "calls_normal", "mean_abnormal",
                    "mean_normal", "max_abnormal", "max_normal"])
        for service, _ in ranked:
            if service not in rows:
                continue
            for direction, side in zip(("caller", "callee"), rows[service]):
                for rank, e in enumerate(side[0], start=1):
                    mean = [np.float64(e[3 + k]) / np.float64(e[1 + k]) if e[1 + k] else np.float64(0.0) for k in (0, 1)]
                    w.writerow([service, rank, direction, e[0], int(e[1]), int(e[2])] +
                               [float(x) for x in _latency_ms(mean)] + [float(x) for x in _latency_ms([e[5], e[6]])])


def _write_timeline(top_list, score_list, rows):
    """timeline.csv beside result.csv: the window's own block first (``result`` = ``*``, rank 0), then for
    each op of result.csv, in its order, one row per time bucket (rows: window_timeline's dict): the
    bucket's first ns, the rows (for ``*``: traces) that start in it on each side of the detector's
    partition, and the mean and the largest of their values.  A mean is sum / count in float64 (0.0 for
    no rows); means and maxima in the SLO's unit and rounding, as calls.csv's."""
    ranked = sorted(zip(top_list, score_list), key=lambda x: x[1], reverse=True)
    with open("timeline.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "bucket", "start", "count_abnormal", "count_normal", "mean_abnormal", "mean_normal",
                    "max_abnormal", "max_normal"])
        for rank, (label, key) in enumerate([("*", -1)] + [(service, service) for service, _ in ranked]):
            r = rows.get(key)
            if r is None:
                continue
            for b, (start, cnt, tot, mx) in enumerate(zip(r["start"], r["cnt"], r["sum"], r["max"])):
                mean = [np.float64(tot[k]) / np.float64(cnt[k]) if cnt[k] else np.float64(0.0) for k in (1, 0)]
                w.writerow([label, rank, b, int(start), int(cnt[1]), int(cnt[0])] + [float(x) for x in _latency_ms(mean)] +
                           [float(x) for x in _latency_ms([mx[1], mx[0]])])


def _write_replicas(top_list, score_list, rows):
    """replicas.csv beside result.csv: for each op of result.csv, in its order, the listed replicas of its
    service-op in answer order (rows: window_replicas' dict), one row per replica: its rows on each side of
    the detector's partition, the mean and the largest of their values, then the op's live replicas and the
    replicas the table knows.  ``is_result`` is 1 on the row of the ranked pod-op itself.  A mean is sum /
    count in float64 (0.0 for no rows); means and maxima in the SLO's unit and rounding, as calls.csv's."""
    ranked = sorted(zip(top_list, score_list), key=lambda x: x[1], reverse=True)
    with open("replicas.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "pod", "is_result", "count_abnormal", "count_normal", "mean_abnormal", "mean_normal",
                    "max_abnormal", "max_normal", "live", "replicas"])
        for service, _ in ranked:
            r = rows.get(service)
            if r is None:
                continue
            for rank, e in enumerate(r["entries"], start=1):
                mean = [np.float64(e[3 + k]) / np.float64(e[1 + k]) if e[1 + k] else np.float64(0.0) for k in (0, 1)]
                w.writerow([service, rank, e[0], int(e[0] == service), int(e[1]), int(e[2])] +
                           [float(x) for x in _latency_ms(mean)] + [float(x) for x in _latency_ms([e[5], e[6]])] +
                           [int(r["live"]), int(r["all"])])


def _replica_args(m, what="self"):
    """(m, MR_LAT_* code) of the replicas keywords: m an integer in 1..32, what "self" or "duration";
    ValueError otherwise -- before any device work."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= 32:
        raise ValueError(f"the replicas per op must be an integer in 1..32, not {m!r}")
    w = _lib.LATENCY_VALUES.get(what) if isinstance(what, str) else None
    if w is None:
        raise ValueError(f"what must be one of {sorted(_lib.LATENCY_VALUES)}, not {what!r}")
    return int(m), w


def _replica_names(table, rows):
    """windows_replicas' dict of one window with pod-op names (ops and replicas) where the table has them."""
    names = table.podop_names
    if names is None:
        return rows
    return {names[c]: dict(r, entries=[(names[e[0]],) + e[1:] for e in r["entries"]]) for c, r in rows.items()}


def _timeline_args(buckets, what="self"):
    """(buckets, MR_LAT_* code) of the timeline keywords: buckets an integer in 1..512, what "self" or
    "duration"; ValueError otherwise -- before any device work."""
    if isinstance(buckets, bool) or not isinstance(buckets, (int, np.integer)) or not 1 <= buckets <= 512:
        raise ValueError(f"the time buckets must be an integer in 1..512, not {buckets!r}")
    w = _lib.LATENCY_VALUES.get(what) if isinstance(what, str) else None
    if w is None:
        raise ValueError(f"what must be one of {sorted(_lib.LATENCY_VALUES)}, not {what!r}")
    return int(buckets), w


def _timeline_lists(r):
    """A slot of windows_timeline's answer as plain lists of Python ints."""
    return {k: v.tolist() for k, v in r.items()}


def _timeline_names(table, rows):
    """windows_timeline's dict of one window with pod-op names where the table has them (-1 stays -1)."""
    names = table.podop_names
    return {(c if c < 0 or names is None else names[c]): _timeline_lists(r) for c, r in rows.items()}


def _call_m(m):
    """The call_edges keyword / windows_call_edges' m: an integer in 1..32, else ValueError."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= 32:
        raise ValueError(f"the peers per op and direction must be an integer in 1..32, not {m!r}")
    return int(m)


def _call_names(table, rows):
    """windows_call_edges' dict of one window with pod-op names (ops and peers) where the table has them."""
    names = table.podop_names
    if names is None:
        return rows
    return {names[c]: tuple(([(names[e[0]],) + e[1:] for e in side[0]],) + side[1:] for side in r) for c, r in rows.items()}


def _kind_m(m):
    """The kind_breakdown keyword / windows_kind_breakdown's m: an integer in 1..32, else ValueError."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= 32:
        raise ValueError(f"the kinds per op must be an integer in 1..32, not {m!r}")
    return int(m)


def _kind_names(table, rows):
    """windows_kind_breakdown's dict of one window with pod-op and trace names where the table has them."""
    names, tnames = table.podop_names, table.trace_names
    return {(None if c is None else names[c] if names is not None else c):
            ([((tnames[e[0]] if tnames is not None else e[0]),) + e[1:] for e in r[0]],) + r[1:] for c, r in rows.items()}


def _latency_args(q, what, method="linear"):
    """(q as a float64 vector, MR_LAT_* code, MR_Q_* code) of the latency keywords; ValueError for a bad
    q (get_operation_quantiles' rules, at most 16 values), what or method -- before any device work."""
    qv, code = _quantile_args(q, method)
    if qv.size > 16:
        raise ValueError(f"q holds {qv.size} values; at most 16")
    w = _lib.LATENCY_VALUES.get(what) if isinstance(what, str) else None
    if w is None:
        raise ValueError(f"what must be one of {sorted(_lib.LATENCY_VALUES)}, not {what!r}")
    return qv, w, code


def _latency_ms(v):
    """Raw duration units -> the SLO's unit and rounding (preprocess_data.py:72-73)."""
    return [np.float64(x) for x in np.round(np.asarray(v, np.float64) / 1000.0, 4)]


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
               latency_what="self", kind_breakdown=None, call_edges=None, timeline=None, replicas=None):
    """Every ranked window of the chain in ONE mr_windows_batch_ex call: {m: (codes, scores, ...)}.
    exemplars, exemplar_kinds: rank_windows' keywords (a 7th element per window).
    latency (a q, scalar or sequence): ONE windows_latency call over the triggered windows' top lists;
    its answer goes to plan["latency"] = (q, {m: windows_latency's dict}) for the replay (latency.csv).
    kind_breakdown (an integer 1..32): ONE windows_kind_breakdown call over the triggered windows -- the
    whole window, then its top list; plan["kinds"] = {m: windows_kind_breakdown's dict} (kinds.csv).
    call_edges (an integer 1..32): ONE windows_call_edges call over the triggered windows' top lists;
    plan["calls"] = {m: windows_call_edges' dict} (calls.csv).
    timeline (an integer 1..512, the buckets): ONE windows_timeline call over the triggered windows -- the
    window's own traces (-1), then its top list; plan["timeline"] = {m: windows_timeline's dict}
    (timeline.csv).
    replicas (an integer 1..32): ONE windows_replicas call over the triggered windows' top lists;
    plan["replicas"] = {m: windows_replicas' dict} (replicas.csv)."""
    exemplar_kinds = check_exemplar_kinds(exemplar_kinds, exemplars)
    plan.pop("replicas", None)
    if replicas is not None:
        replicas = _replica_args(replicas)[0]
    plan.pop("latency", None)
    plan.pop("kinds", None)
    plan.pop("calls", None)
    plan.pop("timeline", None)
    if timeline is not None:
        timeline = _timeline_args(timeline)[0]
    if call_edges is not None:
        call_edges = _call_m(call_edges)
    if kind_breakdown is not None:
        kind_breakdown = _kind_m(kind_breakdown)
    if latency is not None:
        qv = _latency_args(latency, latency_what)[0]
    todo = [e[1] for e in events if e[0] == "window" and e[4]]
    width = plan["step_n"] * plan["grain"]
    if not todo:
        return {}
    wins = [(plan["dev"], plan["t_begin"] + mm * plan["grain"], plan["t_begin"] + mm * plan["grain"] + width,
             plan["a3"], plan["ok"]) for mm in todo]
    ranked = rank_windows(plan["ctx"], wins, precision=precision, iters=iters, exemplars=exemplars,
                          exemplar_kinds=exemplar_kinds)
    if latency is not None:
        lat = windows_latency(plan["ctx"], wins, [r[0] for r in ranked], q=qv, what=latency_what)
        plan["latency"] = (qv, dict(zip(todo, lat)))
    if kind_breakdown is not None:
        kinds = windows_kind_breakdown(plan["ctx"], wins, [[None] + r[0].tolist() for r in ranked], m=kind_breakdown)
        plan["kinds"] = dict(zip(todo, kinds))
    if call_edges is not None:
        calls = windows_call_edges(plan["ctx"], wins, [r[0] for r in ranked], m=call_edges)
        plan["calls"] = dict(zip(todo, calls))
    if timeline is not None:
        tl = windows_timeline(plan["ctx"], wins, [[-1] + r[0].tolist() for r in ranked], buckets=timeline)
        plan["timeline"] = dict(zip(todo, tl))
    if replicas is not None:
        rp = windows_replicas(plan["ctx"], wins, [r[0] for r in ranked], m=replicas)
        plan["replicas"] = dict(zip(todo, rp))
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


def _sweep_run(plan, iters=ITERATIONS, exemplars=None, exemplar_kinds=False, latency=None, latency_what="self",
               kind_breakdown=None, call_edges=None, timeline=None, replicas=None):
    """The chain, one batched ranking of its triggered windows, then the driver's output replayed
    in window order; an empty window raises the reference's TypeError (T2) after the output of
    the windows before it."""
    events = sweep_chain(plan)
    _sweep_emit(plan, events, sweep_rank(plan, events, iters=iters, exemplars=exemplars, exemplar_kinds=exemplar_kinds,
                                         latency=latency, latency_what=latency_what, kind_breakdown=kind_breakdown,
                                         call_edges=call_edges, timeline=timeline, replicas=replicas),
                exemplar_kinds)


def _sweep_emit(plan, events, results, exemplar_kinds=False):
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
        if len(results[mm]) > 6:   # (exemplars asked: the batch's answer, trace names where the table has them)
            tnames = plan["table"].trace_names
            rows = {(names[c] if names is not None else c): [(tnames[r[0]] if tnames is not None else r[0],) + tuple(r[1:])
                                                             for r in lst]
                    for c, lst in results[mm][6].items()}
            _write_exemplars(top_list, score_list, rows, exemplar_kinds)
        if "latency" in plan:   # (latency asked: the batch's answer in the SLO's unit, by name)
            qv, lat = plan["latency"]
            rows = {(names[c] if names is not None else c): {"normal": _latency_ms(r[0]), "abnormal": _latency_ms(r[1]),
                                                             "n_normal": r[2], "n_abnormal": r[3]}
                    for c, r in lat[mm].items()}
            _write_latency(top_list, score_list, rows, qv)
        if "kinds" in plan:     # (kind breakdown asked: the batch's answer, by name)
            _write_kinds(top_list, score_list, _kind_names(plan["table"], plan["kinds"][mm]))
        if "calls" in plan:     # (call evidence asked: the batch's answer, by name)
            _write_calls(top_list, score_list, _call_names(plan["table"], plan["calls"][mm]))
        if "timeline" in plan:  # (timeline asked: the batch's answer, by name)
            _write_timeline(top_list, score_list, _timeline_names(plan["table"], plan["timeline"][mm]))
        if "replicas" in plan:  # (replicas asked: the batch's answer, by name)
            _write_replicas(top_list, score_list, _replica_names(plan["table"], plan["replicas"][mm]))


def online_anomaly_detect_RCA(data, slo, operation_list, *, ctx=None, iters=ITERATIONS, exemplars=None,
                              exemplar_kinds=False, latency=None, latency_what="self", kind_breakdown=None,
                              call_edges=None, timeline=None, replicas=None):
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

    replicas: an integer m (1..32): every trigger also rewrites ``replicas.csv`` beside result.csv
    (columns result, rank, pod, is_result, count_abnormal, count_normal, mean_abnormal, mean_normal,
    max_abnormal, max_normal, live, replicas): is it the pod, or the operation?  For each op of result.csv,
    in its order, the m pod-ops of the same service-op (the op itself among them, ``is_result`` 1) with the
    most spans on the abnormal traces -- their spans on each side of the detector's partition with the mean
    and the largest self time (the SLO's unit and rounding, as calls.csv; a mean of no rows is 0.0) --
    then the replicas with a span in the window (``live``) and those the table knows (``replicas``).  From
    ONE windows_replicas call over the triggered windows on the sweep path, a call per window otherwise.
    stdout and result.csv do not change; without it no file is written."""
    if replicas is not None:
        replicas = _replica_args(replicas)[0]
    if timeline is not None:
        timeline = _timeline_args(timeline)[0]
    if call_edges is not None:
        call_edges = _call_m(call_edges)
    if kind_breakdown is not None:
        kind_breakdown = _kind_m(kind_breakdown)
    check_converge_args(0.0, iters, 1)
    exemplar_kinds = check_exemplar_kinds(exemplar_kinds, exemplars)
    if exemplars is not None:
        exemplars = check_exemplar_m(exemplars)
    if latency is not None:
        _latency_args(latency, latency_what)
    window_normal = pd.Timedelta(minutes=5)
    window_abnormal = pd.Timedelta(minutes=4)
    start = data["startTime"].min()
    end = data["endTime"].max()
    plan = _sweep_plan(data, slo, start, end, window_normal, window_abnormal, ctx)
    if plan is not None:
        return _sweep_run(plan, iters, exemplars, exemplar_kinds, latency, latency_what, kind_breakdown, call_edges,
                          timeline, replicas)
    _window_loop(data, slo, operation_list, start, end, iters, exemplars, exemplar_kinds, latency, latency_what,
                 kind_breakdown, call_edges, timeline, replicas)


def _window_loop(data, slo, operation_list, current_time, end, iters=ITERATIONS, exemplars=None, exemplar_kinds=False,
                 latency=None, latency_what="self", kind_breakdown=None, call_edges=None, timeline=None, replicas=None):
    """online_rca.py:164-216 window by window from current_time while it is before end; returns
    where the chain goes on."""
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
            if exemplars is not None:
                rows = window_exemplars(data, start_time, end_time, slo, top_list, m=exemplars, iters=iters,
                                        distinct_kinds=exemplar_kinds) if top_list else {}
                _write_exemplars(top_list, score_list, rows, exemplar_kinds)
            if latency is not None:
                rows = op_latency(data, start_time, end_time, slo, top_list, q=latency, what=latency_what) if top_list else {}
                _write_latency(top_list, score_list, rows, _latency_args(latency, latency_what)[0])
            if kind_breakdown is not None:
                _write_kinds(top_list, score_list, window_kinds(data, start_time, end_time, slo, top_list, m=kind_breakdown))
            if call_edges is not None:
                _write_calls(top_list, score_list, window_calls(data, start_time, end_time, slo, top_list, m=call_edges))
            if timeline is not None:
                _write_timeline(top_list, score_list,
                                window_timeline(data, start_time, end_time, slo, top_list, buckets=timeline))
            if replicas is not None:
                _write_replicas(top_list, score_list, window_replicas(data, start_time, end_time, slo, top_list, m=replicas))
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
    iters: the PageRank iterations of every window, as online_anomaly_detect_RCA's; exemplars,
    exemplar_kinds: its keywords (exemplars.csv rewritten at every trigger); latency, latency_what: its
    keywords (latency.csv rewritten at every trigger); kind_breakdown: its keyword (kinds.csv rewritten
    at every trigger); call_edges: its keyword (calls.csv rewritten at every trigger); timeline: its keyword
    (timeline.csv rewritten at every trigger); replicas: its keyword (replicas.csv rewritten at every trigger)."""

    WINDOW = pd.Timedelta(minutes=5)
    STEP_ABNORMAL = pd.Timedelta(minutes=4)

    def __init__(self, slo, operation_list, *, ctx=None, device_append=True, iters=ITERATIONS, exemplars=None,
                 exemplar_kinds=False, latency=None, latency_what="self", kind_breakdown=None, call_edges=None,
                 timeline=None, replicas=None):
        check_converge_args(0.0, iters, 1)
        self.replicas = None if replicas is None else _replica_args(replicas)[0]
        self.timeline = None if timeline is None else _timeline_args(timeline)[0]
        self.call_edges = None if call_edges is None else _call_m(call_edges)
        self.kind_breakdown = None if kind_breakdown is None else _kind_m(kind_breakdown)
        if latency is not None:
            _latency_args(latency, latency_what)
        self.latency, self.latency_what = latency, latency_what
        self.exemplar_kinds = check_exemplar_kinds(exemplar_kinds, exemplars)
        self.exemplars = None if exemplars is None else check_exemplar_m(exemplars)
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
                    self.cur = _window_loop(data, self.slo, self.operation_list, self.cur, limit, self.iters, self.exemplars,
                                            self.exemplar_kinds, self.latency, self.latency_what, self.kind_breakdown,
                                            self.call_edges, self.timeline, self.replicas)
                else:
                    self.cur = self._loop_complete(data, limit)
            else:
                events = sweep_chain(plan)
                _sweep_emit(plan, events, sweep_rank(plan, events, iters=self.iters, exemplars=self.exemplars,
                                                     exemplar_kinds=self.exemplar_kinds, latency=self.latency,
                                                     latency_what=self.latency_what,
                                                     kind_breakdown=self.kind_breakdown,
                                                     call_edges=self.call_edges, timeline=self.timeline,
                                                     replicas=self.replicas),
                            self.exemplar_kinds)
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
            nxt = _window_loop(data, self.slo, self.operation_list, cur, cur + pd.Timedelta(1, unit="ns"), self.iters,
                               self.exemplars, self.exemplar_kinds, self.latency, self.latency_what, self.kind_breakdown,
                               self.call_edges, self.timeline, self.replicas)
            cur = nxt
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
    a3, ok = slo_arrays(table, slo)
    state = np.zeros(table.n_traces, np.uint8)
    na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
    rc = _lib.load().mr_detect(ctx.h, dev.h, to_ns(start_time), to_ns(end_time), ptr(a3, C.c_double),
                               ptr(ok, C.c_uint8), ptr(state, C.c_uint8), C.byref(na), C.byref(nn), C.byref(nin))
    if rc == _lib.MR_ERR_VALUE and nin.value == 0:
        return {}
    ctx.check(rc, "mr_detect")
    mask = state == 2
    if not mask.any():
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
               timeline=None, replicas=None):
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

    latency: a q (scalar or sequence) adds the key ``"latency"``: op_latency's dict for the ops of the
    top list (latency_what: "self" or "duration").  Every other key stays what it is.

    kind_breakdown: an integer m (1..32) adds the key ``"kinds"``: window_kinds' dict for the whole
    window (key None) and then the ops of the top list.  Every other key stays what it is.

    call_edges: an integer m (1..32) adds the key ``"calls"``: window_calls' dict for the ops of the top
    list.  Every other key stays what it is.

    timeline: an integer B (1..512) adds the key ``"timeline"``: window_timeline's dict for the window's
    own traces (key -1) and then the ops of the top list, over B buckets.  Every other key stays what it is.

    replicas: an integer m (1..32) adds the key ``"replicas"``: window_replicas' dict for the ops of the top
    list, m replicas each.  Every other key stays what it is."""
    tol = _iter_args(iters, tol, check_every, info, dict)
    if replicas is not None:
        replicas = _replica_args(replicas)[0]
    if timeline is not None:
        timeline = _timeline_args(timeline)[0]
    if call_edges is not None:
        call_edges = _call_m(call_edges)
    if kind_breakdown is not None:
        kind_breakdown = _kind_m(kind_breakdown)
    if latency is not None:
        _latency_args(latency, latency_what)
    exemplar_kinds = check_exemplar_kinds(exemplar_kinds, exemplars)
    if exemplars is not None:
        exemplars = check_exemplar_m(exemplars)
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
                                            distinct_kinds=exemplar_kinds) if m else {}
    if latency is not None:
        res["latency"] = op_latency(data, start_time, end_time, slo, res["top"], q=latency, what=latency_what, ctx=ctx,
                                    table=table, dev=dev) if m else {}
    if kind_breakdown is not None:
        res["kinds"] = window_kinds(data, start_time, end_time, slo, res["top"], m=kind_breakdown, ctx=ctx, table=table,
                                    dev=dev)
    if call_edges is not None:
        res["calls"] = window_calls(data, start_time, end_time, slo, res["top"], m=call_edges, ctx=ctx, table=table,
                                    dev=dev)
    if timeline is not None:
        res["timeline"] = window_timeline(data, start_time, end_time, slo, res["top"], buckets=timeline, ctx=ctx,
                                          table=table, dev=dev)
    if replicas is not None:
        res["replicas"] = window_replicas(data, start_time, end_time, slo, res["top"], m=replicas, ctx=ctx, table=table,
                                          dev=dev)
    return res


def _op_codes(table, ops):
    """Pod-op codes of ``ops`` (names of the table's pod-ops, or codes); ValueError for any other."""
    names = table.podop_names
    code_of = {n: c for c, n in enumerate(names)} if names is not None else {}
    codes = []
    for op in ops:
        if isinstance(op, (int, np.integer)) and not isinstance(op, bool):
            code = int(op) if 0 <= int(op) < table.n_podops else None
        else:
            code = code_of.get(op)
        if code is None:
            raise ValueError(f"{op!r} is no pod-op of the span table")
        codes.append(code)
    return codes


def op_latency(data, start_time, end_time, slo, ops, *, q=(0.5, 0.99), what="self", method="linear", ctx=None,
               table=None, dev=None):
    """How slow are the ops a window's ranking names, in the abnormal traces and in the normal ones?
    For each pod-op of ``ops`` (names, or pod-op codes) the q-quantiles (np.quantile's semantics,
    ``method`` 'linear', 'lower' or 'higher') of its spans' values on each side of the detector's
    partition of the window: {op: {"normal": [...], "abnormal": [...], "n_normal": int, "n_abnormal":
    int}} (mr_detect, then mr_op_latency; csrc/mr_latency.hip).  ``what``: "self" -- a span's duration
    minus the durations of its children (the spans whose ParentSpanId is its spanID), which does not
    grow when a callee is slow -- or "duration".  Values are np.float64, np.round(v / 1000.0, 4): the
    SLO's unit and rounding, as get_operation_quantiles gives them; a side without a span of the op
    has n 0 and values 0.0.  An op that is no pod-op of the table raises ValueError; an empty window
    returns {}."""
    qv, wcode, mcode = _latency_args(q, what, method)
    ops = list(ops)
    ctx = ctx or _lib.default_context()
    if table is None or dev is None:
        table, dev = span_table(data, ctx)
    codes = _op_codes(table, ops)
    if not ops:
        return {}
    a3, ok = slo_arrays(table, slo)
    state = np.zeros(table.n_traces, np.uint8)
    na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
    lib = _lib.load()
    rc = lib.mr_detect(ctx.h, dev.h, to_ns(start_time), to_ns(end_time), ptr(a3, C.c_double), ptr(ok, C.c_uint8),
                       ptr(state, C.c_uint8), C.byref(na), C.byref(nn), C.byref(nin))
    if rc == _lib.MR_ERR_VALUE and nin.value == 0:
        return {}
    ctx.check(rc, "mr_detect")
    res = {}
    for b in range(0, len(ops), 64):   # (mr_op_latency's op limit)
        cod = np.asarray(codes[b:b + 64], np.int32)
        out = np.zeros((cod.size, 2, qv.size), np.float64)
        cnt = np.zeros((cod.size, 2), np.int64)
        ctx.check(lib.mr_op_latency(ctx.h, dev.h, to_ns(start_time), to_ns(end_time), ptr(state, C.c_uint8),
                                    ptr(cod, C.c_int32), cod.size, wcode, ptr(qv, C.c_double), qv.size, mcode,
                                    ptr(out, C.c_double), ptr(cnt, C.c_int64)), "mr_op_latency")
        for j, op in enumerate(ops[b:b + 64]):
            res[op] = {"normal": _latency_ms(out[j, 0]), "abnormal": _latency_ms(out[j, 1]),
                       "n_normal": int(cnt[j, 0]), "n_abnormal": int(cnt[j, 1])}
    return res


def _window_args(windows):
    """``windows`` (rank_windows' tuples) as the leading arguments of the library's evidence entries:
    (keep, spans, t0, t1, a3, ok).  a3 / ok point into ``keep``, the contiguous SLO arrays, which must
    outlive the call; windows that share their SLO array objects give the library one pointer: one upload."""
    n = len(windows)
    keep = [np.ascontiguousarray(w[3], np.float64) for w in windows] + \
           [np.ascontiguousarray(w[4], np.uint8) for w in windows]
    addr = {}
    for i, w in enumerate(windows):
        for src, a in ((w[3], keep[i]), (w[4], keep[n + i])):
            addr.setdefault(id(src), a.ctypes.data)
    spans = (_lib.P * n)(*[w[0].h for w in windows])
    t0 = np.array([int(w[1]) for w in windows], np.int64)
    t1 = np.array([int(w[2]) for w in windows], np.int64)
    a3 = (C.c_void_p * n)(*[addr[id(w[3])] for w in windows])
    ok = (C.c_void_p * n)(*[addr[id(w[4])] for w in windows])
    return keep, spans, t0, t1, a3, ok


def _asked_args(ops, n, none_ok=False):
    """``ops``, one sequence of pod-op codes per window (none_ok: None allowed, passed as -1), as (asked, k,
    cod, n_ops): the codes as Python lists, the widest list's length (at least 1), the (n, k) int32 codes
    and the n list lengths.  ValueError unless there are n lists of at most 64 codes."""
    if len(ops) != n:
        raise ValueError(f"ops holds {len(ops)} lists for {n} windows")
    asked = [[None if none_ok and o is None else int(o) for o in lst] for lst in ops]
    k = max([len(a) for a in asked] + [1])
    if k > 64:
        raise ValueError(f"a window asks {k} ops; at most 64")
    cod = np.zeros((n, k), np.int32)
    n_ops = np.array([len(a) for a in asked], np.int32)
    for i, a in enumerate(asked):
        cod[i, :len(a)] = [-1 if c is None else c for c in a]
    return asked, k, cod, n_ops


def windows_latency(ctx, windows, ops, *, q=(0.5, 0.99), what="self", method="linear"):
    """op_latency's evidence for many windows in one call (mr_windows_latency: one sort for all of
    them).  ``windows`` as rank_windows'; ``ops`` one array of pod-op codes per window -- the first
    element of rank_windows' tuples.  Returns per window {code: (normal[n_q], abnormal[n_q], n_normal,
    n_abnormal)} in raw duration units (rank_windows works in codes; names and rounding are the
    callers'); each window's partition is its own detector's, computed on the device.  An empty
    window (rank_windows' status MR_ERR_VALUE) answers zeros."""
    qv, wcode, mcode = _latency_args(q, what, method)
    n = len(windows)
    asked, k, cod, n_ops = _asked_args([np.ascontiguousarray(o, np.int32).reshape(-1) for o in ops], n)
    if n == 0:
        return []
    keep, spans, t0, t1, a3, ok = _window_args(windows)
    out = np.zeros((n, k, 2, qv.size), np.float64)
    cnt = np.zeros((n, k, 2), np.int64)
    status = np.zeros(n, np.int32)
    ctx.check(_lib.load().mr_windows_latency(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                             ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, wcode, ptr(qv, C.c_double),
                                             qv.size, mcode, ptr(out, C.c_double), ptr(cnt, C.c_int64),
                                             ptr(status, C.c_int32)), "mr_windows_latency")
    return [{c: (out[i, j, 0].copy(), out[i, j, 1].copy(), int(cnt[i, j, 0]), int(cnt[i, j, 1]))
             for j, c in enumerate(asked[i])} for i in range(n)]


def windows_kind_breakdown(ctx, windows, ops, *, m=8):
    """Which trace kinds does each window's anomaly hit (mr_windows_kind_breakdown,
    csrc/mr_kind_breakdown.hip)?  ``windows`` as rank_windows'; ``ops`` one sequence per window of
    pod-op codes, None standing for "every kind" (the window's overall breakdown).  A kind is the
    table's exact class of a trace: its set of pod-ops and its span count's fp32 reciprocal.  Returns
    per window {code or None: (entries, n_kinds, n_abnormal, n_normal)}: ``entries`` the first m kinds
    among the live kinds that contain the pod-op, as (trace code, n_abnormal, n_normal, spans, ops) --
    most abnormal traces first, then fewest normal ones, then the smallest trace code; the trace is
    the kind's first abnormal member (its first normal one where it has none), spans / ops a member's
    rows and distinct pod-ops -- ``n_kinds`` the number of such kinds, ``n_abnormal`` / ``n_normal``
    the traces of ALL of them on each side of the window's own detector partition.  An empty window
    (rank_windows' status MR_ERR_VALUE) answers ([], 0, 0, 0).  ValueError for more than 64 ops in a
    window, m outside 1..32 or len(ops) != len(windows); tables without trace-level times or without
    a layout order are not covered (RuntimeError from the library)."""
    m = _kind_m(m)
    n = len(windows)
    asked, k, cod, n_ops = _asked_args(ops, n, none_ok=True)
    if n == 0:
        return []
    keep, spans, t0, t1, a3, ok = _window_args(windows)
    col = [np.zeros((n, k, m), np.int32) for _ in range(5)]
    cnt, kinds = np.zeros((n, k), np.int32), np.zeros((n, k), np.int32)
    tot = np.zeros((n, k, 2), np.int64)
    status = np.zeros(n, np.int32)
    ctx.check(_lib.load().mr_windows_kind_breakdown(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                                    ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, m,
                                                    *[ptr(c, C.c_int32) for c in col], ptr(cnt, C.c_int32),
                                                    ptr(kinds, C.c_int32), ptr(tot, C.c_int64), ptr(status, C.c_int32)),
              "mr_windows_kind_breakdown")
    cols = [c.tolist() for c in col]
    return [{c: (list(zip(*[cl[i][j][:cnt[i, j]] for cl in cols])), int(kinds[i, j]), int(tot[i, j, 0]), int(tot[i, j, 1]))
             for j, c in enumerate(asked[i])} for i in range(n)]


def window_kinds(data, start_time, end_time, slo, ops, *, m=8, ctx=None, table=None, dev=None):
    """windows_kind_breakdown for one window by names: {None: the whole window, pod-op: ...} for the
    pod-ops of ``ops`` (names, or codes), each (entries, n_kinds, n_abnormal, n_normal) with trace
    names in the entries where the table has them.  An op that is no pod-op of the table raises
    ValueError; ops past the call's 64 slots go in further calls."""
    m = _kind_m(m)
    ops = list(ops)
    ctx = ctx or _lib.default_context()
    if table is None or dev is None:
        table, dev = span_table(data, ctx)
    codes = _op_codes(table, ops)
    a3, ok = slo_arrays(table, slo)
    win = (dev, to_ns(start_time), to_ns(end_time), a3, ok)
    asked = [None] + codes
    rows = {}
    for b in range(0, len(asked), 64):
        rows.update(windows_kind_breakdown(ctx, [win], [asked[b:b + 64]], m=m)[0])
    tnames = table.trace_names
    return {key: ([((tnames[e[0]] if tnames is not None else e[0]),) + e[1:] for e in rows[c][0]],) + rows[c][1:]
            for key, c in zip([None] + ops, asked)}


def windows_call_edges(ctx, windows, ops, *, m=8):
    """Who calls each window's suspect ops, and whom do they call (mr_windows_call_edges,
    csrc/mr_call_edges.hip)?  ``windows`` as rank_windows'; ``ops`` one sequence of pod-op codes per
    window -- the first element of rank_windows' tuples.  Returns per window {code: (callers, callees)},
    each side (entries, n_peers, (calls_abnormal, calls_normal)): ``entries`` the first m peers among
    those with a call in the window, as (peer code, calls_abn, calls_nor, dsum_abn, dsum_nor, dmax_abn,
    dmax_nor) -- most abnormal calls first, then fewest normal ones, then the smallest peer code; a
    call is a (child span, parent span) pair whose two traces lie on the same side of the window's own
    detector partition, dsum / dmax the sum (int64, wrapping) and the maximum of the CHILD span's
    duration in raw units -- ``n_peers`` the number of such peers and the totals the calls of ALL of
    them.  An empty window (rank_windows' status MR_ERR_VALUE) answers ([], 0, (0, 0)) twice.
    ValueError for more than 64 ops in a window, m outside 1..32 or len(ops) != len(windows); trace
    shards and time windows on tables without trace-level times are not covered (RuntimeError from the
    library)."""
    m = _call_m(m)
    n = len(windows)
    asked, k, cod, n_ops = _asked_args(ops, n)
    if n == 0:
        return []
    keep, spans, t0, t1, a3, ok = _window_args(windows)
    peer = np.zeros((n, k, 2, m), np.int32)
    calls, dsum, dmax = (np.zeros((n, k, 2, m, 2), np.int64) for _ in range(3))
    cnt, peers = np.zeros((n, k, 2), np.int32), np.zeros((n, k, 2), np.int32)
    tot = np.zeros((n, k, 2, 2), np.int64)
    status = np.zeros(n, np.int32)
    ctx.check(_lib.load().mr_windows_call_edges(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                                ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, m, ptr(peer, C.c_int32),
                                                ptr(calls, C.c_int64), ptr(dsum, C.c_int64), ptr(dmax, C.c_int64),
                                                ptr(cnt, C.c_int32), ptr(peers, C.c_int32), ptr(tot, C.c_int64),
                                                ptr(status, C.c_int32)), "mr_windows_call_edges")
    pl, cl, sl, xl = peer.tolist(), calls.tolist(), dsum.tolist(), dmax.tolist()

    def side(i, j, d):
        ent = [(pl[i][j][d][e], cl[i][j][d][e][1], cl[i][j][d][e][0], sl[i][j][d][e][1], sl[i][j][d][e][0],
                xl[i][j][d][e][1], xl[i][j][d][e][0]) for e in range(cnt[i, j, d])]
        return ent, int(peers[i, j, d]), (int(tot[i, j, d, 1]), int(tot[i, j, d, 0]))

    return [{c: (side(i, j, 0), side(i, j, 1)) for j, c in enumerate(asked[i])} for i in range(n)]


def window_calls(data, start_time, end_time, slo, ops, *, m=8, ctx=None, table=None, dev=None):
    """windows_call_edges for one window by names: {pod-op: (callers, callees)} for the pod-ops of
    ``ops`` (names, or codes), peers by name where the table has names.  An op that is no pod-op of
    the table raises ValueError; ops past the call's 64 slots go in further calls."""
    m = _call_m(m)
    ops = list(ops)
    ctx = ctx or _lib.default_context()
    if table is None or dev is None:
        table, dev = span_table(data, ctx)
    codes = _op_codes(table, ops)
    if not ops:
        return {}
    a3, ok = slo_arrays(table, slo)
    win = (dev, to_ns(start_time), to_ns(end_time), a3, ok)
    rows = {}
    for b in range(0, len(codes), 64):
        rows.update(windows_call_edges(ctx, [win], [codes[b:b + 64]], m=m)[0])
    names = table.podop_names
    pn = (lambda c: names[c]) if names is not None else (lambda c: c)
    return {key: tuple(([(pn(e[0]),) + e[1:] for e in sd[0]],) + sd[1:] for sd in rows[c]) for key, c in zip(ops, codes)}


def _per_window(v, n, what):
    """A bucket origin / width keyword as n Python ints: one value for every window, or one per window."""
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return [int(v)] * n
    out = [int(x) for x in v]
    if len(out) != n:
        raise ValueError(f"{what} holds {len(out)} values for {n} windows")
    return out


def windows_timeline(ctx, windows, ops, *, buckets=30, what="self", origin=None, width=None):
    """When inside each window did it happen (mr_windows_timeline, csrc/mr_timeline.hip)?  ``windows`` as
    rank_windows'; ``ops`` one sequence per window of pod-op codes, -1 standing for the window's own
    traces.  Returns per window {code or -1: {"start": int64[B], "cnt": int64[B, 2], "sum": int64[B, 2],
    "max": int64[B, 2], "out": int64[2, 2]}}: the window cut into B = ``buckets`` time buckets by TRACE
    start, ``start`` each bucket's first ns; per bucket and side (0 normal, 1 abnormal, the window's own
    detector partition) the op's spans whose trace starts in the bucket, the sum (int64, wrapping) and the
    largest of their values in raw duration units -- ``what``: "self" (duration minus the children's) or
    "duration"; for -1 the traces, each once, valued endTime - startTime; ``max`` is 0 where ``cnt`` is 0 --
    and ``out[side]`` the spans (traces) that start before / after the bucket range.
    Bucket b covers [origin + b * width, origin + (b + 1) * width): by default origin = the window's t0 and
    width = (t1 - t0) // B + 1, which puts every start of [t0, t1] into a bucket, so ``out`` is 0; ``origin``
    / ``width`` (ns; one value, or one per window) choose another grid.  A whole-table window
    (INT64_MIN, INT64_MAX) needs both.  An empty window (rank_windows' status MR_ERR_VALUE) answers zeros.
    ValueError for buckets outside 1..512, an unknown what, more than 64 ops in a window, a width <= 0 or
    len(ops) != len(windows); tables without trace-level times, self time on a trace shard and -1 on a
    trace shard are not covered (RuntimeError from the library)."""
    b, wcode = _timeline_args(buckets, what)
    n = len(windows)
    asked, k, cod, n_ops = _asked_args(ops, n)
    if n == 0:
        return []
    ends = [(int(w[1]), int(w[2])) for w in windows]
    if (origin is None or width is None) and (_lib.INT64_MIN, _lib.INT64_MAX) in ends:
        raise ValueError("a whole-table window has no default buckets: give origin and width")
    org = _per_window(origin, n, "origin") if origin is not None else [a for a, _ in ends]
    wid = _per_window(width, n, "width") if width is not None else [(z - a) // b + 1 for a, z in ends]
    if any(x <= 0 for x in wid):
        raise ValueError(f"a bucket width must be positive, not {min(wid)}")
    b0, bw = np.array(org, np.int64), np.array(wid, np.int64)
    keep, spans, t0, t1, a3, ok = _window_args(windows)   # (behind the checks: they need no table)
    cnt, tot, mx = (np.zeros((n, k, b, 2), np.int64) for _ in range(3))
    out = np.zeros((n, k, 2, 2), np.int64)
    status = np.zeros(n, np.int32)
    ctx.check(_lib.load().mr_windows_timeline(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                              ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, wcode, ptr(b0, C.c_int64),
                                              ptr(bw, C.c_int64), b, ptr(cnt, C.c_int64), ptr(tot, C.c_int64),
                                              ptr(mx, C.c_int64), ptr(out, C.c_int64), ptr(status, C.c_int32)),
              "mr_windows_timeline")
    res = []
    for i in range(n):
        start = b0[i] + np.arange(b, dtype=np.int64) * bw[i]   # (int64 that wraps, for grids past the int64 range)
        res.append({c: {"start": start, "cnt": cnt[i, j].copy(), "sum": tot[i, j].copy(), "max": mx[i, j].copy(),
                        "out": out[i, j].copy()} for j, c in enumerate(asked[i])})
    return res


def window_timeline(data, start_time, end_time, slo, ops, *, buckets=30, what="self", ctx=None, table=None, dev=None):
    """windows_timeline for one window by names: {-1: the window's own traces, pod-op: ...} for the pod-ops
    of ``ops`` (names, or codes), each {"start", "cnt", "sum", "max", "out"} as plain lists of ints over the
    default buckets (origin = the window's start, width = (end - start) // buckets + 1 ns).  An op that is
    no pod-op of the table raises ValueError; ops past the call's 64 slots go in further calls."""
    buckets, _ = _timeline_args(buckets, what)
    ops = list(ops)
    ctx = ctx or _lib.default_context()
    if table is None or dev is None:
        table, dev = span_table(data, ctx)
    codes = _op_codes(table, ops)
    a3, ok = slo_arrays(table, slo)
    win = (dev, to_ns(start_time), to_ns(end_time), a3, ok)
    asked = [-1] + codes
    rows = {}
    for b in range(0, len(asked), 64):
        rows.update(windows_timeline(ctx, [win], [asked[b:b + 64]], buckets=buckets, what=what)[0])
    return {key: _timeline_lists(rows[c]) for key, c in zip([-1] + ops, asked)}


def windows_replicas(ctx, windows, ops, *, m=8, what="self"):
    """Is it the pod, or the operation (mr_windows_replicas, csrc/mr_replicas.hip)?  ``windows`` as
    rank_windows'; ``ops`` one sequence of pod-op codes per window -- the first element of rank_windows'
    tuples.  A pod-op's replicas are the pod-ops that share its service-op on the table's rows.  Returns
    per window {code: {"entries": [(pod code, cnt_abn, cnt_nor, sum_abn, sum_nor, max_abn, max_nor), ...],
    "live": int, "all": int, "place": int, "own": (6 ints, the entries' order), "total": (6 ints)}}:
    ``entries`` the first m replicas among those with a span in the window -- most abnormal spans first, then
    fewest normal ones, then the smallest code; the asked op is a replica like any other -- with the spans
    on each side of the window's own detector partition, the sum (int64, wrapping) and the largest of their
    values in raw duration units (``what``: "self", duration minus the children's, or "duration"; a max of no
    span is 0); ``live`` the replicas with a span in the window, ``all`` those the table knows, ``place`` the
    asked op's 0-based place among ALL live replicas (-1: it has no span in the window; it can be >= m),
    ``own`` its own numbers, listed or not, and ``total`` the numbers over all live replicas: the service-op's
    own.  An empty window (rank_windows' status MR_ERR_VALUE) answers empty entries, place -1 and zeros.
    ValueError for m outside 1..32, an unknown what, more than 64 ops in a window or len(ops) !=
    len(windows); time windows on tables without trace-level times, self time on a trace shard and tables
    where a pod-op has rows of two service-ops are not covered (RuntimeError from the library)."""
    m, wcode = _replica_args(m, what)
    n = len(windows)
    asked, k, cod, n_ops = _asked_args(ops, n)
    if n == 0:
        return []
    keep, spans, t0, t1, a3, ok = _window_args(windows)
    pod = np.zeros((n, k, m), np.int32)
    cnt, tot, mx = (np.zeros((n, k, m, 2), np.int64) for _ in range(3))
    cn, live, every, place = (np.zeros((n, k), np.int32) for _ in range(4))
    own, total = np.zeros((n, k, 2, 3), np.int64), np.zeros((n, k, 2, 3), np.int64)
    status = np.zeros(n, np.int32)
    ctx.check(_lib.load().mr_windows_replicas(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                              ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, m, wcode, ptr(pod, C.c_int32),
                                              ptr(cnt, C.c_int64), ptr(tot, C.c_int64), ptr(mx, C.c_int64),
                                              ptr(cn, C.c_int32), ptr(live, C.c_int32), ptr(every, C.c_int32),
                                              ptr(place, C.c_int32), ptr(own, C.c_int64), ptr(total, C.c_int64),
                                              ptr(status, C.c_int32)), "mr_windows_replicas")
    # (plain lists: a call answers thousands of entries, and indexing numpy scalars would cost more than the call)
    # and an entry's tuples come from one zip over the seven planes, abnormal before normal)
    planes = [a[..., side].tolist() for a in (cnt, tot, mx) for side in (1, 0)]
    pl, nl, ll, al, el = pod.tolist(), cn.tolist(), live.tolist(), every.tolist(), place.tolist()

    def six(v):   # [.., side, {cnt, sum, max}] -> (cnt_abn, cnt_nor, sum_abn, sum_nor, max_abn, max_nor)
        return v[:, :, ::-1, :].transpose(0, 1, 3, 2).reshape(n, k, 6).tolist()

    ol, tl = six(own), six(total)

    def one(i, j):
        return {"entries": list(zip(pl[i][j][:nl[i][j]], *[p[i][j] for p in planes])), "live": ll[i][j], "all": al[i][j],
                "place": el[i][j], "own": tuple(ol[i][j]), "total": tuple(tl[i][j])}

    return [{c: one(i, j) for j, c in enumerate(asked[i])} for i in range(n)]


def window_replicas(data, start_time, end_time, slo, ops, *, m=8, what="self", ctx=None, table=None, dev=None):
    """windows_replicas for one window by names: {pod-op: {"entries", "live", "all", "place", "own", "total"}}
    for the pod-ops of ``ops`` (names, or codes), replicas by name where the table has names.  An op that is
    no pod-op of the table raises ValueError; ops past the call's 64 slots go in further calls."""
    m, _ = _replica_args(m, what)
    ops = list(ops)
    ctx = ctx or _lib.default_context()
    if table is None or dev is None:
        table, dev = span_table(data, ctx)
    codes = _op_codes(table, ops)
    if not ops:
        return {}
    a3, ok = slo_arrays(table, slo)
    win = (dev, to_ns(start_time), to_ns(end_time), a3, ok)
    rows = {}
    for b in range(0, len(codes), 64):
        rows.update(windows_replicas(ctx, [win], [codes[b:b + 64]], m=m, what=what)[0])
    names = table.podop_names
    pn = (lambda c: names[c]) if names is not None else (lambda c: c)
    return {key: dict(rows[c], entries=[(pn(e[0]),) + e[1:] for e in rows[c]["entries"]]) for key, c in zip(ops, codes)}


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
