"""The evidence kinds beside a window's ranking: latency, trace kinds, call edges, timeline, replicas.

Everything a kind owns is here: the check of its keyword, its batch entry (``windows_*``: many windows in
one library call, answers in pod-op codes), its one-window form by names (``window_*`` / ``op_latency``),
the mapper from a batch answer to rows by name and the writer of its CSV file.  ``KINDS`` lists the kinds in
call order and ``evidence_request`` checks a caller's keywords into one request; the drivers in
``online_rca`` loop over that request and never name a kind.  A new kind is one record in ``KINDS``, its
keyword in ``evidence_request`` and in the four public signatures of ``online_rca``, and a docstring line.
An option of a kind (the timeline's ``timeline_q`` / ``timeline_what``) is a keyword of ``evidence_request`` that
ends up in that kind's parameters; ``Kind.batch_for`` / ``window_for`` pick the form that takes them.  A second
grouping of a kind (``kind_by="endpoint"``: the kind breakdown by entry operation) is such an option too: its forms,
its key and its file are a record of ``Kind.variants``.
"""
from __future__ import annotations

import csv
import ctypes as C
from dataclasses import dataclass
from types import MappingProxyType
from typing import Callable, NamedTuple

import numpy as np

from . import _lib
from ._lib import ptr
from .anormaly_detector import slo_arrays
from .graph import check_exemplar_kinds, check_exemplar_m
from .preprocess_data import _quantile_args, span_table
from .spans import to_ns


# ------------------------------------------------------------------------------------------ arguments
def _int_in(value, lo, hi, text):
    """``value`` as an int when it is an integer (no bool) in lo..hi; ValueError naming ``text`` otherwise."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError(f"{text} must be an integer in {lo}..{hi}, not {value!r}")
    return int(value)


def _what_code(what):
    """The MR_LAT_* code of a ``what`` keyword ("self" or "duration"); ValueError otherwise."""
    w = _lib.LATENCY_VALUES.get(what) if isinstance(what, str) else None
    if w is None:
        raise ValueError(f"what must be one of {sorted(_lib.LATENCY_VALUES)}, not {what!r}")
    return w


def _replica_args(m, what="self"):
    """(m, MR_LAT_* code) of the replicas keywords: m an integer in 1..32, what "self" or "duration";
    ValueError otherwise -- before any device work."""
    return _int_in(m, 1, 32, "the replicas per op"), _what_code(what)


def _timeline_args(buckets, what="self"):
    """(buckets, MR_LAT_* code) of the timeline keywords: buckets an integer in 1..512, what "self" or
    "duration"; ValueError otherwise -- before any device work."""
    return _int_in(buckets, 1, 512, "the time buckets"), _what_code(what)


class _TimelineAsk(NamedTuple):
    """The timeline keyword with one of its options (evidence_request): B, timeline_q, timeline_what."""
    buckets: object
    q: object
    what: object


def _timeline_params(v):
    """The timeline kind's parameters: {"buckets": B} for the keyword alone; with timeline_q / timeline_what
    (a _TimelineAsk) also "q" (a float64 vector, _latency_args' rules) and / or "what"."""
    if not isinstance(v, _TimelineAsk):
        return {"buckets": _timeline_args(v)[0]}
    params = {"buckets": _timeline_args(v.buckets, v.what)[0]}
    if v.q is not None:
        params["q"] = _latency_args(v.q, v.what)[0].copy()
        params["q"].setflags(write=False)   # (the request is read-only)
    if v.what != "self":
        params["what"] = v.what
    return params


def _call_m(m):
    """The call_edges keyword / windows_call_edges' m: an integer in 1..32, else ValueError."""
    return _int_in(m, 1, 32, "the peers per op and direction")


def _kind_m(m):
    """The kind_breakdown keyword / windows_kind_breakdown's m: an integer in 1..32, else ValueError."""
    return _int_in(m, 1, 32, "the kinds per op")


def _endpoint_m(m):
    """windows_endpoints' m (the kind_breakdown keyword with kind_by="endpoint"): an integer in 1..32, else
    ValueError."""
    return _int_in(m, 1, 32, "the endpoints per op")


class _KindAsk(NamedTuple):
    """The kind_breakdown keyword with its kind_by option (evidence_request): m, "endpoint"."""
    m: object
    by: str


def _kind_params(v):
    """The kind_breakdown kind's parameters: {"m": m} for the keyword alone (trace kinds); with
    kind_by="endpoint" (a _KindAsk) {"m": m, "by": "endpoint"}: the traces grouped by entry operation."""
    if not isinstance(v, _KindAsk):
        return {"m": _kind_m(v)}
    return {"m": _endpoint_m(v.m), "by": v.by}


def _latency_args(q, what, method="linear"):
    """(q as a float64 vector, MR_LAT_* code, MR_Q_* code) of the latency keywords; ValueError for a bad
    q (get_operation_quantiles' rules, at most 16 values), what or method -- before any device work."""
    qv, code = _quantile_args(q, method)
    if qv.size > 16:
        raise ValueError(f"q holds {qv.size} values; at most 16")
    return qv, _what_code(what), code


def _latency_ms(v):
    """Raw duration units -> the SLO's unit and rounding (preprocess_data.py:72-73)."""
    return [np.float64(x) for x in np.round(np.asarray(v, np.float64) / 1000.0, 4)]


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


def _per_window(v, n, what):
    """A bucket origin / width keyword as n Python ints: one value for every window, or one per window."""
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return [int(v)] * n
    out = [int(x) for x in v]
    if len(out) != n:
        raise ValueError(f"{what} holds {len(out)} values for {n} windows")
    return out


# -------------------------------------------------------------------------------------- batch entries
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
    trace shard are not covered (RuntimeError from the library).
    windows_timeline_q is this call with latency quantiles per bucket."""
    return _windows_timeline(ctx, windows, ops, buckets, what, origin, width, None, "linear")


def windows_timeline_q(ctx, windows, ops, *, q=(0.5, 0.99), buckets=30, what="self", origin=None, width=None,
                       method="linear"):
    """windows_timeline with the latency quantiles of every bucket and side (mr_windows_timeline_q: one selection
    of packed keys and ONE sort per chunk of windows): a percentile SLO laid over the timeline.  ``q``: a float in
    [0, 1] or up to 16 of them; ``method``: 'linear', 'lower' or 'higher'.  Each answer is windows_timeline's dict
    for the same arguments, and gains "q": float64[n_q] and "quantile": float64[B, 2, n_q] -- np.quantile of the
    values counted in ``cnt`` (side 0 normal, 1 abnormal), in raw duration units, 0.0 where ``cnt`` is 0; the spans
    before / after the bucket range get none.  A bad q or method is a ValueError before any device work; values
    whose range takes more bits than a 64-bit key holds beside the class are a ValueError from the library."""
    qv, _, mcode = _latency_args(q, what, method)
    return _windows_timeline(ctx, windows, ops, buckets, what, origin, width, qv, mcode)


def _windows_timeline(ctx, windows, ops, buckets, what, origin, width, qv, mcode):
    """windows_timeline (qv None) / windows_timeline_q (qv, mcode: _latency_args')."""
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
    lead = (ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok, ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k,
            wcode, ptr(b0, C.c_int64), ptr(bw, C.c_int64), b)
    outs = (ptr(cnt, C.c_int64), ptr(tot, C.c_int64), ptr(mx, C.c_int64), ptr(out, C.c_int64))
    if qv is None:
        ctx.check(_lib.load().mr_windows_timeline(*lead, *outs, ptr(status, C.c_int32)), "mr_windows_timeline")
    else:
        tq = np.zeros((n, k, b, 2, qv.size), np.float64)
        ctx.check(_lib.load().mr_windows_timeline_q(*lead, ptr(qv, C.c_double), qv.size, mcode, *outs, ptr(tq, C.c_double),
                                                    ptr(status, C.c_int32)), "mr_windows_timeline_q")
    res = []
    for i in range(n):
        start = b0[i] + np.arange(b, dtype=np.int64) * bw[i]   # (int64 that wraps, for grids past the int64 range)
        res.append({c: {"start": start, "cnt": cnt[i, j].copy(), "sum": tot[i, j].copy(), "max": mx[i, j].copy(),
                        "out": out[i, j].copy()} for j, c in enumerate(asked[i])})
        if qv is not None:
            for j, c in enumerate(asked[i]):
                res[i][c].update(q=qv.copy(), quantile=tq[i, j].copy())
    return res


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


def windows_endpoints(ctx, windows, ops, *, m=8):
    """Which user-facing endpoints are hit, and through which does the anomaly reach each op
    (mr_windows_endpoints, csrc/mr_endpoints.hip)?  ``windows`` as rank_windows'; ``ops`` one sequence per window of
    pod-op codes, None standing for the whole window.  A trace's endpoint is the pod-op of its entry row -- its
    longest root span (no parent in the table), ties to the first row -- or None for a trace without a root row;
    its value is endTime - startTime.  An op selects the traces with at least one of its spans, each ONCE.
    Returns per window {code or None: {"entries": [(endpoint code or None, cnt_abn, cnt_nor, sum_abn, sum_nor,
    max_abn, max_nor), ...], "live": int, "total": (6 ints, the entries' order)}}: ``entries`` the first m
    endpoints among those with a selected trace -- most abnormal traces first, then fewest normal ones, then the
    smallest code, None last -- with the traces on each side of the window's own detector partition, the sum
    (int64, wrapping) and the largest of their values in raw time units (a max of no trace is 0); ``live`` the
    endpoints with a selected trace and ``total`` the numbers over all of them.  An empty window (rank_windows'
    status MR_ERR_VALUE) answers empty entries and zeros.  ValueError for m outside 1..32, more than 64 ops in a
    window or len(ops) != len(windows); trace shards and tables without a per-trace index or trace-level times
    are not covered (RuntimeError from the library)."""
    m = _endpoint_m(m)
    n = len(windows)
    asked, k, cod, n_ops = _asked_args(ops, n, none_ok=True)
    if n == 0:
        return []
    keep, spans, t0, t1, a3, ok = _window_args(windows)
    eop = np.zeros((n, k, m), np.int32)
    cnt, tot, mx = (np.zeros((n, k, m, 2), np.int64) for _ in range(3))
    cn, live = np.zeros((n, k), np.int32), np.zeros((n, k), np.int32)
    total = np.zeros((n, k, 2, 3), np.int64)
    status = np.zeros(n, np.int32)
    ctx.check(_lib.load().mr_windows_endpoints(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                               ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, m, ptr(eop, C.c_int32),
                                               ptr(cnt, C.c_int64), ptr(tot, C.c_int64), ptr(mx, C.c_int64),
                                               ptr(cn, C.c_int32), ptr(live, C.c_int32), ptr(total, C.c_int64),
                                               ptr(status, C.c_int32)), "mr_windows_endpoints")
    planes = [a[..., side].tolist() for a in (cnt, tot, mx) for side in (1, 0)]   # (abnormal before normal)
    el, nl, ll = eop.tolist(), cn.tolist(), live.tolist()
    tl = total[:, :, ::-1, :].transpose(0, 1, 3, 2).reshape(n, k, 6).tolist()

    def one(i, j):
        codes = [None if c == _lib.MR_EP_NONE else c for c in el[i][j][:nl[i][j]]]
        return {"entries": list(zip(codes, *[p[i][j] for p in planes])), "live": ll[i][j], "total": tuple(tl[i][j])}

    return [{c: one(i, j) for j, c in enumerate(asked[i])} for i in range(n)]


# ------------------------------------------------------------------ answers in codes -> rows by name
def _latency_row(table, r):
    """A slot of windows_latency's answer as op_latency gives it: the SLO's unit and rounding."""
    return {"normal": _latency_ms(r[0]), "abnormal": _latency_ms(r[1]), "n_normal": r[2], "n_abnormal": r[3]}


def _kind_row(table, r):
    """A slot of windows_kind_breakdown's answer with trace names where the table has them."""
    tnames = table.trace_names
    return ([((tnames[e[0]] if tnames is not None else e[0]),) + e[1:] for e in r[0]],) + r[1:]


def _call_row(table, r):
    """A slot of windows_call_edges' answer with the peers' pod-op names where the table has them."""
    names = table.podop_names
    return tuple(([((names[e[0]] if names is not None else e[0]),) + e[1:] for e in side[0]],) + side[1:] for side in r)


def _timeline_row(table, r):
    """A slot of windows_timeline's answer as plain lists of Python ints ("q" and "quantile", where the answer
    has them: lists of floats)."""
    return {k: v.tolist() for k, v in r.items()}


def _replica_row(table, r):
    """A slot of windows_replicas' answer with the replicas' pod-op names where the table has them."""
    names = table.podop_names
    return dict(r, entries=[((names[e[0]] if names is not None else e[0]),) + e[1:] for e in r["entries"]])


def _endpoint_row(table, r):
    """A slot of windows_endpoints' answer with the endpoints' pod-op names where the table has them (None stays)."""
    names = table.podop_names
    return dict(r, entries=[((names[e[0]] if names is not None and e[0] is not None else e[0]),) + e[1:]
                            for e in r["entries"]])


# ------------------------------------------------------------------------------------ one-window forms
def _detect_state(ctx, table, dev, slo, start, end):
    """The detector's partition of one window (mr_detect) as the per-trace state vector (uint8; 2 marks an
    abnormal trace); None for the empty window."""
    a3, ok = slo_arrays(table, slo)
    state = np.zeros(table.n_traces, np.uint8)
    na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
    rc = _lib.load().mr_detect(ctx.h, dev.h, to_ns(start), to_ns(end), ptr(a3, C.c_double), ptr(ok, C.c_uint8),
                               ptr(state, C.c_uint8), C.byref(na), C.byref(nn), C.byref(nin))
    if rc == _lib.MR_ERR_VALUE and nin.value == 0:
        return None
    ctx.check(rc, "mr_detect")
    return state


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
    state = _detect_state(ctx, table, dev, slo, start_time, end_time)
    if state is None:
        return {}
    res = {}
    for b in range(0, len(ops), 64):   # (mr_op_latency's op limit)
        cod = np.asarray(codes[b:b + 64], np.int32)
        out = np.zeros((cod.size, 2, qv.size), np.float64)
        cnt = np.zeros((cod.size, 2), np.int64)
        ctx.check(_lib.load().mr_op_latency(ctx.h, dev.h, to_ns(start_time), to_ns(end_time), ptr(state, C.c_uint8),
                                            ptr(cod, C.c_int32), cod.size, wcode, ptr(qv, C.c_double), qv.size, mcode,
                                            ptr(out, C.c_double), ptr(cnt, C.c_int64)), "mr_op_latency")
        for j, op in enumerate(ops[b:b + 64]):
            res[op] = {"normal": _latency_ms(out[j, 0]), "abnormal": _latency_ms(out[j, 1]),
                       "n_normal": int(cnt[j, 0]), "n_abnormal": int(cnt[j, 1])}
    return res


def _one_window(batch, lead, params, row, data, start_time, end_time, slo, ops, ctx, table, dev):
    """A batch entry for one window by names: {lead op or op as given: ``row`` of its slot} for ``lead`` (the
    kind's pseudo-op, or nothing) and then the pod-ops of ``ops`` (names, or codes), asked in slices of the
    entry's 64 slots.  An op that is no pod-op of the table raises ValueError; nothing to ask answers {}."""
    ops = list(ops)
    ctx = ctx or _lib.default_context()
    if table is None or dev is None:
        table, dev = span_table(data, ctx)
    asked = list(lead) + _op_codes(table, ops)
    if not asked:
        return {}
    a3, ok = slo_arrays(table, slo)
    win = (dev, to_ns(start_time), to_ns(end_time), a3, ok)
    rows = {}
    for b in range(0, len(asked), 64):
        rows.update(batch(ctx, [win], [asked[b:b + 64]], **params)[0])
    return {key: row(table, rows[c]) for key, c in zip(list(lead) + ops, asked)}


def window_kinds(data, start_time, end_time, slo, ops, *, m=8, ctx=None, table=None, dev=None):
    """windows_kind_breakdown for one window by names: {None: the whole window, pod-op: ...} for the
    pod-ops of ``ops`` (names, or codes), each (entries, n_kinds, n_abnormal, n_normal) with trace
    names in the entries where the table has them.  An op that is no pod-op of the table raises
    ValueError; ops past the call's 64 slots go in further calls."""
    return _one_window(windows_kind_breakdown, (None,), {"m": _kind_m(m)}, _kind_row, data, start_time, end_time, slo,
                       ops, ctx, table, dev)


def window_calls(data, start_time, end_time, slo, ops, *, m=8, ctx=None, table=None, dev=None):
    """windows_call_edges for one window by names: {pod-op: (callers, callees)} for the pod-ops of
    ``ops`` (names, or codes), peers by name where the table has names.  An op that is no pod-op of
    the table raises ValueError; ops past the call's 64 slots go in further calls."""
    return _one_window(windows_call_edges, (), {"m": _call_m(m)}, _call_row, data, start_time, end_time, slo, ops, ctx,
                       table, dev)


def window_timeline(data, start_time, end_time, slo, ops, *, buckets=30, what="self", ctx=None, table=None, dev=None):
    """windows_timeline for one window by names: {-1: the window's own traces, pod-op: ...} for the pod-ops
    of ``ops`` (names, or codes), each {"start", "cnt", "sum", "max", "out"} as plain lists of ints over the
    default buckets (origin = the window's start, width = (end - start) // buckets + 1 ns).  An op that is
    no pod-op of the table raises ValueError; ops past the call's 64 slots go in further calls.
    window_timeline_q is this call with latency quantiles per bucket."""
    return _one_window(windows_timeline, (-1,), {"buckets": _timeline_args(buckets, what)[0], "what": what},
                       _timeline_row, data, start_time, end_time, slo, ops, ctx, table, dev)


def window_timeline_q(data, start_time, end_time, slo, ops, *, q=(0.5, 0.99), buckets=30, what="self", method="linear",
                      ctx=None, table=None, dev=None):
    """windows_timeline_q for one window by names: window_timeline's dict for the same arguments, each slot with
    "q" and "quantile" ([bucket][side][q], raw duration units) as lists of floats.  A bad q is a ValueError before
    any device work."""
    params = {"q": _latency_args(q, what, method)[0], "buckets": _timeline_args(buckets, what)[0], "what": what,
              "method": method}
    return _one_window(windows_timeline_q, (-1,), params, _timeline_row, data, start_time, end_time, slo, ops, ctx, table,
                       dev)


def window_replicas(data, start_time, end_time, slo, ops, *, m=8, what="self", ctx=None, table=None, dev=None):
    """windows_replicas for one window by names: {pod-op: {"entries", "live", "all", "place", "own", "total"}}
    for the pod-ops of ``ops`` (names, or codes), replicas by name where the table has names.  An op that is
    no pod-op of the table raises ValueError; ops past the call's 64 slots go in further calls."""
    return _one_window(windows_replicas, (), {"m": _replica_args(m, what)[0], "what": what}, _replica_row, data,
                       start_time, end_time, slo, ops, ctx, table, dev)


def window_endpoints(data, start_time, end_time, slo, ops, *, m=8, ctx=None, table=None, dev=None):
    """windows_endpoints for one window by names: {None: the whole window, pod-op: {"entries", "live", "total"}}
    for the pod-ops of ``ops`` (names, or codes), endpoints by pod-op name where the table has names (None: the
    traces without a root row).  An op that is no pod-op of the table raises ValueError; ops past the call's 64
    slots go in further calls."""
    return _one_window(windows_endpoints, (None,), {"m": _endpoint_m(m)}, _endpoint_row, data, start_time, end_time,
                       slo, ops, ctx, table, dev)


# --------------------------------------------------------------------------------------------- writers
def _ranked(top_list, score_list):
    """result.csv's order: (op, score) by score, best first, ties in top-list order."""
    return sorted(zip(top_list, score_list), key=lambda x: x[1], reverse=True)


def _mean_max(cnt, tot, mx):
    """The mean and max columns of a row, abnormal before normal: cnt, tot (a sum) and mx as (abnormal, normal)
    pairs.  A mean is sum / count in float64 (0.0 for a count of 0); means and maxima in the SLO's unit and
    rounding, as latency.csv's values."""
    mean = [np.float64(t) / np.float64(c) if c else np.float64(0.0) for c, t in zip(cnt, tot)]
    return [float(x) for x in _latency_ms(mean + list(mx))]


def _write_latency(top_list, score_list, rows, qv):
    """latency.csv beside result.csv: for each op of result.csv, in its order, the quantiles of the
    op's span values on the normal and then the abnormal traces of the window, one row per q (rows:
    op_latency's dict; ``spans`` the rows of the op on that side)."""
    with open("latency.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "side", "spans", "q", "value"])
        for rank, (service, _) in enumerate(_ranked(top_list, score_list), start=1):
            row = rows.get(service)
            if row is None:
                continue
            for side in ("normal", "abnormal"):
                for qj, v in zip(qv, row[side]):
                    w.writerow([service, rank, side, int(row["n_" + side]), float(qj), float(v)])


def _write_kinds(top_list, score_list, rows):
    """kinds.csv beside result.csv: the whole window's block first (``result`` = ``*``), then for each op
    of result.csv, in its order, the op's trace kinds in answer order (rows: window_kinds' dict)."""
    with open("kinds.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "trace", "n_abnormal", "n_normal", "spans", "ops"])
        for label, key in [("*", None)] + [(service, service) for service, _ in _ranked(top_list, score_list)]:
            if key not in rows:
                continue
            for rank, e in enumerate(rows[key][0], start=1):
                w.writerow([label, rank, e[0], int(e[1]), int(e[2]), int(e[3]), int(e[4])])


def _write_calls(top_list, score_list, rows):
    """calls.csv beside result.csv: for each op of result.csv, in its order, its callers and then its
    callees in answer order (rows: window_calls' dict).  A mean is dsum / calls in float64 (0.0 for no
    calls); means and maxima in the SLO's unit and rounding, as latency.csv's values."""
    with open("calls.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "direction", "peer", "calls_abnormal", "calls_normal", "mean_abnormal",
                    "mean_normal", "max_abnormal", "max_normal"])
        for service, _ in _ranked(top_list, score_list):
            if service not in rows:
                continue
            for direction, side in zip(("caller", "callee"), rows[service]):
                for rank, e in enumerate(side[0], start=1):
                    w.writerow([service, rank, direction, e[0], int(e[1]), int(e[2])] + _mean_max(e[1:3], e[3:5], e[5:7]))


def _write_timeline(top_list, score_list, rows):
    """timeline.csv beside result.csv: the window's own block first (``result`` = ``*``, rank 0), then for
    each op of result.csv, in its order, one row per time bucket (rows: window_timeline's dict): the
    bucket's first ns, the rows (for ``*``: traces) that start in it on each side of the detector's
    partition, and the mean and the largest of their values.  A mean is sum / count in float64 (0.0 for
    no rows); means and maxima in the SLO's unit and rounding, as calls.csv's."""
    with open("timeline.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "bucket", "start", "count_abnormal", "count_normal", "mean_abnormal", "mean_normal",
                    "max_abnormal", "max_normal"])
        for rank, (label, key) in enumerate([("*", -1)] + [(service, service) for service, _ in _ranked(top_list, score_list)]):
            r = rows.get(key)
            if r is None:
                continue
            for b, (start, cnt, tot, mx) in enumerate(zip(r["start"], r["cnt"], r["sum"], r["max"])):   # ([normal, abnormal])
                w.writerow([label, rank, b, int(start), int(cnt[1]), int(cnt[0])] + _mean_max(cnt[::-1], tot[::-1], mx[::-1]))
    if any("quantile" in r for r in rows.values()):
        _write_timeline_q(top_list, score_list, rows)


def _write_timeline_q(top_list, score_list, rows):
    """timeline_q.csv beside timeline.csv, from rows that carry quantiles (window_timeline's with q): the window's
    own block first (``result`` = ``*``, rank 0), then each op of result.csv, in its order; per time bucket the
    normal and then the abnormal side, one row per q: ``spans`` the rows (for ``*``: traces) that start in the
    bucket on that side and ``value`` the q-quantile of their values, in the SLO's unit and rounding as
    latency.csv's (0.0 for no rows).  Every bucket is written."""
    with open("timeline_q.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "bucket", "start", "side", "spans", "q", "value"])
        for rank, (label, key) in enumerate([("*", -1)] + [(service, service) for service, _ in _ranked(top_list, score_list)]):
            r = rows.get(key)
            if r is None or "quantile" not in r:
                continue
            for b, (start, cnt, quant) in enumerate(zip(r["start"], r["cnt"], r["quantile"])):   # ([normal, abnormal])
                for side, name in enumerate(("normal", "abnormal")):
                    for qj, v in zip(r["q"], _latency_ms(quant[side])):
                        w.writerow([label, rank, b, int(start), name, int(cnt[side]), float(qj), float(v)])


def _write_replicas(top_list, score_list, rows):
    """replicas.csv beside result.csv: for each op of result.csv, in its order, the listed replicas of its
    service-op in answer order (rows: window_replicas' dict), one row per replica: its rows on each side of
    the detector's partition, the mean and the largest of their values, then the op's live replicas and the
    replicas the table knows.  ``is_result`` is 1 on the row of the ranked pod-op itself.  A mean is sum /
    count in float64 (0.0 for no rows); means and maxima in the SLO's unit and rounding, as calls.csv's."""
    with open("replicas.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "pod", "is_result", "count_abnormal", "count_normal", "mean_abnormal", "mean_normal",
                    "max_abnormal", "max_normal", "live", "replicas"])
        for service, _ in _ranked(top_list, score_list):
            r = rows.get(service)
            if r is None:
                continue
            for rank, e in enumerate(r["entries"], start=1):
                w.writerow([service, rank, e[0], int(e[0] == service), int(e[1]), int(e[2])] +
                           _mean_max(e[1:3], e[3:5], e[5:7]) + [int(r["live"]), int(r["all"])])


def _write_endpoints(top_list, score_list, rows):
    """endpoints.csv beside result.csv: the whole window's block first (``result`` = ``*``, rank 0), then for each
    op of result.csv, in its order, the listed endpoints in answer order (rows: window_endpoints' dict), one row
    per endpoint: the traces that enter there on each side of the detector's partition, the mean and the largest
    of their endTime - startTime, then the slot's live endpoints.  The traces without a root row are written as
    ``(none)``.  A mean is sum / count in float64 (0.0 for no traces); means and maxima in the SLO's unit and
    rounding, as calls.csv's."""
    with open("endpoints.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["result", "rank", "endpoint", "traces_abnormal", "traces_normal", "mean_abnormal", "mean_normal",
                    "max_abnormal", "max_normal", "live"])
        for rank, (label, key) in enumerate([("*", None)] + [(service, service) for service, _ in _ranked(top_list, score_list)]):
            r = rows.get(key)
            if r is None:
                continue
            for e in r["entries"]:
                w.writerow([label, rank, "(none)" if e[0] is None else e[0], int(e[1]), int(e[2])] +
                           _mean_max(e[1:3], e[3:5], e[5:7]) + [int(r["live"])])


# ------------------------------------------------------------------------------------------- the table
@dataclass(frozen=True)
class Kind:
    """One evidence kind, as the drivers see it.  ``check`` turns the keyword's value into the parameters
    (a dict of keywords) that both ``batch`` (windows_*: many windows, pod-op codes) and ``window`` (one
    window by names) take; ``lead`` is the pseudo-op asked in front of a window's top list; ``row`` maps a
    slot of the batch answer (table, slot) to what ``window`` gives for an op, and ``write`` puts such rows
    into the kind's file.  ``head`` names a parameter that the sweep plan keeps ahead of its answers and that
    the writer takes after the rows (latency's q).  ``quantiles``: the (batch, window) forms that take the
    parameters when an option of the keyword put a "q" among them (timeline_q), where the kind has such forms.
    ``variants``: {by: (key, batch, window, row, write)}, the forms that take the parameters when an option of the
    keyword put that "by" among them (kind_by); "by" chooses only, ``kwargs`` drops it from the call."""
    keyword: str
    key: str
    check: Callable
    lead: tuple
    batch: Callable
    window: Callable
    row: Callable
    write: Callable
    head: str | None = None
    quantiles: tuple | None = None
    variants: dict | MappingProxyType | None = None

    def _form(self, params):
        """(key, batch, window, row, write) of the forms that take ``params``: the kind's own; its ``quantiles``
        forms with a "q" among them; the ``variants`` record of their "by" (a second grouping of the kind, chosen
        by an option of the keyword: {by: (key, batch, window, row, write)})."""
        if self.variants is not None and params.get("by") in self.variants:
            return self.variants[params["by"]]
        if self.quantiles is not None and "q" in params:
            return (self.key,) + tuple(self.quantiles) + (self.row, self.write)
        return self.key, self.batch, self.window, self.row, self.write

    @property
    def keys(self):
        """Every key the kind's forms leave an answer under."""
        return (self.key,) + tuple(v[0] for v in (self.variants or {}).values())

    def key_for(self, params):
        """The key of the answer (and the stem of the file) of the form that takes ``params``."""
        return self._form(params)[0]

    def batch_for(self, params):
        """The batch entry that takes ``params``."""
        return self._form(params)[1]

    def window_for(self, params):
        """The one-window form that takes ``params``."""
        return self._form(params)[2]

    def kwargs(self, params):
        """``params`` as the keywords of batch_for / window_for: without "by", which only chooses the form."""
        return {k: v for k, v in params.items() if k != "by"}

    def names(self, table, rows, params=MappingProxyType({})):
        """One window's batch answer {code: slot} as the writer's rows: by pod-op name where the table has names
        (the lead ops None and -1 stay), each slot through the form's ``row``."""
        names, row = table.podop_names, self._form(params)[3]
        return {(c if c is None or c < 0 or names is None else names[c]): row(table, r) for c, r in rows.items()}

    def plan_value(self, params, by_m):
        """What sweep_rank leaves in the plan under ``key``: the answers {m: the batch's dict}."""
        return by_m if self.head is None else (params[self.head], by_m)

    def answers(self, value):
        """plan_value's {m: ...}."""
        return value if self.head is None else value[1]

    def file(self, top_list, score_list, rows, params):
        """Rewrite the kind's file beside result.csv."""
        self._form(params)[4](top_list, score_list, rows, *(() if self.head is None else (params[self.head],)))


KINDS = (
    Kind("latency", "latency", lambda v: {"q": _latency_args(*v)[0], "what": v[1]}, (), windows_latency, op_latency,
         _latency_row, _write_latency, head="q"),   # (its value: the pair (latency, latency_what))
    Kind("kind_breakdown", "kinds", _kind_params, (None,), windows_kind_breakdown, window_kinds, _kind_row, _write_kinds,
         variants=MappingProxyType({"endpoint": ("endpoints", windows_endpoints, window_endpoints, _endpoint_row,
                                                 _write_endpoints)})),
    # (its value: the keyword, or a _KindAsk with kind_by)
    Kind("call_edges", "calls", lambda m: {"m": _call_m(m)}, (), windows_call_edges, window_calls, _call_row,
         _write_calls),
    Kind("timeline", "timeline", _timeline_params, (-1,), windows_timeline, window_timeline, _timeline_row,
         _write_timeline, quantiles=(windows_timeline_q, window_timeline_q)),   # (its value: the keyword, or a
    # _TimelineAsk with timeline_q / timeline_what)
    Kind("replicas", "replicas", lambda m: {"m": _replica_args(m)[0]}, (), windows_replicas, window_replicas,
         _replica_row, _write_replicas),
)


class Evidence(NamedTuple):
    """What a caller asked beside the ranking: the exemplar keywords, and the asked kinds of KINDS, in its
    order, each with its checked parameters -- ((Kind, read-only dict), ...)."""
    exemplars: int | None = None
    exemplar_kinds: bool = False
    kinds: tuple = ()


NOTHING = Evidence()


def evidence_request(*, exemplars=None, exemplar_kinds=False, latency=None, latency_what="self", kind_breakdown=None,
                     call_edges=None, timeline=None, replicas=None, timeline_q=None, timeline_what="self", kind_by="kind"):
    """The drivers' evidence keywords (online_anomaly_detect_RCA's docstring has each) checked into one
    Evidence; ValueError for a bad one, before any device work.  None means "not asked".  timeline_q and
    timeline_what are options of the timeline kind: its parameters are {"buckets": B} without them.  kind_by is an
    option of the kind_breakdown kind: "kind" leaves its parameters {"m": m}, "endpoint" makes them {"m": m, "by":
    "endpoint"} -- the window's traces grouped by entry operation (windows_endpoints, endpoints.csv) in place of
    the trace kinds."""
    exemplar_kinds = check_exemplar_kinds(exemplar_kinds, exemplars)
    if exemplars is not None:
        exemplars = check_exemplar_m(exemplars)
    _what_code(timeline_what)
    if not isinstance(kind_by, str) or kind_by not in ("kind", "endpoint"):
        raise ValueError(f"kind_by must be 'kind' or 'endpoint', not {kind_by!r}")
    if kind_by != "kind":
        if kind_breakdown is None:
            raise ValueError("kind_by needs kind_breakdown (the entries per op)")
        kind_breakdown = _KindAsk(kind_breakdown, kind_by)
    if timeline_q is not None and timeline is None:
        raise ValueError("timeline_q needs timeline (the number of time buckets)")
    if timeline is not None and (timeline_q is not None or timeline_what != "self"):
        timeline = _TimelineAsk(timeline, timeline_q, timeline_what)
    values = {"latency": None if latency is None else (latency, latency_what), "kind_breakdown": kind_breakdown,
              "call_edges": call_edges, "timeline": timeline, "replicas": replicas}
    kinds = tuple((k, MappingProxyType(k.check(values[k.keyword]))) for k in KINDS if values.get(k.keyword) is not None)
    if exemplars is None and not kinds:
        return NOTHING
    return Evidence(exemplars, exemplar_kinds, kinds)
