"""Reference for the one-exemplar-per-trace-kind tests (MR_EX_DISTINCT_KINDS): the kind of every trace
as pagerank.py:54-66 classes them, and numpy's selection of one trace per kind."""
import numpy as np


def kind_ids(g):
    """kid[t]: an id per exact class of (sorted op set of the trace's P_sr column, fp32(1/len_t) bits; 0
    for a trace without ops) -- orc.trace_kinds' key, so np.bincount(kid)[kid] is orc.trace_kinds(g)."""
    w = (1.0 / np.maximum(g.len_t, 1)).astype(np.float32)
    order = np.lexsort((g.sr_o, g.sr_t))
    sets = [[] for _ in range(g.T)]
    for t, o in zip(np.asarray(g.sr_t)[order].tolist(), np.asarray(g.sr_o)[order].tolist()):
        sets[t].append(o)
    keys = {}
    kid = np.empty(g.T, np.int64)
    for t in range(g.T):
        key = (tuple(sets[t]), w[t].view(np.uint32).item() if sets[t] else 0)
        kid[t] = keys.setdefault(key, len(keys))
    return kid


def distinct_top(row, r, kid, m):
    """The first min(m, kinds in the row) representatives of an op's P_sr row: the row sorted by score
    descending, index ascending on ties, the first trace of each kind kept."""
    row = np.asarray(row, np.int64)
    order = row[np.lexsort((row, -r[row]))]
    seen, out = set(), []
    for t in order.tolist():
        k = int(kid[t])
        if k in seen:
            continue
        seen.add(k)
        out.append(t)
        if len(out) == m:
            break
    return np.asarray(out, np.int64)


def kinds_in_row(row, kid):
    return int(np.unique(kid[np.asarray(row, np.int64)]).size)
