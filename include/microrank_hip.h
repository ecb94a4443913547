/*
 * microrank_hip.h -- C-ABI of libmicrorank_hip.so, the MI355X (gfx950) implementation of
 * MicroRank's ranking hot path.  Plain pointers and sizes only; every entry point returns
 * an MR_* status (0 = ok) and mr_last_error(ctx) describes the failure.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * CUHK-SE-Group/MicroRank @ 2025-02-14).  The Python drop-in modules in
 * microrank_amd/ (pagerank.py, preprocess_data.py, anormaly_detector.py, online_rca.py)
 * bind these with ctypes; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - "host" pointers are caller-owned CPU memory, copied in/out inside the call.
 *   - "device" handles (mr_graph, mr_spans) own HBM; they belong to one mr_ctx.
 *   - Node order, trace order and every tie-break follow the reference.
 *   - Calls on distinct contexts are thread-safe; one context is not re-entrant.
 */
#ifndef MICRORANK_HIP_H
#define MICRORANK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the Python layer maps them onto the reference's exception types) ---- */
enum {
    MR_OK = 0,
    MR_ERR_ARG = 1,       /* bad argument / shape                        -> ValueError/TypeError */
    MR_ERR_HIP = 2,       /* HIP runtime failure                          -> RuntimeError */
    MR_ERR_VALUE = 3,     /* reference raises ValueError (empty graph, list.index miss) */
    MR_ERR_ZERODIV = 4,   /* reference raises ZeroDivisionError (1.0/len of an empty pr list) */
    MR_ERR_OOM = 5,       /* device allocation failed */
    MR_ERR_COMM = 6,      /* RCCL failure */
    MR_ERR_STATE = 7      /* handle used with the wrong context / before setup */
};

enum { MR_FP64 = 0, MR_FP32 = 1 };      /* precision of the rank vectors */

/* mr_pagerank flags */
enum {
    MR_PR_EXACT_SUMS = 1u,  /* sequential fp64 sums in reference order for the one-time scalars
                               (pagerank.py:71-78, 95-96; T7) instead of a fixed-order tree */
    MR_PR_KIND_COMPRESS = 2u /* mr_pagerank only: iterate over one
                               representative trace per kind with its multiplicity -- traces of
                               one kind (pagerank.py:54-66) have identical r; same weights
                               within fp64 rounding, work proportional to the kinds */
};

typedef struct mr_ctx mr_ctx;
typedef struct mr_graph mr_graph;
typedef struct mr_spans mr_spans;

/* ------------------------------------------------------------------ context */
int         mr_version(void);
int         mr_device_count(int* n);
int         mr_ctx_create(int device, uint32_t flags, mr_ctx** out);
void        mr_ctx_destroy(mr_ctx* ctx);
const char* mr_last_error(const mr_ctx* ctx);
int         mr_ctx_sync(mr_ctx* ctx);
/* stream the context launches on (a hipStream_t), for callers that time with HIP events */
void*       mr_ctx_stream(mr_ctx* ctx);
/* live timing of the power-iteration kernel: while enabled every launch is bracketed by HIP
 * events on the context stream; mr_ctx_prof_read syncs, returns the number of ITERATIONS the
 * recorded launches covered (one per launch pair; all of a call's for a persistent k_pr_cluster
 * launch), the summed kernel time and the summed algorithmic bytes (SURVEY §8(d) B_iter), and
 * clears the record */
int         mr_ctx_profile(mr_ctx* ctx, int enable);
int         mr_ctx_prof_read(mr_ctx* ctx, int64_t* launches, double* total_ms, double* total_bytes);
/* the device's measured copy peak (the HBM roofline is also reported against a
 * measured STREAM-copy rate beside the 8 TB/s spec): 16-B-per-lane copy kernels (grid-stride
 * and block-tile shapes, plain and non-temporal) over two buffers of `bytes` each on the context
 * stream, per shape one warm-up and `reps` timed launches; *gbs = the best launch's (read +
 * written) bytes / time in GB/s.  No reference counterpart (measurement) */
int         mr_copy_peak(mr_ctx* ctx, int64_t bytes, int reps, double* gbs);

/* ------------------------------------------------------------------ graph from index arrays
 * Replaces the dense matrix fill of pagerank.trace_pagerank (pagerank.py:16-52): the four
 * dicts become incidence lists.  Node ids follow the operation_operation key order, trace
 * ids the operation_trace key order.
 */
typedef struct mr_graph_desc {
    int32_t n_nodes;          /* N = len(operation_operation)                        */
    int32_t n_traces;         /* T = len(operation_trace)                            */
    int64_t nnz_sr;           /* distinct (trace, op) pairs of P_sr                  */
    const int64_t* sr_off;    /* [T+1] trace-major P_sr incidence (op in operation_trace[t]) */
    const int32_t* sr_ops;    /* [nnz_sr] node ids, ascending within a trace          */
    int64_t nnz_rs;           /* distinct pairs of P_rs; 0 with rs_* NULL = same as sr */
    const int64_t* rs_off;    /* [T+1] trace-major P_rs incidence (t in trace_operation[o]) */
    const int32_t* rs_ops;
    const int32_t* len_t;     /* [T] len(operation_trace[t])  -> P_sr value fp32(1/len_t) */
    const int32_t* len_o;     /* [N] len(trace_operation[o])  -> P_rs value fp32(1/len_o) */
    int64_t n_edges;          /* distinct (child, parent) pairs of P_ss               */
    const int64_t* ss_off;    /* [N+1] by child                                       */
    const int32_t* ss_par;    /* [n_edges] parent node ids, ascending within a child   */
    const int32_t* nchild;    /* [N] len(operation_operation[p]) -> P_ss value fp32(1/nchild) */
    int32_t n_pr;             /* len(pr_trace)                                        */
    const int32_t* pr_trace;  /* [n_pr] trace id of each pr_trace key, in pr_trace order */
    const int32_t* pr_len;    /* [n_pr] len(pr_trace[key])                            */
} mr_graph_desc;

int mr_graph_upload(mr_ctx* ctx, const mr_graph_desc* desc, mr_graph** out);
int mr_graph_free(mr_graph* g);
int mr_graph_info(const mr_graph* g, int32_t* n_nodes, int32_t* n_traces, int64_t* nnz,
                  int64_t* n_edges);

/* ------------------------------------------------------------------ K2: personalised PageRank
 * pagerank.trace_pagerank (pagerank.py:15-112) + pageRank (pagerank.py:116-130):
 * kinds (:54-66), preference vector (:68-85), `iters` Jacobi power iterations with max
 * normalisation (:121-129), weight = s*sum(s)/N and trace coverage (:93-107).
 * Results stay on the device; mr_graph_fetch copies them out.
 */
int mr_pagerank(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters,
                int precision, uint32_t flags);
/* mr_pagerank with the anomaly preference's weight phi exposed (the 0.5 at both places of
 * pagerank.py:82-84; SURVEY §5 config defaults: d = 0.85, alpha = 0.01 at :116, iters = 25 at
 * :117, phi = 0.5).  mr_pagerank is mr_pagerank_ex with phi = 0.5. */
int mr_pagerank_ex(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters, double phi,
                   int precision, uint32_t flags);
/* several independent graphs (e.g. the normal and anomaly graphs of a window, or many windows)
 * ranked together: one launch per Jacobi iteration covers every graph */
int mr_pagerank_batch(mr_ctx* ctx, mr_graph* const* graphs, const int* anomaly, int n_graphs, double d,
                      double alpha, int iters, int precision, uint32_t flags);
/* mr_pagerank_batch with a convergence report and an optional early stop.  The reference iterates
 * a fixed 25 times (pagerank.py:117) and its README's production notices say a large system
 * "needs more iterations in PageRank" (README.md:37); nothing there says whether a count was
 * enough.  After every iteration k = 1, 2, ... the device records, per graph,
 *   resid[k-1] = max over ops of | s_k - s_{k-1} |,
 * s_k the max-normalised vector the reference holds in `s` after k iterations (pagerank.py:126;
 * s_0 = 1/(N+T), :118).  Every check_every iterations, and at max_iters, the host reads the
 * history and stops at the first such check K where every graph's resid[K-1] <= tol.  tol == 0:
 * no intermediate reads, the call runs max_iters iterations and reads the history once.
 * phi as mr_pagerank_ex's.  fp32 residuals bottom out near 6e-8 (one fp32 ulp of a vector whose
 * maximum is 1): a smaller tol with MR_FP32 runs to max_iters.
 * Contract: after a call that ran K = *iters_done iterations, every graph's weights and coverage
 * (mr_graph_fetch) are bitwise those of mr_pagerank_batch(..., iters = K, ...) on the same graphs.
 * MR_ERR_ARG: null pointers (converged_at may be NULL), n_graphs < 1, max_iters < 1,
 * check_every < 1, tol negative or NaN, phi <= 0 -- and the two forms this entry does not cover:
 * MR_PR_KIND_COMPRESS and a graph built by mr_graph_build_sharded (an early stop must be agreed
 * over the ranks: mr_pagerank_sharded_converge does; mr_pagerank_sharded takes a count).  Window batches build their graphs inside
 * the call, so they have entries of their own: mr_windows_batch_ex and mr_rca_window_ex take a
 * count, report the last iteration's residual and stop at a tolerance.  Everything else as
 * mr_pagerank_batch: its errors, the kind-hash collision retry (which reruns the attempt and
 * overwrites the history), mr_graph_fetch afterwards. */
int mr_pagerank_converge(mr_ctx* ctx, mr_graph* const* graphs, const int* anomaly, int n_graphs,
                         double d, double alpha, int max_iters, double phi, int precision, uint32_t flags,
                         double tol, int check_every,
                         int32_t* iters_done,              /* out: iterations every graph ran */
                         double* resid,                    /* [n_graphs * max_iters] host; graph g's history at
                                                              g * max_iters; entries >= iters_done are 0.0 */
                         int32_t* converged_at);           /* [n_graphs] host: first k (1-based) with
                                                              resid[k-1] <= tol, -1 if none; may be NULL */
int mr_graph_fetch(mr_graph* g, double* weight /*[N] host*/, int32_t* coverage /*[N] host*/,
                   double* kind /*[T] host or NULL*/, float* pref /*[T] host or NULL*/);
/* The trace half of the last ranking.  pageRank carries two vectors (pagerank.py:119-127): the
 * operation vector becomes the weights, the trace vector is request_ranking_vector -- how much each
 * trace matters under the same personalisation; the reference drops it at :130.
 * mr_graph_trace_rank: r[t] = the max-normalised value the reference holds in
 * request_ranking_vector[t] after the K iterations of the graph's last successful ranking
 * (mr_pagerank, _ex, _batch; mr_pagerank_converge: the iterations it ran), in the graph's trace
 * order (mr_graph_nodes' trace_code order, or the uploaded operation_trace order).  fp64 in both
 * precisions; K = 0 gives 1/(N+T) for every trace (:119, un-normalised, as the reference holds it).
 * mr_graph_exemplars: for each asked node index ops[i] the m traces with the largest r among the
 * traces of that op's P_sr row (operation_trace, the relation `coverage` counts; pagerank.py:42-45),
 * score descending, trace index ascending on equal values.  out_n[i] = min(m, coverage[ops[i]]);
 * the rest of row i is padded with -1 / 0.0.  A duplicated op is answered each time.
 * MR_ERR_ARG: null pointers, n_ops outside 1..64, m outside 1..32, an op outside [0, N).
 * MR_ERR_STATE: no ranking yet (or its state re-set since); the last ranking was asked with
 * MR_PR_KIND_COMPRESS (the trace vector then lives on the representatives' graph); a trace shard
 * (mr_graph_build_sharded / mr_pagerank_sharded: each rank holds only its own traces;
 * mr_graph_trace_rank_sharded and mr_graph_exemplars_sharded answer a shard). */
int mr_graph_trace_rank(mr_graph* g, double* r /*[T] host*/);
int mr_graph_exemplars(mr_graph* g, const int32_t* ops, int32_t n_ops, int32_t m,
                       int32_t* out_trace /*[n_ops*m] trace indices, -1 padded*/,
                       double* out_score /*[n_ops*m], 0.0 padded*/, int32_t* out_n /*[n_ops]*/);
/* mr_graph_exemplars with flags.  flags == 0 and out_mult == NULL is mr_graph_exemplars itself: the
 * same launches and the same read-back (mr_graph_exemplars(...) is mr_graph_exemplars_ex(..., 0, ...,
 * NULL)).  MR_EX_DISTINCT_KINDS: ONE trace per trace kind.  The kinds are the exact classes of
 * pagerank.py:54-66 that the ranking's own set-up uses (equal operation set and equal fp32(1/len_t);
 * exact classes, not a hash), so a kind lies wholly inside an op's P_sr row or wholly outside it.
 * Each kind of the row is represented by its best member under mr_graph_exemplars' order (score bits
 * descending, trace index ascending); the answer is the first min(m, kinds in the row)
 * representatives in that same order, out_n[i] that count.  Kinds are told apart by identity, never
 * by score: where P_rs is given apart from P_sr the members of one kind have different scores.
 * Entry 0 is mr_graph_exemplars' entry 0; a row of singleton kinds is answered as without the flag;
 * the answer does not depend on how the traces are cut into blocks.  K = 0: every kind by its
 * smallest trace index, in index order.
 * out_mult[i*m + j]: the class size of entry j, the number of traces of that kind in the graph -- the
 * value mr_graph_fetch returns in kind[trace]; 0 padded.  May be NULL.
 * The first call with the flag after a graph's first ranking computes the kinds' representatives once
 * (they depend on the structure alone); it leaves mr_graph_fetch, mr_graph_trace_rank, the plain
 * entry and the next ranking bitwise what they were.
 * MR_ERR_ARG: a flag bit other than MR_EX_DISTINCT_KINDS, out_mult with flags == 0, and everything
 * mr_graph_exemplars rejects.  MR_ERR_STATE: as mr_graph_exemplars (no ranking yet,
 * MR_PR_KIND_COMPRESS, a trace shard: mr_graph_exemplars_sharded has no distinct-kinds form). */
enum { MR_EX_DISTINCT_KINDS = 1u };
int mr_graph_exemplars_ex(mr_graph* g, const int32_t* ops, int32_t n_ops, int32_t m, uint32_t flags,
                          int32_t* out_trace, double* out_score, int32_t* out_n,
                          int32_t* out_mult /* [n_ops*m] or NULL */);

/* ------------------------------------------------------------------ spans (int-coded columns)
 * The DataFrame of online_rca.py:221-248 after factorisation (microrank_amd/spans.py).
 */
typedef struct mr_span_cols {
    int64_t n_spans;
    int32_t n_traces, n_podops, n_svcops;
    const int32_t* trace;     /* trace code (rank of traceID in sorted order)       */
    const int32_t* podop;     /* podName_op code (sorted name order)                */
    const int32_t* svcop;     /* serviceName_op code (sorted name order)            */
    const int64_t* span;      /* spanID code                                        */
    const int64_t* parent;    /* ParentSpanId as a spanID code, -1 if absent        */
    const int64_t* duration;  /* span duration (reference units)                   */
    const int64_t* tstart;    /* trace-level start, ns (NULL if absent)             */
    const int64_t* tend;      /* trace-level end, ns                                */
    const int32_t* row;       /* global row index (NULL: the rows are the whole table) --
                                 a shard of a table split over ranks keeps the table's
                                 row order here for first appearance (T10)           */
} mr_span_cols;

int mr_spans_upload(mr_ctx* ctx, const mr_span_cols* cols, mr_spans** out);
int mr_spans_free(mr_spans* s);

/* SURVEY §8(f) f2 -- span ingest on the device from the string columns of the OTel export
 * (collect_data.py:35-46, renamed at online_rca.py:221-244).  A string column is Arrow-style:
 * value i = bytes[offsets[i] .. offsets[i+1]); valid is an Arrow validity bitmap (bit i of byte
 * i/8, 1 = present) or NULL (no nulls) -- only ParentSpanId may have nulls (a root span).
 * Produces the same table mr_spans_upload would get from SpanTable.from_dataframe: traceID,
 * podName_op and serviceName_op codes in sorted (code-point) name order, op = operationName with
 * ts-ui-dashboard's last '/segment' dropped (preprocess_data.py:26-33, 151-155), ParentSpanId
 * resolved to the equal spanID's code or -1.  Replaces the per-function string work of
 * preprocess_data.py (:26-33, 53-57, 100-104, 151-165). */
typedef struct mr_str_col {
    const int64_t* offsets;   /* [n_spans + 1] */
    const uint8_t* bytes;
    const uint8_t* valid;     /* Arrow bitmap or NULL */
} mr_str_col;
typedef struct mr_span_strings {
    int64_t n_spans;
    mr_str_col trace_id, span_id, parent_id, service, operation, pod;
    const int64_t* duration;  /* [n_spans] */
    const int64_t* tstart;    /* [n_spans] trace-level start, ns (NULL if absent) */
    const int64_t* tend;
} mr_span_strings;
int mr_spans_ingest(mr_ctx* ctx, const mr_span_strings* cols, mr_spans** out);
int mr_spans_info(const mr_spans* s, int64_t* n_spans, int32_t* n_traces, int32_t* n_podops, int32_t* n_svcops);
/* first row of each code in code order, which 0 trace / 1 pod-op / 2 service-op (ingested tables):
 * name of code k = that row's traceID / podName_op / serviceName_op */
int mr_spans_dict_rows(const mr_spans* s, int which, int32_t* rows);
/* SURVEY 8(f) f3, streaming: a new table = the rows of `prev` whose trace-level start is >=
 * keep_from (ns), in their order, then the chunk's rows -- the same table mr_spans_ingest builds
 * from those rows' strings.  The string columns stay on the device, so only the chunk crosses
 * PCIe (the resident rows are gathered device to device and re-coded there).  prev: NULL (the
 * first chunk) or a table this function returned on the same context; it stays valid (free it
 * with mr_spans_free).  The chunk needs tstart / tend.  Replaces the reference's per-window
 * re-read of the whole span frame (online_rca.py:161-216 over preprocess_data.get_span, :10-14). */
int mr_spans_append(mr_ctx* ctx, const mr_spans* prev, int64_t keep_from, const mr_span_strings* chunk,
                    mr_spans** out);
/* tables from mr_spans_append: the stream row number (position in the concatenation of every
 * chunk appended so far) of each code's first row, in code order -- mr_spans_dict_rows in stream
 * terms, so the host can read names from the chunk that holds the row */
int mr_spans_dict_sources(const mr_spans* s, int which, int64_t* src);
/* the code columns of a table (any pointer may be NULL), [n_spans] each */
int mr_spans_codes(const mr_spans* s, int32_t* trace, int32_t* podop, int32_t* svcop, int64_t* span,
                   int64_t* parent);

/* K1: preprocess_data.get_pagerank_graph (preprocess_data.py:146-171) on the device.
 * trace_mask[n_traces] (host, 0/1) selects the trace_list.  Node order = sorted parent ops,
 * then never-parent ops in first-appearance row order (T10).  The parent join ignores
 * traceID (T11). */
int mr_graph_build(mr_ctx* ctx, const mr_spans* s, const uint8_t* trace_mask, mr_graph** out);
/* K1 over a trace-sharded span table (one process per GPU, every span of a trace on one
 * rank, span / pod-op / trace codes global, cols.row set): this rank's graph over the GLOBAL
 * node order -- pod-op counts, first appearances and parent flags reduced over the ranks
 * (preprocess_data.py:159-163, T10), and the ParentSpanId == spanID join resolved across ranks
 * too (:157-158, T11: a child's parent rows may lie in traces of another rank).  len_o, nchild
 * and the call edges stay this rank's parts: mr_pagerank_sharded combines them.  Collectives
 * over the context's backend (mr_comm_init / mr_comm_set_host); replaces the per-rank
 * get_pagerank_graph(trace_list, span_df) of a sharded deployment. */
int mr_graph_build_sharded(mr_ctx* ctx, const mr_spans* s, const uint8_t* trace_mask, mr_graph** out);
/* node order (podop codes) and trace codes of a built graph */
int mr_graph_nodes(const mr_graph* g, int32_t* node_podop /*[N]*/, int32_t* trace_code /*[T]*/);
/* structure export for parity tests: any pointer may be NULL */
int mr_graph_export(const mr_graph* g, int64_t* sr_off /*[T+1]*/, int32_t* sr_ops /*[nnz]*/,
                    int32_t* len_t /*[T]*/, int32_t* len_o /*[N]*/, int64_t* ss_off /*[N+1]*/,
                    int32_t* ss_par /*[E]*/, int32_t* nchild /*[N]*/);

/* ------------------------------------------------------------------ K3: spectrum + top-k
 * online_rca.calculate_spectrum_without_delay_list (online_rca.py:33-152).  Inputs are in the
 * reference's iteration order: the anomaly_result nodes first, then normal-only nodes.
 * has_a/has_n mark membership; method is an index into
 * {dstar2, ochiai, jaccard, sorensendice, m1, m2, goodman, tarantula, russellrao, hamann,
 *  dice, simplematcing, rogers}.  Output: the first min(n, top) indices of the stable
 * descending sort and their scores.  A division by zero sets *zerodiv (the reference
 * raises ZeroDivisionError). */
int mr_spectrum(mr_ctx* ctx, int32_t n, const uint8_t* has_a, const double* a_w, const int64_t* a_num,
                const uint8_t* has_n, const double* n_w, const int64_t* n_num, int64_t a_len,
                int64_t n_len, int method, int32_t top, int32_t* out_idx, double* out_score,
                int32_t* n_out, int32_t* zerodiv);

/* ------------------------------------------------------------------ K4: SLO
 * preprocess_data.get_operation_slo (preprocess_data.py:50-78), the semantic body of the
 * broken anormaly_detector.get_slo (anormaly_detector.py:22-27, T16): per svcop code,
 * round(mean/1000, 4) and round(std/1000, 4) (population std, numpy pairwise order, T13).
 * count[o] = 0 marks an op with no spans. */
int mr_slo(mr_ctx* ctx, const mr_spans* s, double* mean /*[n_svcops]*/, double* std_ /*[n_svcops]*/,
           int64_t* count /*[n_svcops]*/);

/* K4, percentile form: per service-op code, the q[j]-quantiles of the span durations, with
 * numpy.quantile's semantics (bit for bit on int64 durations).  No reference counterpart: extends
 * preprocess_data.get_operation_slo (preprocess_data.py:50-78) so that the detector's per-op
 * expectation can be a p99 instead of mean + 3*std (a percentile SLO is handed on as [Q, 0.0]).
 * Rows: all of the table when t0 == INT64_MIN and t1 == INT64_MAX, otherwise the rows with
 * tstart >= t0 && tend <= t1 (mr_detect's inclusive window); a window on a table uploaded
 * without trace-level times returns MR_ERR_STATE.
 * method: numpy's method= names.  With n rows of an op sorted ascending as a[0..n) and
 * vi = (double)(n-1) * q:  LOWER a[floor(vi)], HIGHER a[ceil(vi)], LINEAR numpy's _lerp between
 * a[floor(vi)] and its successor with g = vi - floor(vi) (taken from the upper end for g >= 0.5).
 * out[o * n_q + j] is in duration units, not scaled and not rounded; count[o] = rows of op o that
 * took part; count 0 gives out = 0.0, as mr_slo does.
 * MR_ERR_ARG: null pointers, n_q < 1, an unknown method, a q[j] that is NaN or outside [0, 1], s of
 * another context, or a duration range too wide to sort: grouping and ordering are ONE sort of
 * keys (op << DB) | (duration - min), DB = bits of (max - min) over the rows that take part, and
 * bits(n_svcops) + DB must not exceed 64 (with 1k ops: a duration spread below 2^54).
 * n_svcops == 0 returns MR_OK and writes nothing; an empty table or a window that selects no row
 * returns MR_OK with every count 0. */
enum { MR_Q_LINEAR = 0, MR_Q_LOWER = 1, MR_Q_HIGHER = 2 };
int mr_slo_quantiles(mr_ctx* ctx, const mr_spans* s, int64_t t0, int64_t t1, const double* q, int32_t n_q,
                     int method, double* out /*[n_svcops * n_q] host*/, int64_t* count /*[n_svcops] host*/);

/* ------------------------------------------------------------------ K5: detector
 * anormaly_detector.system_anomaly_detect (anormaly_detector.py:44-84) with
 * get_operation_duration_data (preprocess_data.py:97-122): window [t0, t1] on trace-level
 * times (inclusive), real = max duration/1000, expect = sum over ops (sorted order) of
 * count*a3[op] with a3 = mean+3*std, ops without SLO (a3_valid=0) contribute 0.
 * state[n_traces] (host): 0 not in window / dropped, 1 normal, 2 abnormal.
 * Returns MR_ERR_VALUE with *n_spans_in_window = 0 for an empty window (the reference
 * returns False, T2). */
int mr_detect(mr_ctx* ctx, const mr_spans* s, int64_t t0, int64_t t1, const double* a3,
              const uint8_t* a3_valid, uint8_t* state, int32_t* n_abnormal, int32_t* n_normal,
              int64_t* n_spans_in_window);

/* SURVEY §8(f) f3 -- the driver's whole window sweep (online_rca.py:161-216) detected at once:
 * for window m in [0, n_win) = [t_begin + m*grain, t_begin + m*grain + window] the counts of
 * mr_detect (abnormal / normal traces, in-window rows; n_rows[m] = 0 is the reference's empty
 * window, T2).  Needs trace-level times constant within each trace (the renamed TraceStart /
 * TraceEnd columns, online_rca.py:229-230): then a trace's partition does not depend on the window
 * and is computed once; state[n_traces] (host, optional) receives it (0 dropped, 1 normal,
 * 2 abnormal), so window m's lists are the traces of that state inside the window.
 * MR_ERR_STATE when times vary within a trace (run mr_detect per window instead). */
int mr_detect_sweep(mr_ctx* ctx, const mr_spans* s, int64_t t_begin, int64_t grain, int64_t window,
                    int32_t n_win, const double* a3, const uint8_t* a3_valid, uint8_t* state,
                    int32_t* n_abnormal, int32_t* n_normal, int64_t* n_rows);

/* ------------------------------------------------------------------ whole RCA window on device
 * online_rca.online_anomaly_detect_RCA body for one window (online_rca.py:164-215):
 * detect -> (swapped, T1) two graph builds -> two PageRanks -> spectrum -> top list, with
 * all intermediates resident in HBM.  out_idx are podop codes. */
int mr_rca_window(mr_ctx* ctx, const mr_spans* s, int64_t t0, int64_t t1, const double* a3,
                  const uint8_t* a3_valid, int method, int32_t top_max, int precision,
                  int32_t* out_podop, double* out_score, int32_t* n_out, int64_t* edges_traversed,
                  int32_t* n_abnormal, int32_t* n_normal);

/* C3: rank n_windows RCA windows in one call -- each as mr_rca_window.  Window i:
 * spans[i] (a span table of this context; windows may share one), [t0[i], t1[i]], the SLO
 * a3[i] / a3_valid[i] (n_svcops of spans[i]).  The windows' detectors and graph builds run
 * concurrently on auxiliary streams of this context, the PageRanks of all their graphs share
 * each power iteration's launches, then the spectra run concurrently.  Per window i:
 * out_podop / out_score[i * (top_max + 6) ..], n_out[i], edges_traversed[i], n_abnormal[i],
 * n_normal[i], status[i] (MR_OK, or MR_ERR_VALUE for an empty window -- the reference's
 * unpack of False, T2).  Replaces a loop of online_anomaly_detect_RCA windows
 * (online_rca.py:161-216) over independent windows.  Device memory: the graphs of large windows
 * (>= 64k traces on average) stay in the context's pools until the next call on it (released
 * there beside the new builds) or mr_ctx_destroy. */
int mr_windows_batch(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                     const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid, int method,
                     int32_t top_max, int precision, int32_t* out_podop, double* out_score, int32_t* n_out,
                     int64_t* edges_traversed, int32_t* n_abnormal, int32_t* n_normal, int32_t* status);

/* mr_windows_batch with a caller-chosen iteration count, a convergence report per window and an
 * optional stop at a tolerance.  The reference ranks every window with 25 iterations
 * (pagerank.py:117) and its README's production notices say a large system "needs more iterations
 * in PageRank" (README.md:37); mr_windows_batch(...) is mr_windows_batch_ex(..., 25, 0.0, 1, NULL,
 * NULL), launch for launch.  Every argument of mr_windows_batch in its order, then:
 *   iters        tol == 0: every ranked window's two graphs run exactly iters iterations, through
 *                mr_windows_batch's pipeline.  tol > 0: the maximum.
 *   tol          > 0: the graphs of a group of windows (the windows whose PageRanks share launches)
 *                are ranked by mr_pagerank_converge's attempt and stop at the first check -- every
 *                check_every iterations, and at iters -- where every graph of the group is <= tol.
 *                That ranking is synchronous: the next group's iterations no longer queue behind
 *                this group's, and a call of one chunk runs its spectrum after the words are read;
 *                this lost overlap is the price of tol.  With MR_FP32 residuals bottom out near
 *                6e-8: a smaller tol runs to iters.
 *   check_every  tol > 0 only (ignored otherwise, but checked).
 *   iters_done   [n_windows] host or NULL: iterations window i's graphs ran; 0 for a window that
 *                ranked nothing (an empty window, status MR_ERR_VALUE, or a window without abnormal
 *                or without normal traces).  Windows of one group report the same count.
 *   resid        [2 * n_windows] host or NULL: resid[2i] the residual max over ops of
 *                | s_k - s_{k-1} | (mr_pagerank_converge's, k = iters_done[i]) of the last
 *                iteration run by the graph of the detector's abnormal traces (ranked with
 *                anomaly = 0, T1), resid[2i + 1] that of the graph of its normal traces
 *                (anomaly = 1); 0.0 for a window that ranked nothing.
 * edges_traversed[i] counts iters_done[i] iterations.  With both report pointers NULL no residual
 * kernel is launched and nothing extra is copied; with one, a fixed-count call adds one k_resid
 * launch per group behind its last iteration, read with the group's error words.
 * Contract: window i's top list and scores are bitwise those of a fixed-count call (tol = 0) with
 * iters = iters_done[i], whatever the grouping of the windows.  A kind-hash collision rerun keeps
 * iters / tol and overwrites the report.
 * MR_ERR_ARG: iters < 1, check_every < 1, tol negative or NaN, and mr_windows_batch's. */
int mr_windows_batch_ex(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                        const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid, int method,
                        int32_t top_max, int precision, int32_t* out_podop, double* out_score, int32_t* n_out,
                        int64_t* edges_traversed, int32_t* n_abnormal, int32_t* n_normal, int32_t* status,
                        int iters, double tol, int check_every, int32_t* iters_done, double* resid);
/* A test and diagnostic hook, not part of the ranking interface: how the windows of tables with a
 * layout order were built, counted over the process since the library was loaded (process-wide
 * counters; MR_WIN_PHASES prints the same two numbers).  The window build
 * has two forms with the same result: the direct form adds every entry of the window's traces
 * into its two graphs; the complement form takes the larger graph (the detector's normal traces)
 * as the table's totals minus everything else and walks only the other traces' entries.  A table
 * carries what the complement form needs when its index could build it; a window takes that form
 * when the table's time summary says it leaves out at most a quarter of the table's traces.
 * MR_LO_COMPLEMENT (read per call): 0 always direct, 1 complement wherever the table allows.
 *   n_complement  windows launched in the complement form
 *   n_rebuilt     of those, windows built again in the direct form because the table's first-row
 *                 candidates of some op all lay outside the window's normal traces
 * Either pointer may be NULL. */
int mr_lo_complement_counts(int64_t* n_complement, int64_t* n_rebuilt);
/* mr_windows_batch_ex that also says WHICH TRACES: for every op of a window's top list the ex_m
 * traces to open, read from the state the window's ranking leaves on the device before its graphs
 * are released.  Every argument of mr_windows_batch_ex in its order, then:
 *   ex_m       traces per op, 1..32
 *   ex_trace   [n_windows * K * ex_m] host, K = top_max + 6: trace codes of spans[i] (the index of
 *              mr_detect's state[]), -1 padded
 *   ex_score   [n_windows * K * ex_m] host, 0.0 padded
 *   ex_n       [n_windows * K] host
 * Row (i, j) answers out_podop[i * K + j] for j < n_out[i]: the ex_m traces with the largest r_K
 * among the traces of that pod-op's P_sr row in window i's graph of the detector's abnormal traces
 * (the graph ranked with anomaly = 0, T1), K the iters_done[i] the window ran; r_K[t] =
 * (q / w_t) / M_r(K) in fp64 in both precisions, mr_graph_trace_rank's expression.  Score descending
 * by fp64 bits, trace code ascending on equal bits: the answer does not depend on how the traces
 * are cut into blocks, on the grouping of the windows or on a window's place in the call.
 * ex_n[i * K + j] = min(ex_m, the op's coverage in that graph); 0 for a pod-op that is no node of
 * it (it occurs only in the detector's normal traces), for j >= n_out[i], and for a window that
 * ranked nothing or is empty.  A kind-hash collision rerun and a tol stop answer from the final
 * state.  Windows tiled from their table's layout order are answered by one selection launch and
 * one merge launch for the whole call; the others through mr_graph_exemplars' kernels, a window at
 * a time.  mr_windows_batch_ex itself is unchanged: it allocates, launches and copies nothing of this.
 * MR_ERR_ARG: ex_m outside 1..32, a null exemplar pointer, out_podop or n_out null,
 * top_max + 6 > 64 (mr_graph_exemplars' op limit), and mr_windows_batch_ex's. */
int mr_windows_batch_exemplars(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                               const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                               int method, int32_t top_max, int precision, int32_t* out_podop, double* out_score,
                               int32_t* n_out, int64_t* edges_traversed, int32_t* n_abnormal, int32_t* n_normal,
                               int32_t* status, int iters, double tol, int check_every, int32_t* iters_done,
                               double* resid, int32_t ex_m, int32_t* ex_trace, double* ex_score, int32_t* ex_n);
/* mr_windows_batch_exemplars with mr_graph_exemplars_ex's flags: every argument of
 * mr_windows_batch_exemplars in its order, then ex_flags and ex_mult.  ex_flags == 0 with ex_mult ==
 * NULL is mr_windows_batch_exemplars itself (which is this call with 0, NULL): the same launches.
 * MR_EX_DISTINCT_KINDS: row (i, j) holds one trace per trace kind of window i's graph of the
 * detector's abnormal traces (pagerank.py:54-66's exact classes, as that graph's ranking counts
 * them), each kind by its best member (score bits descending, trace code ascending), the first
 * min(ex_m, kinds in the row) of them in that order; ex_n[i * K + j] is that count.
 * ex_mult [n_windows * K * ex_m] host or NULL: the class size of every entry (the traces of that
 * kind in the window's graph), 0 padded and 0 wherever ex_trace is -1.  The answer does not depend on
 * the cut into blocks, on the grouping of the windows or on a window's place in the call; windows
 * tiled from their table's layout order are still answered by one selection launch and one merge
 * launch for the whole call (their kinds are the table's classes, kept by position only under the flag).
 * MR_ERR_ARG: a flag bit other than MR_EX_DISTINCT_KINDS, ex_mult with ex_flags == 0, and
 * mr_windows_batch_exemplars'.  MR_ERR_STATE: as mr_windows_batch_exemplars. */
int mr_windows_batch_exemplars_ex(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                                  const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                                  int method, int32_t top_max, int precision, int32_t* out_podop, double* out_score,
                                  int32_t* n_out, int64_t* edges_traversed, int32_t* n_abnormal, int32_t* n_normal,
                                  int32_t* status, int iters, double tol, int check_every, int32_t* iters_done,
                                  double* resid, int32_t ex_m, int32_t* ex_trace, double* ex_score, int32_t* ex_n,
                                  uint32_t ex_flags, int32_t* ex_mult /* [n_windows*K*ex_m] or NULL */);
/* mr_rca_window with the same five: iters_done one word, resid two (NULL: no report).
 * mr_rca_window(...) is mr_rca_window_ex(..., 25, 0.0, 1, NULL, NULL). */
int mr_rca_window_ex(mr_ctx* ctx, const mr_spans* s, int64_t t0, int64_t t1, const double* a3,
                     const uint8_t* a3_valid, int method, int32_t top_max, int precision,
                     int32_t* out_podop, double* out_score, int32_t* n_out, int64_t* edges_traversed,
                     int32_t* n_abnormal, int32_t* n_normal, int iters, double tol, int check_every,
                     int32_t* iters_done, double* resid);

/* ------------------------------------------------------------------ latency evidence
 * How slow is a suspect op in the abnormal traces, compared with the normal traces of the same
 * window?  No reference counterpart: the evidence an operator holds against a ranking before
 * believing it.  Per row i of a span table the value is
 *   MR_LAT_DURATION  duration[i]
 *   MR_LAT_SELF      duration[i] - csum[span[i]], csum[c] the sum of duration[j] over ALL rows j of
 *                    the table with parent[j] == c (parent[j] < 0 adds nothing); int64 arithmetic
 *                    that wraps, as numpy's.  The join is T11's: it ignores traceID, rows that
 *                    share a spanID code each receive the full child sum, an orphan's parent code
 *                    is -1.  Self time may be negative (duplicated spanIDs, broken traces).  csum
 *                    depends on the table alone: it is computed by the first call that needs it
 *                    and kept with the table, in a buffer nothing else reads.
 * A span's duration contains its children's, so every ancestor of a slow op looks slow; its self
 * time does not.
 * The selected rows of pod-op p, side s (0 normal, 1 abnormal, in the DETECTOR's sense -- the sense
 * the exemplars use) are the rows with podop[i] == p, state[trace[i]] == s + 1 (mr_detect's
 * state: 0 outside the window or dropped, 1 normal, 2 abnormal) and tstart[i] >= t0 && tend[i] <= t1
 * (inclusive; t0 == INT64_MIN and t1 == INT64_MAX: the whole table, as in mr_slo_quantiles).
 * Per asked op and side: count, the number of selected rows, and for each q[j]
 * numpy.quantile(values, q[j], method=...) with mr_slo_quantiles' three methods, bit for bit, in
 * duration units, not scaled and not rounded; a count of 0 gives 0.0.
 *
 * mr_op_latency: one window, the partition given by the caller (mr_detect's state[], host).
 * out[(j * 2 + side) * n_q + k] answers podops[j] and q[k]; count[j * 2 + side].  A duplicated
 * asked op is answered each time.
 * MR_ERR_ARG: a null pointer, n_ops outside 1..64 (mr_graph_exemplars' op limit), n_q outside
 * 1..16, an unknown what or method, a q[j] that is NaN or outside [0, 1], an asked op outside
 * [0, n_podops), s of another context, or a value range too wide to sort: grouping and ordering
 * are ONE sort of keys class << DB | (value - min) over the selected rows, class = (window * K +
 * slot) * 2 + side, DB = bits of (max - min) of the selected values, and bits(n_windows * K * 2) +
 * DB must not exceed 64.  MR_ERR_STATE: a time window on a table without trace-level times;
 * MR_LAT_SELF on a shard of a larger table (cols.row set: children may lie on another rank).
 * An argument error leaves the context usable. */
enum { MR_LAT_DURATION = 0, MR_LAT_SELF = 1 };
int mr_op_latency(mr_ctx* ctx, const mr_spans* s, int64_t t0, int64_t t1,
                  const uint8_t* state /*[n_traces] host*/, const int32_t* podops, int32_t n_ops, int what,
                  const double* q, int32_t n_q, int method, double* out /*[n_ops * 2 * n_q]: op, side, q */,
                  int64_t* count /*[n_ops * 2]*/);

/* Many windows: window i = spans[i], [t0[i], t1[i]], a3[i] / a3_valid[i] as in mr_windows_batch; the
 * partition is that window's mr_detect partition, computed on the device and never copied out.
 * podops[i * K + j], j < n_ops[i], are the asked ops: the row a ranking call returned in out_podop
 * with its n_out, K = that call's top_max + 6.  Entries j >= n_ops[i] are ignored: their out / count
 * are 0.  out[((i * K + j) * 2 + side) * n_q + k], count[(i * K + j) * 2 + side].  status[i]: MR_OK,
 * or MR_ERR_VALUE for an empty window (T2), whose out / count are 0.  One sort, one bounds pass and
 * one pick launch answer the whole call; a window's answer does not depend on its place in the call
 * or on the other windows.  The ranking entries (mr_windows_batch*, mr_rca_window*) are untouched:
 * evidence is a separate call that takes their top lists.
 * MR_ERR_ARG: K outside 1..64, n_ops[i] outside 0..K, and everything mr_op_latency rejects.
 * MR_ERR_STATE: a table without trace-level times; MR_LAT_SELF on a shard. */
int mr_windows_latency(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                       const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                       const int32_t* podops, const int32_t* n_ops, int32_t K, int what, const double* q,
                       int32_t n_q, int method, double* out /*[n_windows * K * 2 * n_q]*/,
                       int64_t* count /*[n_windows * K * 2]*/, int32_t* status /*[n_windows]*/);

/* ------------------------------------------------------------------ kind breakdown
 * Which request shapes does the anomaly hit, and which pass through a suspect op unharmed?
 * No reference counterpart: per asked pod-op of a window -- and for the window as a whole -- its
 * trace kinds with their abnormal and normal trace counts.  "Every call path through the op is slow"
 * points at the op; "one call path out of forty is" points at a caller.
 * Window i = spans[i], [t0[i], t1[i]], a3[i] / a3_valid[i] as in mr_windows_batch / mr_windows_latency;
 * its partition is that window's mr_detect partition (state 0 outside or dropped, 1 normal, 2
 * abnormal), computed on the device and never copied out.
 * Kind of a trace: the table's exact class -- the sorted set of distinct pod-op codes over ALL rows of
 * the trace and the bits of (float)(1.0 / rows of the trace) (pagerank.py:54-66's key).  A window
 * keeps whole traces, so its kinds are the table's classes restricted to the traces of state 1 or 2; a
 * kind is LIVE in the window when it has at least one such trace.
 * Asked slots: podops[i * K + j], j < n_ops[i].  A pod-op code p >= 0 selects the live kinds whose op
 * set contains p; -1 selects every live kind (the window's overall breakdown).  Per selected kind:
 *   n_abn  its traces in state 2          n_nor  its traces in state 1
 *   rep    its smallest trace code in state 2, or (n_abn == 0) its smallest trace code in state 1
 *   spans  the rows of a member           ops    the distinct pod-ops of a member
 * The answer of a slot is the first min(m, selected kinds) kinds under the total order n_abn
 * descending, then n_nor ascending, then rep ascending (rep is unique per kind):
 * kb_trace[(i * K + j) * m + e] = rep (-1 padded), kb_abn / kb_nor / kb_spans / kb_ops the same shape
 * (0 padded), kb_n[i * K + j] the entries, kb_kinds[i * K + j] the number of selected kinds,
 * kb_tot[(i * K + j) * 2 + {0, 1}] the summed n_abn / n_nor over ALL selected kinds -- for -1 the
 * window's abnormal and normal trace counts, for an op its trace coverage on each side.  A slot
 * asked twice is answered each time; an op with no trace in the window answers 0 entries and zero
 * totals; entries j >= n_ops[i] are ignored and answer the padding.  status[i]: MR_OK, or
 * MR_ERR_VALUE for an empty window (T2), whose outputs are the padding.  The answer does not depend
 * on the cut into blocks, the chunking of the call's windows (their dense per-kind counters stay
 * under a fixed scratch size), a window's place in the call, or the other windows: every count is an
 * integer sum, every order total.  The ranking entries are untouched and no ranking state is read:
 * evidence is a separate call that takes their top lists.
 * MR_ERR_ARG: a null pointer, K outside 1..64, m outside 1..32 (the exemplar entries' limits),
 * n_ops[i] outside 0..K, a code outside [-1, n_podops), a table of another context.
 * MR_ERR_STATE: a trace shard of a larger table (cols.row set: its counts would cover this rank's
 * traces only, and nothing merges the ranks'), a table without a per-trace index (its key bits did
 * not fit), a table without trace-level times (per-span window times cut traces: the table's classes
 * are not the window's kinds), or a table without a layout order (more than 4096 pod-ops, or past
 * the edge / count limits of the window build); the message names which.  There is no fallback for
 * any of them.
 * An argument error leaves the context usable. */
int mr_windows_kind_breakdown(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                              const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                              const int32_t* podops /*[n_windows * K], -1 = every kind*/, const int32_t* n_ops,
                              int32_t K, int32_t m, int32_t* kb_trace /*[n_windows * K * m] rep trace code, -1 padded*/,
                              int32_t* kb_abn, int32_t* kb_nor, int32_t* kb_spans,
                              int32_t* kb_ops /*same shape, 0 padded*/, int32_t* kb_n /*[n_windows * K] entries*/,
                              int32_t* kb_kinds /*[n_windows * K] selected kinds*/,
                              int64_t* kb_tot /*[n_windows * K * 2] abnormal, normal traces*/,
                              int32_t* status /*[n_windows]*/);

/* ------------------------------------------------------------------ call evidence
 * Is a suspect op slow whoever calls it, or only from one caller -- and which of its downstream calls
 * got slower on the abnormal traces?  No reference counterpart as an entry: the call graph of the
 * reference's model (operation_operation, preprocess_data.py:156-163) shown per asked pod-op, on each
 * side of the window's detector partition.
 * Window i = spans[i], [t0[i], t1[i]], a3[i] / a3_valid[i] as in mr_windows_batch; its partition is that
 * window's mr_detect state (0 outside or dropped, 1 normal, 2 abnormal), computed on the device and never
 * copied out.
 * Call pair: (child row c, parent row r) with parent[c] >= 0 and span[r] == parent[c] -- T11's join, as in
 * MR_LAT_SELF: traceID is ignored, EVERY row that shares the spanID code pairs with the child, an orphan
 * makes no pair.
 * Side: a pair belongs to side s (0 normal, 1 abnormal) when BOTH rows' traces have state s + 1 and both
 * rows lie in the window (tstart >= t0 && tend <= t1, inclusive; t0 == INT64_MIN and t1 == INT64_MAX: the
 * whole table, as in mr_op_latency).  With this rule the calls of edge (a -> b) on side s equal the
 * multiplicity of b in operation_operation[a] that the reference builds from that side's trace list over
 * the window's rows.
 * Per edge (parent pod-op -> child pod-op) and side:
 *   calls  the pair count (int64)
 *   dsum   the sum of the CHILD row's duration over the pairs (int64 that wraps, as numpy's)
 *   dmax   the largest child duration, 0 when calls == 0
 * Asked slots: podops[i * K + j], j < n_ops[i], a pod-op code p.  Two directions per slot: direction 0,
 * callers: the edges (q -> p), peer q; direction 1, callees: the edges (p -> c), peer c.  A self edge
 * p -> p appears in both.  Only peers with calls[0] + calls[1] > 0 in the window are selected: an edge of
 * the table that is dead in the window is not listed.
 * The answer of a (slot, direction) is the first min(m, selected) peers under the total order abnormal
 * calls descending, then normal calls ascending, then peer code ascending:
 *   ce_peer[((i * K + j) * 2 + dir) * m + e]                             the peer's code, -1 padded
 *   ce_calls / ce_dsum / ce_dmax[(((i * K + j) * 2 + dir) * m + e) * 2 + side]   0 padded
 *   ce_n[(i * K + j) * 2 + dir]      the entries
 *   ce_peers[(i * K + j) * 2 + dir]  the number of selected peers
 *   ce_tot[((i * K + j) * 2 + dir) * 2 + side]  the calls summed over ALL selected peers, not only the listed
 *   status[i]  MR_OK, or MR_ERR_VALUE for an empty window (T2), whose outputs are the padding
 * A slot asked twice is answered each time; an op with no call in the window answers 0 entries and zero
 * totals; entries j >= n_ops[i] answer the padding.
 * Every count is an integer sum or maximum and every order is total, so the answer does not depend on
 * the cut into blocks, the chunking of the call's windows (their dense per-edge counters stay under a
 * fixed scratch size), a window's place in the call, or the other windows: it is bitwise reproducible.
 * The ranking entries are untouched and no ranking state is read: evidence is a separate call that takes
 * their top lists.  No layout order is needed: tables with more than 4096 pod-ops work.
 * MR_ERR_ARG: a null pointer, K outside 1..64, m outside 1..32, n_ops[i] outside 0..K, a code outside
 * [0, n_podops), a table of another context.
 * MR_ERR_STATE: a trace shard of a larger table (cols.row set: parents may lie on another rank); a
 * table without the per-trace index (its key bits did not fit, or it is empty), whose edge dictionary
 * -- the sorted distinct (parent pod-op, child pod-op) keys of the join -- the counters and the
 * selection are laid out by; a table without startTime / endTime columns (unlike mr_op_latency, whose
 * caller brings the partition, this entry runs the window's detector, which reads them -- for the
 * whole table too); a time window on a table without trace-level times (the entry tells "in the
 * window" from the traces' states); a table whose join has 2^32 or more pairs in all (the selection
 * orders by a key that packs both sides' counts in 32 bits each, exact below that) or 2^31 or more
 * distinct edges (a list entry's id).  They are tested in this order and the message names which.
 * There is no fallback for any of them.
 * An argument error leaves the context usable. */
int mr_windows_call_edges(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                          const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                          const int32_t* podops /*[n_windows * K]*/, const int32_t* n_ops, int32_t K, int32_t m,
                          int32_t* ce_peer /*[n_windows * K * 2 * m] peer code, -1 padded*/,
                          int64_t* ce_calls, int64_t* ce_dsum,
                          int64_t* ce_dmax /*[n_windows * K * 2 * m * 2]: ..., side; 0 padded*/,
                          int32_t* ce_n /*[n_windows * K * 2] entries*/,
                          int32_t* ce_peers /*[n_windows * K * 2] selected peers*/,
                          int64_t* ce_tot /*[n_windows * K * 2 * 2] normal, abnormal calls*/,
                          int32_t* status /*[n_windows]*/);

/* ------------------------------------------------------------------ timeline evidence
 * WHEN inside the window: did the anomaly start at 14:03:10 and is it still going on, or was it a burst of
 * twenty seconds that is over; did the suspect op get slow at the moment the abnormal traces began, or was
 * it slow all along; is the abnormal share rising or falling?  No reference counterpart: per asked pod-op --
 * and for the window as a whole -- a dense, exact, integer histogram over time buckets, on each side of the
 * window's detector partition.  Every other evidence entry collapses the window's time axis.
 * Window i = spans[i], [t0[i], t1[i]], a3[i] / a3_valid[i]; its partition and its sides are exactly those of
 * mr_windows_call_edges / mr_windows_latency: that window's mr_detect state (0 outside or dropped, 1 normal,
 * 2 abnormal), computed on the device and never copied out; side 0 is normal, side 1 abnormal; t0 ==
 * INT64_MIN and t1 == INT64_MAX: the whole table.
 * Asked slots: podops[i * K + j], j < n_ops[i].
 *   A pod-op code p >= 0: the selected rows of (p, side) are mr_op_latency's -- podop[r] == p, the row's trace
 *   in state side + 1, the row inside the window.  A row's value is duration[r] for MR_LAT_DURATION and
 *   duration[r] - csum[span[r]] for MR_LAT_SELF, csum as in mr_op_latency (T11's join: traceID ignored; the
 *   buffer the first MR_LAT_SELF call on the table computes and keeps); int64 arithmetic that wraps, and the
 *   value may be negative.
 *   -1: the window's own timeline.  Each trace of state 1 or 2 counts ONCE, through the per-trace index; its
 *   value is the trace's tend - tstart (int64 that wraps), whatever `what` is.
 * Bucket of a row or trace: from its TRACE-LEVEL tstart (the table's times are constant within a trace, so a
 * trace falls in one bucket).  tstart < b0[i]: "before".  Otherwise delta = (uint64)tstart - (uint64)b0[i]
 * (exact since tstart >= b0, for b0 == INT64_MIN too), b = delta / bw[i] (unsigned); b >= B: "after".
 * Outputs, window i, asked entry j:
 *   tl_cnt / tl_sum / tl_max[((i * K + j) * B + b) * 2 + side]  the selected rows (traces) of bucket b: their
 *       number, the sum of their values (int64 that wraps, as numpy's) and the largest value; tl_max is 0
 *       where tl_cnt is 0
 *   tl_out[((i * K + j) * 2 + side) * 2 + {0, 1}]  the selected rows that fell before / after the bucket range
 *   status[i]  MR_OK, or MR_ERR_VALUE for an empty window (T2), whose outputs are all zero
 * So for an op slot the buckets' tl_cnt + before + after equals mr_windows_latency's count of that op and
 * side, and for slot -1 the window's normal or abnormal trace count.  A slot asked twice is answered each
 * time; an op without a row in the window answers zeros; entries j >= n_ops[i] answer zeros.
 * Every output is an integer sum or maximum, so the answer does not depend on the cut into blocks, the
 * chunking of the call's windows (their dense counters, K * (B + 2) * 2 * 3 words per window, stay under a
 * fixed scratch size), a window's place in the call, or the other windows: it is bitwise reproducible.
 * One row pass and one trace pass answer a chunk of windows, never a launch per op or per bucket.  The
 * ranking entries are untouched and no ranking state is read: evidence is a separate call that takes their
 * top lists.
 * MR_ERR_ARG: a null pointer, K outside 1..64, B outside 1..512, bw[i] <= 0, n_ops[i] outside 0..K, a code
 * outside [-1, n_podops), an unknown what, a table of another context.
 * MR_ERR_STATE, tested in this order: a table without startTime / endTime columns; a table whose times are
 * not trace-level (per-span window times: a trace must fall in one bucket -- for the whole table too; an
 * unindexed table with rows has no record that they are); MR_LAT_SELF on a trace shard of a larger table
 * (cols.row set: children may lie on another rank); slot -1 on a trace shard (its counts would cover this
 * rank's traces only), or on a table without the per-trace index.  The message names which.  There is no
 * fallback for any of them.  Op slots with MR_LAT_DURATION on a shard are allowed: they cover THAT RANK's
 * rows, under that rank's detector partition; nothing merges the ranks' timelines.
 * An argument error leaves the context usable. */
int mr_windows_timeline(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                        const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                        const int32_t* podops /*[n_windows * K], -1 = the window's traces*/, const int32_t* n_ops,
                        int32_t K, int what /*MR_LAT_DURATION | MR_LAT_SELF*/,
                        const int64_t* b0 /*[n_windows] bucket origin, ns*/,
                        const int64_t* bw /*[n_windows] bucket width, ns, > 0*/, int32_t B /*buckets, 1..512*/,
                        int64_t* tl_cnt, int64_t* tl_sum,
                        int64_t* tl_max /*[n_windows * K * B * 2]: window, slot, bucket, side*/,
                        int64_t* tl_out /*[n_windows * K * 2 * 2]: window, slot, side, {before, after}*/,
                        int32_t* status /*[n_windows]*/);

/* mr_windows_timeline with latency quantiles per bucket and side: lay a percentile SLO over the timeline, and
 * tell "p50 moved: everything got slower" from "only p99 moved: a few requests hang".
 * The arguments are mr_windows_timeline's, then q[n_q] (n_q in 1..16, every q in [0, 1]) and method (MR_Q_LINEAR
 * / MR_Q_LOWER / MR_Q_HIGHER), as mr_windows_latency's.  tl_cnt, tl_sum, tl_max, tl_out and status are, word
 * for word, what mr_windows_timeline writes for the same arguments.
 *   tl_q[(((i * K + j) * B + b) * 2 + side) * n_q + k]  the q[k]-quantile of the values counted in
 *       tl_cnt[((i * K + j) * B + b) * 2 + side], by numpy 2.x's np.quantile(values, q, method=...) on the int64
 *       values -- for a pod-op the op's selected rows whose trace starts in bucket b, valued by `what`; for -1
 *       the window's traces, each valued tend - tstart.  float64 in raw duration units, bit for bit
 *       mr_slo_quantiles' arithmetic; 0.0 where the count is 0.  The two outside buckets get no quantiles.
 * A code asked twice is answered each time; entries j >= n_ops[i] and an empty window answer zeros.
 * Per chunk of windows: the counters as in mr_windows_timeline, then one selection of packed keys, class <<
 * db | (value - vmin), class = ((window in chunk * slots + slot) * B + bucket) * 2 + side, db the bits of the
 * chunk's (vmax - vmin); ONE sort, one bounds pass and one pick for the chunk -- never a launch, a sort or a host
 * synchronisation per window, asked op or bucket.  Everything is integer until the pick, so tl_q is the same
 * bits under any cut into blocks, any chunking, any place of a window in the call and any neighbours.
 * MR_ERR_ARG: mr_windows_timeline's, and: n_q outside 1..16, a q outside [0, 1] (NaN too), an unknown method; a
 * chunk whose class bits plus db exceed 64 ("value range too wide to sort", naming the range; which chunks
 * fit depends on the cut).
 * MR_ERR_STATE: mr_windows_timeline's list, order and messages.
 * An argument error leaves the context usable. */
int mr_windows_timeline_q(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                          const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                          const int32_t* podops /*[n_windows * K], -1 = the window's traces*/, const int32_t* n_ops,
                          int32_t K, int what /*MR_LAT_DURATION | MR_LAT_SELF*/, const int64_t* b0, const int64_t* bw,
                          int32_t B /*buckets, 1..512*/, const double* q /*[n_q]*/, int32_t n_q /*1..16*/,
                          int method /*MR_Q_*/, int64_t* tl_cnt, int64_t* tl_sum, int64_t* tl_max, int64_t* tl_out,
                          double* tl_q /*[n_windows * K * B * 2 * n_q]: window, slot, bucket, side, q*/,
                          int32_t* status /*[n_windows]*/);

/* ------------------------------------------------------------------ replica evidence
 * Is it this POD, or is it the OPERATION?  The ranking names pod-ops (podName_op); the detector and the SLO
 * speak in service-ops (serviceName_op).  For each asked pod-op this entry answers with the pod-ops that
 * share its service-op -- its replicas -- on each side of the window's detector partition: one replica
 * slow and the others fine is a pod to drain; every replica slow on the abnormal traces is the operation.
 * No reference counterpart.
 * The table's map: sv(p) is the service-op code on the table's rows whose pod-op is p, over ALL rows of the
 * table (not a window's); a pod-op without a row has sv(p) = -1; a pod-op whose rows carry two different
 * service-op codes makes the table ambiguous (MR_ERR_STATE).  The replicas of service-op s are R(s) =
 * { q : sv(q) == s }, in code order.  The map is built at the first call on a table and kept with it.
 * Window, partition, sides and the selected rows are exactly mr_windows_timeline's op slots: window i =
 * spans[i], [t0[i], t1[i]], a3[i] / a3_valid[i]; its own mr_detect state, computed on the device and never
 * copied out; side 0 normal, side 1 abnormal; the selected rows of (q, side) have podop == q, their trace in
 * state side + 1, and lie inside the window; t0 == INT64_MIN and t1 == INT64_MAX: the whole table.  A row's
 * value is duration (MR_LAT_DURATION) or duration - csum[span] (MR_LAT_SELF, csum as in mr_op_latency):
 * int64 that wraps, possibly negative.
 * Per asked entry p = podops[i * K + j], j < n_ops[i], s = sv(p); for every q in R(s) and side: cnt the
 * selected rows, sum their values (int64 that wraps), max their largest value (0 where cnt is 0).  A replica
 * is LIVE when cnt[0] + cnt[1] > 0.  The live replicas are ordered by abnormal count descending, then normal
 * count ascending, then code ascending (mr_windows_call_edges' rule: a total order).
 * Outputs, window i, asked entry j (x = i * K + j):
 *   rp_pod[x * m + e]                       the first min(m, live) replicas, -1 padded; p is a replica like any other
 *   rp_cnt / rp_sum / rp_max[(x * m + e) * 2 + side]   their numbers, 0 padded
 *   rp_n[x]      the number of entries
 *   rp_live[x]   the live replicas
 *   rp_all[x]    |R(s)|, the replicas the table knows
 *   rp_place[x]  the 0-based place of p among ALL live replicas under the order: -1 when p has no selected
 *                row; it can be >= m
 *   rp_own[(x * 2 + side) * 3 + {cnt, sum, max}]   the numbers of p itself, listed or not
 *   rp_tot[(x * 2 + side) * 3 + {cnt, sum, max}]   the numbers over ALL live replicas: the service-op's own
 *   status[i]    MR_OK, or MR_ERR_VALUE for an empty window (T2), whose outputs are the padding
 * The padding: rp_pod -1, rp_place -1, everything else 0 (rp_all too).  A code asked twice is answered each
 * time; two asked codes with the same sv get the same list and totals with their own rp_place and rp_own;
 * sv(p) == -1 answers the padding; entries j >= n_ops[i] answer the padding.
 * Every output is an integer sum, an integer maximum or a place in a total order, so the answer is the same
 * bits under any cut into blocks, any chunking of the call's windows, any place of a window in the call and
 * any neighbours: it is bitwise reproducible.  The order compares the two counts as they are (no packed
 * key), so it is exact for every count a table can hold.
 * MR_ERR_ARG: a null pointer, K outside 1..64, m outside 1..32, n_ops[i] outside 0..K, a code outside
 * [0, n_podops), an unknown what, a table of another context.
 * MR_ERR_STATE, tested in this order, the message naming which: a table without startTime / endTime columns;
 * a time window on a table without trace-level times (the whole table is allowed there); MR_LAT_SELF on a
 * trace shard of a larger table (cols.row set: children may lie on another rank); an ambiguous table (the
 * message gives one offending pod-op code and its two service-op codes); a window whose asked service-ops
 * hold 2^30 or more replicas (a counter's key has 31 bits).  There is no fallback for any of them.
 * MR_LAT_DURATION on a shard is allowed: it covers THAT RANK's rows and that rank's map, as the timeline's op
 * slots do; nothing merges the ranks' replicas.
 * An argument error or a state error leaves the context usable. */
int mr_windows_replicas(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                        const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                        const int32_t* podops /*[n_windows * K]*/, const int32_t* n_ops, int32_t K /*1..64*/,
                        int32_t m /*1..32*/, int what /*MR_LAT_DURATION | MR_LAT_SELF*/,
                        int32_t* rp_pod /*[n_windows * K * m]*/, int64_t* rp_cnt, int64_t* rp_sum,
                        int64_t* rp_max /*[n_windows * K * m * 2]: window, entry, replica, side*/,
                        int32_t* rp_n, int32_t* rp_live, int32_t* rp_all, int32_t* rp_place /*[n_windows * K]*/,
                        int64_t* rp_own, int64_t* rp_tot /*[n_windows * K * 2 * 3]: window, entry, side, {cnt, sum, max}*/,
                        int32_t* status /*[n_windows]*/);

/* ------------------------------------------------------------------ endpoint evidence
 * Which user-facing endpoints are hit, and through which of them does the anomaly reach a suspect op?
 * "POST /preserve has 412 abnormal traces of 430, GET /stations 0 of 9800"; "every abnormal trace through
 * order_query entered at preserve".  The kind breakdown splits one endpoint into dozens of exact op sets and
 * never names it; this entry groups a window's traces by their ENTRY operation.  It is the first evidence that
 * counts DISTINCT TRACES per op.  No reference counterpart.
 * Per table, independent of the window:
 *   Root row: a row r with parent[r] < 0 -- its ParentSpanId is null or is no spanID of the table.
 *   Entry row of trace t: among t's root rows the one with the largest duration, compared as int64; ties go to
 *   the smallest row position in the table.
 *   Endpoint of t: podop[entry row]; MR_EP_NONE (-2) when t has no root row (a parent cycle, or every parent
 *   resolving to another trace's span).
 *   Value of t: d(t) = tend - tstart at trace level, as the int64 it wraps to.
 *   Endpoint universe: the table's distinct endpoints in pod-op code order, MR_EP_NONE last.
 * The endpoints are computed at the first call on a table and kept with it; mr_spans_entry_ops copies them out:
 * ep[t], t < n_traces, the endpoint's pod-op code or MR_EP_NONE.
 * Window i = spans[i], [t0[i], t1[i]], a3[i] / a3_valid[i] as in mr_windows_kind_breakdown; its partition is that
 * window's mr_detect state (0 not counted, 1 normal, 2 abnormal), computed on the device and never copied out;
 * side 0 is normal, side 1 abnormal.
 * Asked slots: podops[i * K + j], j < n_ops[i].  -1 selects every trace of the window (state 1 or 2); a pod-op
 * code p >= 0 selects the traces with AT LEAST ONE row of pod-op p -- each trace once, however many spans of p
 * it holds.  Per slot, endpoint E and side:
 *   cnt  the selected traces whose endpoint is E
 *   sum  the sum of d(t) over them (uint64 that wraps, given as int64)
 *   max  the largest d(t), 0 where cnt is 0
 * An endpoint is LIVE in a slot when cnt[0] + cnt[1] > 0.  The live endpoints are ordered by abnormal count
 * descending, then normal count ascending, then code ascending with MR_EP_NONE last: a total order.
 * Outputs, window i, asked entry j (x = i * K + j):
 *   ep_op[x * m + e]                                  the first min(m, live) endpoints: a pod-op code or MR_EP_NONE; -1 padded
 *   ep_cnt / ep_sum / ep_max[(x * m + e) * 2 + side]  their numbers, 0 padded
 *   ep_n[x]     the number of entries
 *   ep_live[x]  the live endpoints
 *   ep_tot[(x * 2 + side) * 3 + {cnt, sum, max}]      the numbers over ALL live endpoints: for -1 the window's
 *               traces of that side, for an op its trace coverage
 *   status[i]   MR_OK, or MR_ERR_VALUE for an empty window (T2), whose outputs are the padding
 * The padding: ep_op -1, everything else 0.  A slot asked twice is answered each time; an op with no trace in
 * the window and entries j >= n_ops[i] answer the padding.
 * Every output is an integer sum, an integer maximum or a place in a total order, so the answer is the same
 * bits under any cut into blocks, any chunking of the call's windows (MR_EP_CHUNK / MR_EP_BLOCKS, read per call,
 * force a cut), any place of a window in the call and any neighbours.  One count launch answers a chunk of
 * windows, never a launch per op or per endpoint.  The ranking entries are untouched and no ranking state is read.
 * MR_ERR_ARG: a null pointer, K outside 1..64, m outside 1..32, n_ops[i] outside 0..K, a code outside
 * [-1, n_podops), a table of another context.
 * MR_ERR_STATE, tested in this order, the message naming which: a table without the per-trace index (its key
 * bits did not fit, or it is empty: its per-trace distinct pod-op lists are what an op slot reads); a table
 * without trace-level times (no startTime / endTime columns, or times that vary within a trace: d(t) is the
 * trace's); a trace shard of a larger table (cols.row set: a parent may lie on another rank, so a local root
 * need not be a root; mr_spans_entry_ops refuses it too); a window whose slots times (endpoints + 1) reach 2^30
 * (a counter's key is an int32).  There is no fallback for any of them.
 * An argument error or a state error leaves the context usable. */
#define MR_EP_NONE (-2)
int mr_spans_entry_ops(mr_ctx* ctx, const mr_spans* s, int32_t* ep /*[n_traces]: endpoint pod-op code or MR_EP_NONE*/);
int mr_windows_endpoints(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                         const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                         const int32_t* podops /*[n_windows * K], -1 = the window's traces*/, const int32_t* n_ops,
                         int32_t K /*1..64*/, int32_t m /*1..32*/,
                         int32_t* ep_op /*[n_windows * K * m] endpoint code, MR_EP_NONE, or -1 padding*/,
                         int64_t* ep_cnt, int64_t* ep_sum,
                         int64_t* ep_max /*[n_windows * K * m * 2]: window, entry, endpoint, side; 0 padded*/,
                         int32_t* ep_n, int32_t* ep_live /*[n_windows * K]*/,
                         int64_t* ep_tot /*[n_windows * K * 2 * 3]: window, entry, side, {cnt, sum, max}*/,
                         int32_t* status /*[n_windows]*/);

/* ------------------------------------------------------------------ multi-GPU (RCCL over xGMI)
 * One process per GPU.  The unique id (128 bytes) is produced by rank 0 and broadcast by the
 * caller (torch.distributed / any host channel).  Used by the trace-sharded PageRank. */
int mr_comm_unique_id(uint8_t id[128]);
int mr_comm_init(mr_ctx* ctx, int nranks, int rank, const uint8_t id[128]);
int mr_comm_allreduce_f64(mr_ctx* ctx, double* dev_buf, int64_t n, int op /*0 sum, 1 max*/);

/* Host-staged collectives instead of RCCL (ranks sharing one GPU, CPU-side transports, tests):
 * the library copies the operand to host memory, calls fn, and copies the result back.
 *   coll 0 allreduce: buf[n] in/out, op 0 sum / 1 max
 *   coll 1 allgather: buf[nranks * n]; this rank's n elements are at rank * n on entry
 * dtype: 0 float64, 1 int32, 2 uint64, 3 int64.  fn returns 0 on success. */
typedef int (*mr_host_coll_fn)(void* user, int coll, void* buf, int64_t n, int dtype, int op);
int mr_comm_set_host(mr_ctx* ctx, mr_host_coll_fn fn, void* user, int nranks, int rank);

/* One-shot peer all-reduce for the per-iteration exchange of mr_pagerank_sharded (collective:
 * every rank of the context's backend calls it).  enable != 0: each rank exports a receive region
 * (uncached device memory) by IPC and maps every other rank's; an iteration's P_sr r limbs are then
 * written straight into every rank's region (xGMI stores between GPUs, one hop) and summed locally
 * in rank order, instead of an RCCL ring all-reduce (2 (R - 1) dependent steps).  The handles are
 * exchanged over the context's collectives on first use; enable = 0 unmaps them. */
int mr_comm_peer_enable(mr_ctx* ctx, int enable);
/* *active: 1 while the peer path carries this context's all-reduces (enabled and its regions
 * mapped on every rank), 0 otherwise -- e.g. after the ranks agreed that a mapping failed and fell
 * back to the RCCL / host collective, or after a peer timeout reset the regions.  Not collective. */
int mr_comm_peer_active(mr_ctx* ctx, int* active);

/* Trace-sharded PageRank: g holds THIS rank's traces (every span of
 * a trace on one rank) over the GLOBAL node index space, with this rank's partial len_o and
 * nchild and its local call edges.  Once per graph the library sums len_o / nchild / coverage,
 * unites the call edges, merges the trace-kind classes and the preference sums over the ranks;
 * per iteration it takes the max of r' and sums the P_sr r partials: exact fixed-point uint64
 * limbs on the fused iteration (N <= 16384), fp64 per-op sums on the tile path (larger N, C5).
 * Afterwards every rank holds the same weight and coverage vectors (mr_graph_fetch).
 * Requires a collective backend (mr_comm_init or mr_comm_set_host). */
int mr_pagerank_sharded(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters,
                        int precision, uint32_t flags);

/* mr_pagerank_sharded with mr_pagerank_converge's convergence report and early stop: the answer to
 * README.md:37 ("more iterations in PageRank" on a large system) on the path built for large systems,
 * where pagerank.py:117's fixed count is least likely to fit.  A shard of mr_graph_build_sharded or
 * an uploaded one.  Collective: every rank calls it, with the same arguments.
 * After every iteration each rank records resid[k-1] = max over ops of | s_k - s_{k-1} | of the WHOLE
 * graph (the vectors are replicated after the iteration's all-reduce).  At every check -- every
 * check_every iterations, at max_iters, or once at the end when tol == 0 -- the stretch's words meet
 * in one MAX all-reduce over the context's collective (never the peer regions) and only then are
 * read, so every rank reads the same words and takes the same decision: one small collective per
 * check, none per iteration.  Before the first iteration the ranks all-gather their requests
 * (max_iters, check_every, tol, d, alpha, phi, precision, flags, anomaly): ranks that asked
 * differently would run different numbers of collectives and hang.
 * Contract: after a call that ran K = *iters_done iterations, mr_graph_fetch is bitwise that of
 * mr_pagerank_sharded(..., iters = K, ...) on the same shards and backend; resid is identical on
 * every rank; mr_graph_trace_rank_sharded / mr_graph_exemplars_sharded follow the K iterations.
 * A kind-hash collision reruns the attempt on every rank and overwrites the history.
 * One rank without a backend runs with no collective at all.
 * MR_ERR_ARG: bad handles, iters_done or resid null (converged_at may be NULL), requests that
 * differ between the ranks (on EVERY rank, before anything ran), max_iters < 1, check_every < 1,
 * tol negative or NaN, phi <= 0, MR_PR_KIND_COMPRESS.  MR_ERR_COMM: several ranks and no backend.
 * MR_ERR_STATE: a kind-hash collision under every seed.  Everything else as mr_pagerank_sharded. */
int mr_pagerank_sharded_converge(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int max_iters,
                                 double phi, int precision, uint32_t flags, double tol, int check_every,
                                 int32_t* iters_done,      /* out: iterations run, the same on every rank */
                                 double* resid,            /* [max_iters] host; entries >= iters_done are 0.0 */
                                 int32_t* converged_at);   /* one word: first k (1-based) with resid[k-1] <= tol,
                                                              -1 if none; may be NULL */

/* The trace half of the last SHARDED ranking (mr_pagerank_sharded, mr_pagerank_sharded_converge: the
 * iterations it ran), for this rank's traces: mr_graph_trace_rank on a shard.  pagerank.py:119-127's
 * request_ranking_vector is max-normalised over ALL traces; the whole graph's maximum M_r(K) is on
 * every rank already (it rides the per-iteration all-reduce), so r[t] = (q / w_t) / M_r(K) needs no
 * exchange and the ranks' vectors concatenate to the whole graph's.  Not collective.  fp64 in both
 * precisions; K = 0 gives 1 / (N + T of all ranks); the rule for traces without ops is
 * mr_graph_trace_rank's.  A shard without traces writes nothing.
 * gid[t] (may be NULL): the trace's global id -- its trace code on a graph of mr_graph_build_sharded
 * (the codes are global), else the lower ranks' trace count + t (the position in the ranks'
 * concatenation; the counts are gathered once per graph).
 * MR_ERR_ARG: g or r null.  MR_ERR_STATE: no ranking yet (or its state re-set since), or the graph's
 * last ranking was not a sharded one. */
int mr_graph_trace_rank_sharded(mr_graph* g, double* r /*[T] host: this rank's traces*/,
                                int64_t* gid /*[T] host or NULL*/);
/* mr_graph_exemplars over the WHOLE graph of a sharded ranking.  Collective: every rank calls it with
 * the same ops and m, and every rank receives the same answer.  For each asked node index ops[i] the
 * m traces with the largest r among the traces of that op's P_sr row on ANY rank (pagerank.py:42-45,
 * the relation `coverage` counts), score descending, global id (mr_graph_trace_rank_sharded's gid:
 * the trace code on a graph of mr_graph_build_sharded) ascending on equal fp64 values.  out_n[i] = min(m, coverage[ops[i]] of the whole graph); the rest of
 * row i is padded with -1 / 0.0.  A duplicated op is answered each time.
 * Each rank selects from its own traces with mr_graph_exemplars' kernels; the lists meet in ONE
 * all-gather of a buffer whose size does not depend on the request (64 x 32 records, 64 counts, a
 * header), and every rank merges them.  A rank without a trace of an op, or without traces, sends
 * empty lists and still joins the collective.
 * MR_ERR_ARG: null pointers, n_ops outside 1..64, m outside 1..32, an op outside [0, N), more than
 * 256 ranks -- checked per rank before the collective, so every rank must pass them alike -- and, on
 * EVERY rank after it, requests (ops, m) or rankings (iterations, precision) that differ between the
 * ranks.  MR_ERR_STATE: as mr_graph_trace_rank_sharded.  Not covered: MR_EX_DISTINCT_KINDS across
 * shards (kinds are merged over the ranks by hash only) and kind-compressed rankings. */
int mr_graph_exemplars_sharded(mr_graph* g, const int32_t* ops, int32_t n_ops, int32_t m,
                               int64_t* out_trace /*[n_ops*m] global ids, -1 padded*/,
                               double* out_score /*[n_ops*m], 0.0 padded*/, int32_t* out_n /*[n_ops]*/);

#ifdef __cplusplus
}
#endif
#endif /* MICRORANK_HIP_H */
