// The span table on the device: mr_spans_upload (int-coded columns from the host), the spanID ->
// rows multimap that the parent join ParentSpanId == spanID reads (preprocess_data.py:157-158; a
// counting sort by spanID code, duplicates kept, T11), and mr_spans_free.  mr_spans_finish is the
// common tail of mr_spans_upload and mr_spans_ingest (mr_ingest.hip): the multimap, then the
// per-trace index every graph build and detector reads (mr_span_index.hip).
#include <algorithm>

#include "mr_internal.h"
#include "mr_prim.h"
#include "mr_sort.h"

namespace {
__global__ void k_count_codes(const int64_t* span, int64_t S, int32_t* cnt) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S) atomicAdd(&cnt[span[i]], 1);
}
__global__ void k_fill_ids(const int64_t* span, int64_t S, const int64_t* off, int32_t* cur, int32_t* rows) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S) {
        int64_t c = span[i];
        rows[off[c] + atomicAdd(&cur[c], 1)] = (int32_t)i;
    }
}
// rows inside a spanID bucket ascending (buckets hold duplicates only: tiny)
__global__ void k_sort_buckets(const int64_t* off, int64_t n_codes, int32_t* rows) {
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_codes) return;
    int64_t a = off[c], b = off[c + 1];
    for (int64_t i = a + 1; i < b; ++i) {
        int32_t v = rows[i];
        int64_t j = i - 1;
        while (j >= a && rows[j] > v) {
            rows[j + 1] = rows[j];
            --j;
        }
        rows[j + 1] = v;
    }
}
}  // namespace

int mr_spans_finish(mr_ctx* ctx, mr_spans* s);

extern "C" int mr_spans_upload(mr_ctx* ctx, const mr_span_cols* c, mr_spans** out) {
    if (!ctx || !c || !out) return mr_fail(ctx, MR_ERR_ARG, "mr_spans_upload: null argument");
    *out = nullptr;
    const int64_t S = c->n_spans;
    if (S < 0 || S >= (1ll << 31)) return mr_fail(ctx, MR_ERR_ARG, "n_spans out of range (int32 row ids)");
    if (S && (!c->trace || !c->podop || !c->svcop || !c->span || !c->parent || !c->duration))
        return mr_fail(ctx, MR_ERR_ARG, "mr_spans_upload: missing column");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    int64_t max_code = -1;
    for (int64_t i = 0; i < S; ++i) {
        if (c->span[i] < 0) return mr_fail(ctx, MR_ERR_ARG, "negative span code at row %lld", (long long)i);
        if (c->trace[i] < 0 || c->trace[i] >= c->n_traces || c->podop[i] < 0 || c->podop[i] >= c->n_podops ||
            c->svcop[i] < 0 || c->svcop[i] >= c->n_svcops)
            return mr_fail(ctx, MR_ERR_ARG, "code out of range at row %lld", (long long)i);
        max_code = std::max(max_code, c->span[i]);
    }
    auto* s = new mr_spans();
    s->ctx = ctx;
    s->S = S;
    s->n_traces = c->n_traces;
    s->n_podops = c->n_podops;
    s->n_svcops = c->n_svcops;
    s->n_span_codes = max_code + 1;
    s->has_times = c->tstart && c->tend;
    int64_t row_max = S;
    if (c->row) {
        row_max = 0;
        for (int64_t i = 0; i < S; ++i) {
            if (c->row[i] < 0 || (i && c->row[i] <= c->row[i - 1]))
                return mr_fail(ctx, MR_ERR_ARG, "row: global row indices must be non-negative and ascending");
            row_max = std::max<int64_t>(row_max, c->row[i]);
        }
    }
    s->row_bits = bits_for((uint64_t)std::max<int64_t>(row_max, 1));
    int rc = MR_OK;
    auto fail = [&](int code) {
        delete s;
        return code;
    };
    if ((rc = s->trace.upload(ctx, c->trace, S)) || (rc = s->podop.upload(ctx, c->podop, S)) ||
        (rc = s->svcop.upload(ctx, c->svcop, S)) || (rc = s->span.upload(ctx, c->span, S)) ||
        (rc = s->parent.upload(ctx, c->parent, S)) || (rc = s->duration.upload(ctx, c->duration, S)))
        return fail(rc);
    if (s->has_times && ((rc = s->tstart.upload(ctx, c->tstart, S)) || (rc = s->tend.upload(ctx, c->tend, S))))
        return fail(rc);
    if (c->row && (rc = s->grow.upload(ctx, c->row, S))) return fail(rc);
    if ((rc = mr_spans_finish(ctx, s))) return fail(rc);
    mr_handle_add(ctx, s, [](void* h) { delete (mr_spans*)h; });
    *out = s;
    return MR_OK;
}

// device columns in place -> the spanID -> rows multimap (counting sort by code) and the
// per-trace index; shared by mr_spans_upload (int codes) and mr_spans_ingest (strings)
int mr_spans_finish(mr_ctx* ctx, mr_spans* s) {
    const int64_t S = s->S, U = s->n_span_codes;
    DBuf<int32_t> cnt;
    DBuf<int64_t> tmp;
    MR_TRY(cnt.zero(ctx, (size_t)U));
    MR_TRY(s->id_off.alloc(ctx, (size_t)U + 1));
    MR_TRY(s->id_rows.alloc(ctx, (size_t)S));
    MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(U)));
    if (S) hipLaunchKernelGGL(k_count_codes, dim3(cdiv(S, 256)), dim3(256), 0, ctx->stream, s->span.p, S, cnt.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, cnt.p, s->id_off.p, U, tmp.p));
    if (U) MR_TRY_HIP(ctx, hipMemsetAsync(cnt.p, 0, U * sizeof(int32_t), ctx->stream));
    if (S)
        hipLaunchKernelGGL(k_fill_ids, dim3(cdiv(S, 256)), dim3(256), 0, ctx->stream, s->span.p, S, s->id_off.p, cnt.p,
                           s->id_rows.p);
    if (U) hipLaunchKernelGGL(k_sort_buckets, dim3(cdiv(U, 256)), dim3(256), 0, ctx->stream, s->id_off.p, U, s->id_rows.p);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        return mr_fail(ctx, MR_ERR_HIP, "span table setup: kernel failure");
    return mr_spans_index(ctx, s);
}

extern "C" int mr_spans_free(mr_spans* s) {
    if (!s || !mr_handle_take(s)) return MR_OK;   // (freed with its context)
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    delete s;
    return MR_OK;
}
