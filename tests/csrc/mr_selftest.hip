// Test-only entry points (libmicrorank_selftest.so) that drive the shared device primitives alone:
// the scan and the sort through the product's own compiled host functions (linked from
// libmicrorank_hip.so), the header primitives of mr_prim.h / mr_evidence.h through thin kernels that
// call them the way the product's kernels do.  Host arrays in, host arrays out, one launch sequence
// and one stream synchronise per call.  Loaded by tests/prim_util.py; no part of the public ABI.
#include "mr_evidence.h"
#include "mr_internal.h"
#include "mr_prim.h"
#include "mr_sort.h"

namespace {
constexpr int ST_T = 256;   // threads per block of the run / table kernels (the evidence kernels' EX_T, TL_T, RP_T)

// every lane of every wave calls wave_run_reduce; lanes past n bring key -1 and no value (as the
// evidence kernels' lanes past their last row do)
template <class K>
__global__ void __launch_bounds__(ST_T) k_runs(const int64_t* keys, const uint8_t* has, const unsigned long long* d,
                                               int64_t n, unsigned long long* on, unsigned long long* os,
                                               unsigned long long* om, uint8_t* last) {
    const int64_t i = (int64_t)blockIdx.x * ST_T + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const K kd = i < n ? (K)keys[i] : (K)-1;
    EvRun run = ev_run_of(i < n && has[i] != 0, i < n ? d[i] : 0ull);
    const bool tail = wave_run_reduce(lane, kd, run);
    if (i < n) {
        on[i] = run.n;
        os[i] = run.sum;
        om[i] = run.mx;
        last[i] = tail ? 1 : 0;
    }
}

// k_tl_count / k_rp_count / k_ce_count's frame: clear, barrier, tiles block by block (a wave without a
// key skips the reduction), barrier, flush.  Tile t of block b is tile t * gridDim.x + b.
template <class K>
__global__ void __launch_bounds__(ST_T) k_evtable(const int64_t* keys, const unsigned long long* d, int64_t n, int direct_,
                                                  int tiles, unsigned long long* cnt) {
    __shared__ EvTable tab;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool direct = direct_ != 0;
    tab.clear(threadIdx.x, ST_T);
    __syncthreads();
    for (int t = 0; t < tiles; ++t) {   // (block-uniform)
        const int64_t c = ((int64_t)t * gridDim.x + blockIdx.x) * ST_T + threadIdx.x;
        K kd = c < n ? (K)keys[c] : (K)-1;
        if (kd < 0) kd = -1;
        const unsigned long long dd = c < n ? d[c] : 0ull;
        if (__ballot(kd >= 0) == 0ull) continue;   // (wave-uniform)
        EvRun run = ev_run_of(kd >= 0, dd);
        const bool tail = wave_run_reduce(lane, kd, run);
        if (kd >= 0 && tail) tab.add(direct, cnt, kd, run);
    }
    __syncthreads();
    tab.flush<K>(direct, cnt, threadIdx.x, ST_T);
}

// op: 0 block_sum, 1 block_max, 2 wave_sum, 3 wave_max (doubles), 4 wave_sum_i64; every thread
// writes the value it holds
__global__ void k_block_reduce(int op, const double* in, double* out) {
    __shared__ double red[1024 / WAVE];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (op == 4) {
        ((int64_t*)out)[i] = wave_sum_i64(((const int64_t*)in)[i]);
        return;   // (launch-uniform)
    }
    const double v = in[i];
    out[i] = op == 0 ? block_sum(v, red) : op == 1 ? block_max(v, red) : op == 2 ? wave_sum(v) : wave_max(v);
}

struct OwnerD {   // a descriptor with its start behind another field, as the product's (GDev, PDev, ...)
    int32_t tag, first;
};
__global__ void k_block_owner(const OwnerD* ds, int32_t n, int32_t nblk, int32_t* out) {
    const int32_t b = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b < nblk) out[b] = block_owner<OwnerD, &OwnerD::first>(ds, n, b);
}

int sync(mr_ctx* ctx) {
    MR_TRY_HIP(ctx, hipGetLastError());
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MR_OK;
}
}  // namespace

extern "C" {

// in: n int64 (is32 == 0) or int32 counts; out: n + 1 int64.  in_place (int64 only): the scan runs
// with in == out on the device.
int mrt_scan(mr_ctx* ctx, const void* in, int is32, int64_t n, int in_place, int64_t* out) {
    if (!ctx || n < 0 || !out || (n && !in) || (is32 && in_place)) return mr_fail(ctx, MR_ERR_ARG, "mrt_scan: bad arguments");
    DBuf<int64_t> d_out, d_tmp, d_in64;
    DBuf<int32_t> d_in32;
    MR_TRY(d_out.alloc(ctx, (size_t)n + 1));
    MR_TRY(d_tmp.alloc(ctx, (size_t)scan_tmp_elems(n)));
    if (is32) {
        MR_TRY(d_in32.upload(ctx, (const int32_t*)in, (size_t)n));
        MR_TRY(mr_exclusive_scan_i32(ctx, d_in32.p, d_out.p, n, d_tmp.p));
    } else if (in_place) {
        if (n) MR_TRY_HIP(ctx, hipMemcpyAsync(d_out.p, in, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        MR_TRY(mr_exclusive_scan(ctx, d_out.p, d_out.p, n, d_tmp.p));
    } else {
        MR_TRY(d_in64.upload(ctx, (const int64_t*)in, (size_t)n));
        MR_TRY(mr_exclusive_scan(ctx, d_in64.p, d_out.p, n, d_tmp.p));
    }
    MR_TRY(d_out.download(ctx, out, (size_t)n + 1));
    return sync(ctx);
}

// the context's scan epoch as the next look-back scan will find it
int mrt_set_scan_epoch(mr_ctx* ctx, uint32_t epoch) {
    if (!ctx) return MR_ERR_ARG;
    ctx->scan_epoch = epoch;
    return MR_OK;
}
// ... and the epoch of the last one with the status words the context holds
int mrt_scan_state(mr_ctx* ctx, uint32_t* epoch, uint64_t* words) {
    if (!ctx || !epoch || !words) return MR_ERR_ARG;
    *epoch = ctx->scan_epoch;
    *words = (uint64_t)ctx->scan_cap;
    return MR_OK;
}

// keys [n] (and vals [n], or null) sorted in place on the keys' low `bits` bits
int mrt_sort(mr_ctx* ctx, uint64_t* keys, uint32_t* vals, int64_t n, int bits) {
    if (!ctx || n < 0 || (n && !keys) || bits < 0 || bits > 64) return mr_fail(ctx, MR_ERR_ARG, "mrt_sort: bad arguments");
    DBuf<uint64_t> dk;
    DBuf<uint32_t> dv;
    MR_TRY(dk.upload(ctx, keys, (size_t)n));
    if (vals) MR_TRY(dv.upload(ctx, vals, (size_t)n));
    {
        SortScratch ws;
        MR_TRY(mr_radix_sort(ctx, dk.p, vals ? dv.p : nullptr, n, bits, ws));
        MR_TRY(dk.download(ctx, keys, (size_t)n));
        if (vals) MR_TRY(dv.download(ctx, vals, (size_t)n));
        MR_TRY(sync(ctx));
    }
    return MR_OK;
}

int mrt_bits_for(uint64_t maxval) { return bits_for(maxval); }

// wave_run_reduce over the stream keys / has / d [n] cut into waves of 64 lanes (K: int32_t for
// key_bits == 32, int64_t for 64; a last partial wave is filled with key -1, no value).  Per lane: the
// EvRun it holds afterwards (n, sum, biased max) and whether it was told it is its run's last.
int mrt_runs(mr_ctx* ctx, int key_bits, const int64_t* keys, const uint8_t* has, const uint64_t* d, int64_t n,
             uint64_t* out_n, uint64_t* out_sum, uint64_t* out_max, uint8_t* out_last) {
    if (!ctx || (key_bits != 32 && key_bits != 64) || n < 1 || !keys || !has || !d || !out_n || !out_sum || !out_max || !out_last)
        return mr_fail(ctx, MR_ERR_ARG, "mrt_runs: bad arguments");
    if (key_bits == 32)
        for (int64_t i = 0; i < n; ++i)
            if (keys[i] != (int64_t)(int32_t)keys[i]) return mr_fail(ctx, MR_ERR_ARG, "mrt_runs: key %lld is no int32", (long long)keys[i]);
    DBuf<int64_t> dk;
    DBuf<uint8_t> dh, dl;
    DBuf<unsigned long long> dd, dn, ds, dm;
    MR_TRY(dk.upload(ctx, keys, (size_t)n));
    MR_TRY(dh.upload(ctx, has, (size_t)n));
    MR_TRY(dd.upload(ctx, (const unsigned long long*)d, (size_t)n));
    MR_TRY(dn.alloc(ctx, (size_t)n));
    MR_TRY(ds.alloc(ctx, (size_t)n));
    MR_TRY(dm.alloc(ctx, (size_t)n));
    MR_TRY(dl.alloc(ctx, (size_t)n));
    const dim3 grid(cdiv(n, ST_T)), block(ST_T);
    if (key_bits == 32)
        hipLaunchKernelGGL(k_runs<int32_t>, grid, block, 0, ctx->stream, dk.p, dh.p, dd.p, n, dn.p, ds.p, dm.p, dl.p);
    else
        hipLaunchKernelGGL(k_runs<int64_t>, grid, block, 0, ctx->stream, dk.p, dh.p, dd.p, n, dn.p, ds.p, dm.p, dl.p);
    MR_TRY(dn.download(ctx, (unsigned long long*)out_n, (size_t)n));
    MR_TRY(ds.download(ctx, (unsigned long long*)out_sum, (size_t)n));
    MR_TRY(dm.download(ctx, (unsigned long long*)out_max, (size_t)n));
    MR_TRY(dl.download(ctx, out_last, (size_t)n));
    return sync(ctx);
}

// One EvTable launch: `blocks` blocks of `tiles` 256-row tiles each over keys / d [n] (a key < 0: the row
// brings nothing), every block with its own table, into zeroed dense counters cnt [n_keys * 3].  direct:
// the keys are below EV_H.  K as mrt_runs'.
int mrt_evtable(mr_ctx* ctx, int key_bits, int direct, const int64_t* keys, const uint64_t* d, int64_t n, int64_t n_keys,
                int blocks, int tiles, uint64_t* cnt) {
    if (!ctx || (key_bits != 32 && key_bits != 64) || n < 1 || !keys || !d || n_keys < 1 || blocks < 1 || tiles < 1 || !cnt ||
        (int64_t)blocks * tiles * ST_T < n)
        return mr_fail(ctx, MR_ERR_ARG, "mrt_evtable: bad arguments");
    const int64_t kmax = direct ? std::min<int64_t>(n_keys, EV_H) : key_bits == 32 ? std::min<int64_t>(n_keys, INT32_MAX) : n_keys;
    for (int64_t i = 0; i < n; ++i)
        if (keys[i] >= kmax) return mr_fail(ctx, MR_ERR_ARG, "mrt_evtable: key %lld is not below %lld", (long long)keys[i], (long long)kmax);
    DBuf<int64_t> dk;
    DBuf<unsigned long long> dd, dc;
    MR_TRY(dk.upload(ctx, keys, (size_t)n));
    MR_TRY(dd.upload(ctx, (const unsigned long long*)d, (size_t)n));
    MR_TRY(dc.zero(ctx, (size_t)n_keys * 3));
    const dim3 grid((unsigned)blocks), block(ST_T);
    if (key_bits == 32)
        hipLaunchKernelGGL(k_evtable<int32_t>, grid, block, 0, ctx->stream, dk.p, dd.p, n, direct, tiles, dc.p);
    else
        hipLaunchKernelGGL(k_evtable<int64_t>, grid, block, 0, ctx->stream, dk.p, dd.p, n, direct, tiles, dc.p);
    MR_TRY(dc.download(ctx, (unsigned long long*)cnt, (size_t)n_keys * 3));
    return sync(ctx);
}

// in / out: n 8-byte words (doubles; int64 for op 4), n a multiple of `block` (64, 256 or 1024 threads):
// a block per `block` words, out[i] what thread i holds after the reduction (k_block_reduce's ops)
int mrt_block_reduce(mr_ctx* ctx, int op, int block, const void* in, int64_t n, void* out) {
    if (!ctx || op < 0 || op > 4 || (block != 64 && block != 256 && block != 1024) || n < 1 || n % block || !in || !out)
        return mr_fail(ctx, MR_ERR_ARG, "mrt_block_reduce: bad arguments");
    DBuf<double> di, dout;
    MR_TRY(di.upload(ctx, (const double*)in, (size_t)n));
    MR_TRY(dout.alloc(ctx, (size_t)n));
    hipLaunchKernelGGL(k_block_reduce, dim3((unsigned)(n / block)), dim3(block), 0, ctx->stream, op, di.p, dout.p);
    MR_TRY(dout.download(ctx, (double*)out, (size_t)n));
    return sync(ctx);
}

// out[b] = the descriptor owning block b, b in [0, n_blocks), for the n non-decreasing starts `first`
int mrt_block_owner(mr_ctx* ctx, const int32_t* first, int32_t n, int32_t n_blocks, int32_t* out) {
    if (!ctx || !first || n < 1 || n_blocks < 1 || !out) return mr_fail(ctx, MR_ERR_ARG, "mrt_block_owner: bad arguments");
    std::vector<OwnerD> h((size_t)n);
    for (int32_t i = 0; i < n; ++i) h[(size_t)i] = OwnerD{~i, first[i]};
    DBuf<OwnerD> dd;
    DBuf<int32_t> dout;
    MR_TRY(dd.upload(ctx, h.data(), (size_t)n));
    MR_TRY(dout.alloc(ctx, (size_t)n_blocks));
    hipLaunchKernelGGL(k_block_owner, dim3(cdiv(n_blocks, 256)), dim3(256), 0, ctx->stream, dd.p, n, n_blocks, dout.p);
    MR_TRY(dout.download(ctx, out, (size_t)n_blocks));
    return sync(ctx);
}

}  // extern "C"
