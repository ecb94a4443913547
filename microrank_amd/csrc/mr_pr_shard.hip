// Trace-sharded graphs for K2 (mr_pagerank_sharded): the exchange that makes a rank's shard rank as
// the whole graph does -- the op constants and call edges over the ranks (shard_exchange) and the
// kind classes (pagerank.py:54-66) merged across ranks (shard_kinds).  The sharded iteration itself:
// iterate (mr_pagerank.hip) around k_fx_b's / k_iter_b's modes 1 and 2 (mr_pr_fxb_dev.h,
// mr_pr_tile_dev.h); the collectives: mr_comm.hip.
#include <algorithm>

#include "mr_pr_dev.h"
#include "mr_pr_internal.h"
#include "mr_sort.h"

namespace {

__global__ void k_op_consts(const int32_t* len_o, const int32_t* nchild, float* u_o, float* pw, int32_t N) {
    int32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= N) return;
    u_o[o] = len_o[o] > 0 ? (float)(1.0 / (double)len_o[o]) : 0.0f;
    pw[o] = nchild[o] > 0 ? (float)(1.0 / (double)nchild[o]) : 0.0f;
}

// ---------------------------------------------------------------- trace-sharded graphs
// local call edges (child, parent) as sort keys c << nb | p
__global__ void k_sh_edge_keys(const int64_t* ss_off, const int32_t* ss_par, int32_t N, int nb, uint64_t* key) {
    const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    for (int64_t e = ss_off[c]; e < ss_off[c + 1]; ++e) key[e] = ((uint64_t)c << nb) | (uint32_t)ss_par[e];
}
__global__ void k_sh_pad(uint64_t* key, int64_t from, int64_t to, uint64_t pad) {
    const int64_t i = from + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < to) key[i] = pad;
}
// heads of distinct real keys in the sorted union (pads sort last and are dropped)
__global__ void k_sh_edge_heads(const uint64_t* key, int64_t n, uint64_t pad, int32_t* head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head[i] = key[i] != pad && (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}
__global__ void k_sh_edge_out(const uint64_t* key, const int32_t* head, const int64_t* pos, int64_t n, int nb,
                              int32_t* ss_par, int32_t* ccount) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    ss_par[pos[i]] = (int32_t)(key[i] & ((1ull << nb) - 1ull));
    atomicAdd(&ccount[(int32_t)(key[i] >> nb)], 1);
}
// this rank's kind classes as (key, check hash of the representative, count); empty slots skipped
__global__ void k_sh_kind_list(const unsigned long long* hk, const KCnt* cr, const uint64_t* hchk, int64_t cap, const int32_t* flag,
                               const int64_t* pos, uint64_t* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || !flag[i]) return;
    const int64_t p = pos[i];
    out[3 * p] = hk[i];
    out[3 * p + 1] = hchk[i];   // k_kind_insert<true>: the representative's check hash
    out[3 * p + 2] = cr[i].cnt;
}
__global__ void k_sh_kind_flags(const unsigned long long* hk, int64_t cap, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) flag[i] = hk[i] != 0ull;
}
// all ranks' lists into one table: counts summed per key; a key whose check hash differs
// between ranks is a 64-bit collision across ranks -> flag
__global__ void k_sh_kind_merge(const uint64_t* in, int64_t n, uint64_t* gk, uint64_t* gh, unsigned long long* gc,
                                uint64_t mask, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = in[3 * i];
    if (!k) return;
    uint64_t s = mix64(k) & mask;
    for (;;) {
        const unsigned long long old = atomicCAS((unsigned long long*)&gk[s], 0ull, (unsigned long long)k);
        if (old == 0ull) {
            gh[s] = in[3 * i + 1];   // first writer; later writers compare after the table settles
            break;
        }
        if (old == k) break;
        s = (s + 1) & mask;
    }
    atomicAdd(&gc[s], (unsigned long long)in[3 * i + 2]);
}
__global__ void k_sh_kind_check(const uint64_t* in, int64_t n, const uint64_t* gk, const uint64_t* gh, uint64_t mask,
                                int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !in[3 * i]) return;
    const uint64_t k = in[3 * i];
    uint64_t s = mix64(k) & mask;
    while (gk[s] != k) s = (s + 1) & mask;
    if (gh[s] != in[3 * i + 1]) atomicOr(flag, 1);
}
// ---- the kind-class exchange partitioned by key (peer regions): a class key is OWNED by rank
// owner(key); every rank sends its (key, check hash, count) records to their owners, each owner
// sums the counts of the keys it owns and returns every record's total to its sender
__device__ __forceinline__ int kind_owner(uint64_t key, int R) { return (int)((mix64(key ^ 0x5bd1e995ull) >> 33) % (uint64_t)R); }
__global__ void k_kx_count(const uint64_t* rec, int64_t n, int R, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&cnt[kind_owner(rec[3 * i], R)], 1ull);
}
// records by owner: record i -> send slot spos[i] (order inside an owner's run arbitrary: the
// owner's sums and the returned totals do not depend on it)
__global__ void k_kx_place(const uint64_t* rec, int64_t n, int R, unsigned long long* cursor, uint64_t* send,
                           int64_t* spos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t p = (int64_t)atomicAdd(&cursor[kind_owner(rec[3 * i], R)], 1ull);
    send[3 * p] = rec[3 * i];
    send[3 * p + 1] = rec[3 * i + 1];
    send[3 * p + 2] = rec[3 * i + 2];
    spos[i] = p;
}
// the owner's totals back to the senders: received record j came from rank s (roff: first record of
// each source) and goes to slot soff_at_s + (j - roff[s]) of s's area B
__global__ void k_kx_return(const uint64_t* in, int64_t n, const uint64_t* gk, const unsigned long long* gc, uint64_t mask,
                            const int64_t* roff, const int64_t* dbase, int R, unsigned long long* const* areas) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t k = in[3 * j];
    uint64_t s = mix64(k) & mask;
    while (gk[s] != k) s = (s + 1) & mask;
    int src = 0;
    while (src + 1 < R && roff[src + 1] <= j) ++src;
    __hip_atomic_store((__attribute__((address_space(1))) unsigned long long*)areas[src] + dbase[src] + (j - roff[src]),
                       gc[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// kind[t] = the returned total of its class's record
__global__ void k_kx_apply(const unsigned long long* hk, const int32_t* slot_of, const int32_t* flag, const int64_t* pos,
                           const int64_t* spos, const unsigned long long* ret, int32_t T, double* kind) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int32_t sl = slot_of[t];
    (void)hk;
    (void)flag;
    kind[t] = (double)ret[spos[pos[sl]]];
}
// kind[t] = the class size over all ranks
__global__ void k_sh_kind_apply(const unsigned long long* hk, const int32_t* slot_of, int32_t T, const uint64_t* gk,
                                const unsigned long long* gc, uint64_t mask, double* kind) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t k = hk[slot_of[t]];
    uint64_t s = mix64(k) & mask;
    while (gk[s] != k) s = (s + 1) & mask;
    kind[t] = (double)gc[s];
}

}  // namespace

// ------------------------------------------------------------------------------ sharded graphs
// the kind classes over the ranks through the peer regions: records partitioned by owner (one
// exchange round), merged by their owners, totals returned (a second round).  Each rank sends and
// receives ~ its own class count, instead of receiving every rank's list (the all-gather below).
static int shard_kinds_peer(mr_ctx* ctx, mr_graph* g, uint64_t cap, const DBuf<int32_t>& fl, const DBuf<int64_t>& pos,
                            int64_t Kl) {
    hipStream_t st = ctx->stream;
    const int32_t T = g->T;
    const int R = ctx->nranks, me = ctx->rank;
    DBuf<uint64_t> rec, send;
    DBuf<int64_t> spos;
    DBuf<unsigned long long> cnt;
    MR_TRY(rec.alloc(ctx, (size_t)3 * std::max<int64_t>(Kl, 1)));
    MR_TRY(send.alloc(ctx, (size_t)3 * std::max<int64_t>(Kl, 1)));
    MR_TRY(spos.alloc(ctx, (size_t)std::max<int64_t>(Kl, 1)));
    MR_TRY(cnt.zero(ctx, (size_t)R));
    hipLaunchKernelGGL(k_sh_kind_list, dim3(cdiv(cap, 256)), dim3(256), 0, st, g->ht_key.p, g->ht_cr.p, g->ht_chk.p,
                       (int64_t)cap, fl.p, pos.p, rec.p);
    if (Kl) hipLaunchKernelGGL(k_kx_count, dim3(cdiv(Kl, 256)), dim3(256), 0, st, rec.p, Kl, R, cnt.p);
    std::vector<int64_t> scnt((size_t)R), M((size_t)R * R);
    MR_TRY_HIP(ctx, hipMemcpyAsync(scnt.data(), cnt.p, sizeof(int64_t) * R, hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    std::vector<int64_t> soff((size_t)R + 1, 0);
    for (int o = 0; o < R; ++o) soff[(size_t)o + 1] = soff[(size_t)o] + scnt[(size_t)o];
    MR_TRY(cnt.upload(ctx, (const unsigned long long*)soff.data(), (size_t)R));   // cursors
    if (Kl) hipLaunchKernelGGL(k_kx_place, dim3(cdiv(Kl, 256)), dim3(256), 0, st, rec.p, Kl, R, cnt.p, send.p, spos.p);
    {   // every rank's counts per owner: M[s * R + o]
        DBuf<int64_t> mine, all;
        MR_TRY(mine.upload(ctx, scnt.data(), (size_t)R));
        MR_TRY(all.alloc(ctx, (size_t)R * R));
        MR_TRY(mr_coll_allgather(ctx, mine.p, all.p, R, MR_DT_I64));
        MR_TRY(all.download(ctx, M.data(), (size_t)R * R));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    }
    int64_t xa = 1, xb = 1;   // words: area A receives 3 per record owned, area B one total per record sent
    for (int o = 0; o < R; ++o) {
        int64_t in = 0, out = 0;
        for (int s = 0; s < R; ++s) {
            in += M[(size_t)s * R + o];
            out += M[(size_t)o * R + s];
        }
        xa = std::max(xa, 3 * in);
        xb = std::max(xb, out);
    }
    MR_TRY(mr_peer_xensure(ctx, xa, xb));
    // round 1: my records to their owners' areas A (after the records of lower ranks)
    for (int o = 0; o < R; ++o) {
        int64_t at = 0;
        for (int s = 0; s < me; ++s) at += M[(size_t)s * R + o];
        MR_TRY(mr_peer_put(ctx, (const unsigned long long*)send.p + 3 * soff[(size_t)o], 3 * scnt[(size_t)o], o, 0, 3 * at));
    }
    MR_TRY(mr_peer_round(ctx));
    // merge the records I own
    std::vector<int64_t> roff((size_t)R + 1, 0), dbase((size_t)R);
    for (int s = 0; s < R; ++s) {
        roff[(size_t)s + 1] = roff[(size_t)s] + M[(size_t)s * R + me];
        int64_t b = 0;   // where s keeps the totals of its records for me: its send offset of owner me
        for (int o = 0; o < me; ++o) b += M[(size_t)s * R + o];
        dbase[(size_t)s] = b;
    }
    const int64_t n = roff[(size_t)R];
    const uint64_t* in = (const uint64_t*)mr_peer_area(ctx, me, 0);
    uint64_t gcap = 1;
    while (gcap < 2 * (uint64_t)std::max<int64_t>(n, 1)) gcap <<= 1;
    DBuf<uint64_t> gk, gh;
    DBuf<unsigned long long> gc;
    DBuf<int64_t> droff, ddbase;
    MR_TRY(gk.zero(ctx, gcap));
    MR_TRY(gh.zero(ctx, gcap));
    MR_TRY(gc.zero(ctx, gcap));
    MR_TRY(droff.upload(ctx, roff.data(), roff.size()));
    MR_TRY(ddbase.upload(ctx, dbase.data(), dbase.size()));
    std::vector<unsigned long long*> areas((size_t)R);
    for (int s = 0; s < R; ++s) areas[(size_t)s] = mr_peer_area(ctx, s, 1);
    DBuf<unsigned long long*> dareas;
    MR_TRY(dareas.upload(ctx, areas.data(), areas.size()));
    if (n) {
        hipLaunchKernelGGL(k_sh_kind_merge, dim3(cdiv(n, 256)), dim3(256), 0, st, in, n, gk.p, gh.p, gc.p, gcap - 1,
                           g->flag.p);
        hipLaunchKernelGGL(k_sh_kind_check, dim3(cdiv(n, 256)), dim3(256), 0, st, in, n, gk.p, gh.p, gcap - 1, g->flag.p);
        // round 2: every record's total back to its sender's area B
        hipLaunchKernelGGL(k_kx_return, dim3(cdiv(n, 256)), dim3(256), 0, st, in, n, gk.p, gc.p, gcap - 1, droff.p,
                           ddbase.p, R, dareas.p);
    }
    MR_TRY(mr_peer_round(ctx));
    if (T)
        hipLaunchKernelGGL(k_kx_apply, dim3(cdiv(T, 256)), dim3(256), 0, st, g->ht_key.p, g->slot_of.p, fl.p, pos.p,
                           spos.p, (const unsigned long long*)mr_peer_area(ctx, me, 1), T, g->kind.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    return mr_peer_check(ctx, "kind exchange");   // (syncs: the scratch leaves scope)
}

int shard_kinds(mr_ctx* ctx, mr_graph* g, uint64_t cap) {
    hipStream_t st = ctx->stream;
    const int32_t T = g->T;
    DBuf<int32_t> fl;
    DBuf<int64_t> pos, tmp;
    MR_TRY(fl.alloc(ctx, cap));
    MR_TRY(pos.alloc(ctx, cap + 1));
    MR_TRY(tmp.alloc(ctx, scan_tmp_elems((int64_t)cap)));
    hipLaunchKernelGGL(k_sh_kind_flags, dim3(cdiv(cap, 256)), dim3(256), 0, st, g->ht_key.p, (int64_t)cap, fl.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, fl.p, pos.p, (int64_t)cap, tmp.p));
    DBuf<int64_t> kn;
    MR_TRY(kn.alloc(ctx, 1));
    MR_TRY_HIP(ctx, hipMemcpyAsync(kn.p, pos.p + cap, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    int64_t Kl = 0;
    MR_TRY(kn.download(ctx, &Kl, 1));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    if (mr_peer_ready(ctx)) {   // MR_ERR_STATE: the ranks could not map each other's regions (collective)
        const int rc = shard_kinds_peer(ctx, g, cap, fl, pos, Kl);
        if (rc != MR_ERR_STATE) return rc;
    }
    MR_TRY(mr_coll_allreduce(ctx, kn.p, 1, MR_DT_I64, 1));
    int64_t Kmax = 0;
    MR_TRY(kn.download(ctx, &Kmax, 1));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    const int R = ctx->nranks;
    DBuf<uint64_t> send, recv;
    MR_TRY(send.zero(ctx, (size_t)3 * std::max<int64_t>(Kmax, 1)));
    MR_TRY(recv.alloc(ctx, (size_t)3 * std::max<int64_t>(Kmax, 1) * R));
    hipLaunchKernelGGL(k_sh_kind_list, dim3(cdiv(cap, 256)), dim3(256), 0, st, g->ht_key.p, g->ht_cr.p, g->ht_chk.p,
                       (int64_t)cap, fl.p, pos.p, send.p);
    MR_TRY(mr_coll_allgather(ctx, send.p, recv.p, 3 * std::max<int64_t>(Kmax, 1), MR_DT_U64));
    const int64_t n = std::max<int64_t>(Kmax, 1) * R;
    uint64_t gcap = 1;
    while (gcap < 2 * (uint64_t)n) gcap <<= 1;
    DBuf<uint64_t> gk, gh;
    DBuf<unsigned long long> gc;
    MR_TRY(gk.zero(ctx, gcap));
    MR_TRY(gh.zero(ctx, gcap));
    MR_TRY(gc.zero(ctx, gcap));
    hipLaunchKernelGGL(k_sh_kind_merge, dim3(cdiv(n, 256)), dim3(256), 0, st, recv.p, n, gk.p, gh.p, gc.p, gcap - 1,
                       g->flag.p);
    hipLaunchKernelGGL(k_sh_kind_check, dim3(cdiv(n, 256)), dim3(256), 0, st, recv.p, n, gk.p, gh.p, gcap - 1, g->flag.p);
    if (T)
        hipLaunchKernelGGL(k_sh_kind_apply, dim3(cdiv(T, 256)), dim3(256), 0, st, g->ht_key.p, g->slot_of.p, T, gk.p,
                           gc.p, gcap - 1, g->kind.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // scratch leaves scope
    return MR_OK;
}

// once per graph: per-op sums, the union of the call edges, the number of traces
int shard_exchange(mr_ctx* ctx, mr_graph* g) {
    hipStream_t st = ctx->stream;
    const int32_t N = g->N;
    MR_TRY(mr_coll_allreduce(ctx, g->len_o.p, N, MR_DT_I32, 0));
    MR_TRY(mr_coll_allreduce(ctx, g->nchild.p, N, MR_DT_I32, 0));
    MR_TRY(mr_coll_allreduce(ctx, g->cov.p, N, MR_DT_I32, 0));
    if (N) hipLaunchKernelGGL(k_op_consts, dim3(cdiv(N, 256)), dim3(256), 0, st, g->len_o.p, g->nchild.p, g->u_o.p, g->pw.p, N);
    const int R = ctx->nranks;
    DBuf<int64_t> sc, tc;
    int64_t h[2] = {(int64_t)g->T, g->E};
    MR_TRY(sc.upload(ctx, h, 2));
    MR_TRY(tc.alloc(ctx, (size_t)R));
    // every rank's trace count: their sum is the whole graph's T, the lower ranks' the global id of
    // this shard's first trace (mr_graph_trace_rank_sharded)
    MR_TRY(mr_coll_allgather(ctx, sc.p, tc.p, 1, MR_DT_I64));
    MR_TRY(mr_coll_allreduce(ctx, sc.p + 1, 1, MR_DT_I64, 1));   // largest local edge list
    std::vector<int64_t> tr((size_t)R);
    MR_TRY(tc.download(ctx, tr.data(), (size_t)R));
    MR_TRY(sc.download(ctx, h, 2));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    g->T_all = g->t_base = 0;
    for (int r = 0; r < R; ++r) {
        if (r < ctx->rank) g->t_base += tr[(size_t)r];
        g->T_all += tr[(size_t)r];
    }
    const int64_t Emax = std::max<int64_t>(h[1], 1);
    const int nb = std::max(1, bits_for((uint64_t)std::max(N - 1, 0)));
    const uint64_t pad = 1ull << (2 * nb);   // above every real key
    DBuf<uint64_t> send, recv;
    MR_TRY(send.alloc(ctx, (size_t)Emax));
    MR_TRY(recv.alloc(ctx, (size_t)Emax * R));
    if (N) hipLaunchKernelGGL(k_sh_edge_keys, dim3(cdiv(N, 256)), dim3(256), 0, st, g->ss_off.p, g->ss_par.p, N, nb, send.p);
    if (Emax > g->E) hipLaunchKernelGGL(k_sh_pad, dim3(cdiv(Emax - g->E, 256)), dim3(256), 0, st, send.p, g->E, Emax, pad);
    MR_TRY(mr_coll_allgather(ctx, send.p, recv.p, Emax, MR_DT_U64));
    const int64_t n = Emax * R;
    SortScratch ws;
    MR_TRY(mr_radix_sort(ctx, recv.p, nullptr, n, 2 * nb + 1, ws));
    DBuf<int32_t> head, ccount;
    DBuf<int64_t> pos, tmp;
    MR_TRY(head.alloc(ctx, n));
    MR_TRY(pos.alloc(ctx, n + 1));
    MR_TRY(tmp.alloc(ctx, std::max(scan_tmp_elems(n), scan_tmp_elems(std::max(N, 1)))));
    hipLaunchKernelGGL(k_sh_edge_heads, dim3(cdiv(n, 256)), dim3(256), 0, st, recv.p, n, pad, head.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, head.p, pos.p, n, tmp.p));
    int64_t E = 0;
    MR_TRY_HIP(ctx, hipMemcpyAsync(&E, pos.p + n, sizeof E, hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    MR_TRY(ccount.zero(ctx, N));
    g->ss_par.reset();
    MR_TRY(g->ss_par.alloc(ctx, (size_t)std::max<int64_t>(E, 1)));
    hipLaunchKernelGGL(k_sh_edge_out, dim3(cdiv(n, 256)), dim3(256), 0, st, recv.p, head.p, pos.p, n, nb, g->ss_par.p,
                       ccount.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, ccount.p, g->ss_off.p, N, tmp.p));
    g->E = E;
    MR_TRY_HIP(ctx, hipGetLastError());
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    return MR_OK;
}
