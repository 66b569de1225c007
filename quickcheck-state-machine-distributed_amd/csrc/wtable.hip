// wtable.hip -- QSMD_MODEL_WTABLE: table.hip's search for a model too large
// for LDS (include/qsmd.h qsmd_wtable_model): up to 65,536 states, 256
// invocation and 256 response symbols.  The semantics are model 3's,
//     post  = bit r of post[s][i]            (word r >> 5, bit r & 31)
//     raise = bit r of post_err[s][i]
//     next  = on_resp[on_inv[s][i]][r]
// and so is the structure: one lane per history over the Lemma L1 bitsets and
// seven pid planes (table_lane.h), three width classes, pass 1 with
// "table_budget", pass 2 grid-stride over the heavy list from the root, the
// optional state memo, a finish kernel.  Three things differ:
//   * the tables are read from device memory (internal.h WTableDev: one
//     record per (state, invocation) holding on_inv and the postcondition
//     words).  Given (state, i, rc) the record's on_inv word, its post word
//     rc >> 5 and (only when the model has one) its post_err word are
//     independent loads issued together; on_resp is the one dependent load;
//   * a state has 16 bits, so the DFS stack is one 32-bit word per level
//     (event 8 | state before the step 16), [level][lane]: bank lane % 32
//     whatever the level.  The events stay 16 bits in col16's paired words;
//   * the memo's tag word is epoch 16 | state 16 (table.hip: 24 | 8).
// LDS per workgroup: 4 / 8 / 16 KB of events and as much of stack (with the
// memo, 8 / 16 / 32 KB of node counts more); no table.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "lane.h"
#include "mask.h"
#include "table_lane.h"

namespace qsmd {

namespace {

using namespace tlane;

// One lane's search state (registers) over its LDS columns: table.hip's
// TableDFS with the wide step.
template <class M>
struct WTableDFS {
    using MO = MaskOps<M>;
    M INV, RESP, P[7];
    M rem, cand;
    uint32_t state, depth, found;
    uint64_t nodes;

    __device__ __forceinline__ M same_pid(uint32_t j) const {
        M acc = t_ones<M>();
#pragma unroll
        for (int b = 0; b < 7; ++b) acc = acc & (t_test(P[b], j) ? P[b] : ~P[b]);
        return acc;
    }

    __device__ __forceinline__ void init(uint32_t state0) {
        rem = INV | RESP;
        cand = t_cands(rem, INV, RESP);
        state = state0;
        depth = 0;
        found = 0;
        nodes = 0;
    }

    static constexpr int kTerm = 64;
    __device__ __forceinline__ int finish(int status) const {
        return status != kTerm ? status
                               : ((!found && depth > 0) ? QSMD_STATUS_LINEARISABLE : QSMD_STATUS_NONLINEARISABLE);
    }

    // One iteration: TableDFS::step with the tables in device memory and the
    // 32-bit stack.  Returns -1 = go on, kTerm, QSMD_STATUS_BUDGET or
    // QSMD_STATUS_MODEL_ERROR.
    // EXPLAIN (the explain calls, never with MEMO): xp records the deepest
    // path into `path` (DeepPath, table_lane.h).
    template <bool MEMO, bool EXPLAIN>
    __device__ __forceinline__ int step(const WTableDev& t, const uint16_t* on_resp, const uint16_t* ev,
                                        uint32_t* stk, int lane, uint64_t limit, TableMemo<M>& mm,
                                        DeepPath<uint32_t>& xp, uint8_t* path) {
        const bool empty = !MO::any(cand);
        if (empty && (found == 0u || depth == 0u)) return kTerm;
        if (empty) {
            --depth;
            if constexpr (EXPLAIN) xp.fell_to(depth);
            if constexpr (MEMO) {
                if (!mm.skip) mm.record(rem, state, nodes - mm.entry[depth * C_LANES]);
                mm.skip = false;
            }
            const uint32_t st = stk[depth * C_LANES + lane];
            const uint32_t j = st & 0xFFu;
            state = st >> 8;
            const M gone = ~rem & same_pid(j);
            rem = rem | t_topbit<M>(gone & INV) | t_topbit<M>(gone & RESP);
            cand = t_cands(rem, INV, RESP) & ~MO::below((int)j + 1);
            found = 1u;
            if (!MO::any(cand)) return -1;
        }
        const uint32_t j = (uint32_t)MO::ctz(cand);
        cand = MO::clear_lowest(cand);
        const M pmj = same_pid(j);
        const M rr = rem & pmj & RESP;
        if (!MO::any(rr)) return -1;             // findResponse => []: no child, no node
        if (nodes >= limit) return QSMD_STATUS_BUDGET;
        const uint32_t r = (uint32_t)MO::ctz(rr);
        const uint32_t i = ev[col16(j, lane)] >> 8, rc = ev[col16(r, lane)] >> 8;
        // the record of (state, i): three independent loads, post_err's only
        // when the model has one (a uniform condition)
        const uint32_t* rec = t.blob + (state * t.n_inv + i) * t.rec_words;
        const uint32_t w = rc >> 5, b = rc & 31u;
        const uint32_t mid = rec[0];
        const uint32_t pw = rec[1u + w];
        const uint32_t ew = t.has_err ? rec[1u + t.post_words + w] : 0u;
        ++nodes;
        found = 1u;
        if ((ew >> b) & 1u) return QSMD_STATUS_MODEL_ERROR;
        if ((pw >> b) & 1u) {
            stk[depth * C_LANES + lane] = j | (state << 8);
            ++depth;
            state = on_resp[mid * t.n_resp + rc];
            rem = rem & ~(MO::lowest(rem & pmj & INV) | MO::bit((int)r));
            cand = t_cands(rem, INV, RESP);
            found = 0u;
            if constexpr (EXPLAIN)
                xp.descended(path, depth, state, [&](uint32_t d) { return stk[d * C_LANES + lane] & 0xFFu; });
            if constexpr (MEMO) {
                mm.entry[(depth - 1u) * C_LANES] = nodes;
                uint64_t c;
                if (mm.probe(rem, state, c)) {
                    ++mm.hits;
                    uint64_t sum;
                    if (__builtin_add_overflow(nodes, c, &sum) || sum > limit) {   // the budget falls inside that subtree
                        nodes = limit;
                        return QSMD_STATUS_BUDGET;
                    }
                    nodes = sum;                 // the subtree's nodes, counted; it failed
                    cand = t_zero<M>();
                    found = 1u;
                    mm.skip = true;
                }
            }
        }
        return -1;
    }
};

// table.hip's table_bin for model id 4
__global__ __launch_bounds__(C_LANES) void wtable_bin(WTableArgs a) {
    const int lane = threadIdx.x;
    WaveCounters cnt;
    for (uint64_t base = (uint64_t)blockIdx.x * C_LANES; base < a.s.n_hist; base += (uint64_t)gridDim.x * C_LANES) {
        const uint64_t h = base + lane;
        const bool active = h < a.s.n_hist;
        qsmd_hdr H{0, 0, 0, 0, 0, 0};
        if (active) H = a.s.hdr[h];
        const bool enc_ok = H.model_id == QSMD_MODEL_WTABLE && H.n_ev <= QSMD_MAX_EVENTS &&
                            (uint64_t)H.ev_off + H.n_ev <= a.s.n_events;
        const bool out = active && (!enc_ok || H.n_ev == 0);
        const int status = enc_ok ? QSMD_STATUS_LINEARISABLE : QSMD_STATUS_ENCODE_ERROR;   // src/Linearisability.hs:59
        if (out) {
            a.s.status[h] = (uint8_t)status;
            if (a.s.nodes) a.s.nodes[h] = 0;
        }
        cnt.add(out, status, 0);
        const bool go = active && !out;
        wave_append(go && H.n_ev <= 32u, (uint32_t)h, a.class_list[0], a.cnt + TC_CLASS + 0, lane);
        wave_append(go && H.n_ev > 32u && H.n_ev <= 64u, (uint32_t)h, a.class_list[1], a.cnt + TC_CLASS + 1, lane);
        wave_append(go && H.n_ev > 64u, (uint32_t)h, a.class_list[2], a.cnt + TC_CLASS + 2, lane);
    }
    cnt.flush(a.s.buckets, lane);
}

// table.hip's table_search: PASS2 false = the class list with the pass-1
// budget, true = the class's heavy list to the end; MEMO = pass 2 with the
// state memo.
template <class M, bool MEMO, bool EXPLAIN>
__global__ __launch_bounds__(C_LANES) void wtable_search(WTableArgs a, uint32_t pass2) {
    constexpr int EV = TW<M>::EV, K = TW<M>::CLASS;
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const uint32_t* list = pass2 ? a.heavy_list[K] : a.class_list[K];
    const uint32_t total = a.cnt[(pass2 ? TC_HEAVY : TC_CLASS) + K];
    if ((uint64_t)blockIdx.x * C_LANES >= total) return;

    // LDS: events [EV / 2][64] words, stack [EV / 2][64] words, (MEMO: the
    // node counts at entry, [EV / 2][64] u64)
    uint16_t* ev = reinterpret_cast<uint16_t*>(lds);
    uint32_t* stk = lds + (EV / 2) * C_LANES;
    TableMemo<M> mm;
    if constexpr (MEMO) {
        mm.entry = reinterpret_cast<uint64_t*>(lds + EV * C_LANES) + lane;
        mm.tab = a.memo + ((uint64_t)blockIdx.x * C_LANES + (uint64_t)lane) * (uint64_t)a.memo_entries * 2ull;
        mm.mask = a.memo_entries - 1u;
        mm.tag = a.memo_epoch << 16;
        mm.hits = 0u;
    }
    const uint16_t* on_resp = reinterpret_cast<const uint16_t*>(a.t.blob + a.t.on_resp_off);

    WaveCounters cnt;
    const uint64_t t0 = a.s.time_limit ? __builtin_amdgcn_s_memrealtime() : 0;
    const uint64_t user_limit = a.s.max_nodes ? a.s.max_nodes : ~0ull;
    const bool tiered = !pass2 && a.budget && a.budget < user_limit;
    const uint64_t limit = tiered ? a.budget : user_limit;

    for (uint64_t base = (uint64_t)blockIdx.x * C_LANES; base < total; base += (uint64_t)gridDim.x * C_LANES) {
        const uint64_t idx = base + lane;
        const bool active = idx < total;
        const uint32_t h = active ? list[idx] : 0u;
        qsmd_hdr H{0, 0, 0, 0, 0, 0};
        if (active) H = a.s.hdr[h];
        WTableDFS<M> dfs;
        dfs.depth = 0;
        dfs.nodes = 0;
        dfs.found = 0;
        // -2: no history in this lane
        int status = -2;
        if (active) {
            status = stage_table<M>(a, H, ev, lane, dfs) ? -1 : QSMD_STATUS_ENCODE_ERROR;
            if (status == -1) dfs.init(a.state0);
        }
        if constexpr (MEMO) mm.begin(h);
        DeepPath<uint32_t> xp;
        if constexpr (EXPLAIN) xp.begin(H.ev_off, a.state0);
        // the search, the time limit checked every 1024 iterations (a
        // wavefront-uniform counter: the loop runs while any lane searches)
        while (__ballot(status == -1) != 0ull) {
            for (uint32_t k = 0; k < 1024u; ++k) {
                if (status == -1)
                    status = dfs.template step<MEMO, EXPLAIN>(a.t, on_resp, ev, stk, lane, limit, mm, xp, a.path);
                if (__ballot(status == -1) == 0ull) break;
            }
            if (status == -1 && a.s.time_limit && __builtin_amdgcn_s_memrealtime() - t0 > a.s.time_limit) {
                atomicOr(a.s.timed_out, 1u);
                status = QSMD_STATUS_BUDGET;
            }
        }
        if (status >= 0) status = dfs.finish(status);
        // over pass 1's budget (not the caller's): pass 2 searches it again
        const bool heavy = tiered && status == QSMD_STATUS_BUDGET && dfs.nodes >= limit;
        wave_append(heavy, h, a.heavy_list[K], a.cnt + TC_HEAVY + K, lane);
        const bool out = active && !heavy;
        if (out) {
            a.s.status[h] = (uint8_t)status;
            if (a.s.nodes) a.s.nodes[h] = dfs.nodes;
            if (a.s.witness && status == QSMD_STATUS_LINEARISABLE) {
                uint8_t* w = a.s.witness + H.ev_off;
                for (uint32_t d = 0; d < dfs.depth; ++d) w[d] = (uint8_t)(stk[d * C_LANES + lane] & 0xFFu);
                if (dfs.depth < H.n_ev) w[dfs.depth] = QSMD_WITNESS_END;
            }
        }
        if constexpr (EXPLAIN) {
            const auto at = [&](uint32_t d) { return stk[d * C_LANES + lane] & 0xFFu; };
            if (out) xp.finish(a.path, status, H.n_ev, dfs.depth, dfs.state, at, a.explain + h);
        }
        cnt.add(out, status, dfs.nodes);
        if constexpr (MEMO) {
            // the group's hits: one atomic per wavefront
            const uint64_t hits = wave_sum64(mm.hits);
            mm.hits = 0u;
            if (lane == 0 && hits)
                __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a.cnt + TC_HITS), (unsigned long long)hits,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    cnt.flush(a.s.buckets, lane);
}

// The call's totals from the buckets, the probe for the host (table.hip's
// table_finish).
__global__ __launch_bounds__(C_LANES) void wtable_finish(WTableArgs a) {
    const uint32_t k = threadIdx.x;
    if (k < (uint32_t)T_N) {
        uint64_t v = 0;
        for (uint32_t b = 0; b < kBuckets; ++b) v += a.s.buckets[(uint64_t)b * kBucketWords + k];
        reinterpret_cast<uint64_t*>(a.totals)[k] = v;
    }
    if (k == 0 && a.probe_host) {
        a.probe_host[C_TIMED] = a.cnt[TC_TIMED];
        a.probe_host[kProbeTabPass2] = a.cnt[TC_HEAVY] + a.cnt[TC_HEAVY + 1] + a.cnt[TC_HEAVY + 2];
        for (int c = 0; c < 3; ++c) a.probe_host[kProbeTabClass + c] = a.cnt[TC_CLASS + c];
        a.probe_host[kProbeTabHits] = a.cnt[TC_HITS];
        a.probe_host[kProbeTabHits + 1] = a.cnt[TC_HITS + 1];
        __threadfence_system();
    }
}

// (at most 64 KB, the 128-event class with the memo: no attribute to raise)
template <class M, bool MEMO, bool EXPLAIN = false>
hipError_t launch_class(const WTableArgs& p, uint32_t grid, uint32_t pass2, hipStream_t s) {
    constexpr size_t lds = (size_t)(TW<M>::EV + (MEMO ? TW<M>::EV : 0)) * C_LANES * 4;
    static_assert(lds <= 64u * 1024u, "dynamic LDS within the default limit");
    hipLaunchKernelGGL((wtable_search<M, MEMO, EXPLAIN>), dim3(grid), dim3(C_LANES), lds, s, p, pass2);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_table(const WTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                        hipStream_t s) {
    const uint32_t gb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((p.s.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(wtable_bin, dim3(gb), dim3(C_LANES), 0, s, p);
    hipError_t e = hipGetLastError();
    for (uint32_t pass2 = 0; pass2 < (p.budget ? 2u : 1u) && e == hipSuccess; ++pass2) {
        const uint32_t* g = pass2 ? grid2 : grid1;
        if (pass2 && p.memo) {
            if (e == hipSuccess && (classes & 1u)) e = launch_class<uint32_t, true>(p, g[0], pass2, s);
            if (e == hipSuccess && (classes & 2u)) e = launch_class<uint64_t, true>(p, g[1], pass2, s);
            if (e == hipSuccess && (classes & 4u)) e = launch_class<M128, true>(p, g[2], pass2, s);
            continue;
        }
        if (e == hipSuccess && (classes & 1u)) e = launch_class<uint32_t, false>(p, g[0], pass2, s);
        if (e == hipSuccess && (classes & 2u)) e = launch_class<uint64_t, false>(p, g[1], pass2, s);
        if (e == hipSuccess && (classes & 4u)) e = launch_class<M128, false>(p, g[2], pass2, s);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wtable_finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

// The explain call's launches (include/qsmd.h qsmd_explain_batch): launch_table
// with the EXPLAIN instantiations, always the plain search (p.memo null); the
// caller has run launch_explain_prepare on the stream.
hipError_t launch_table_explain(const WTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                                hipStream_t s) {
    const uint32_t gb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((p.s.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(wtable_bin, dim3(gb), dim3(C_LANES), 0, s, p);
    hipError_t e = hipGetLastError();
    for (uint32_t pass2 = 0; pass2 < (p.budget ? 2u : 1u) && e == hipSuccess; ++pass2) {
        const uint32_t* g = pass2 ? grid2 : grid1;
        if (e == hipSuccess && (classes & 1u)) e = launch_class<uint32_t, false, true>(p, g[0], pass2, s);
        if (e == hipSuccess && (classes & 2u)) e = launch_class<uint64_t, false, true>(p, g[1], pass2, s);
        if (e == hipSuccess && (classes & 4u)) e = launch_class<M128, false, true>(p, g[2], pass2, s);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wtable_finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

}  // namespace qsmd
