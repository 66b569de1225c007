// ktable.hip -- QSMD_MODEL_KTABLE: the reference search on the product of
// n_keys (1..8) copies of one narrow table model (include/qsmd.h
// qsmd_ktable_set).  The model value is a vector s[0..n_keys) of component
// states; an invocation carries its component symbol in `code` and its key in
// `a`, and a step from s with invocation (k, i) and response r is
//     post  = bit r of post[s[k]][i]
//     raise = bit r of post_err[s[k]][i]      (wins over post)
//     s[k] := on_resp[on_inv[s[k]][i]][r]     (every other key unchanged)
// -- src/Linearisability.hs:63-65 on the product model, whose flat table
// would have n_states^n_keys states.
//
// Everything else is table.hip's search (TableDFS): one lane per history over
// the Lemma L1 event bitset and seven pid planes, three width classes, pass 1
// with "table_budget", pass 2 grid-stride over the heavy list from the root,
// a finish kernel, the time limit every 1024 iterations.  What differs is the
// lane's step:
//   * the state is the 8 component bytes in one 64-bit register pair; s[k]
//     is read and written with 64-bit shifts on the lane's own k, so the
//     model is never in memory;
//   * a stack entry stays 16 bits: chosen event 8 | the state s[k] had before
//     the step 8, k being that event's key.  Undo reads the key from the
//     event and restores that one byte;
//   * an event stays 16 bits in LDS: pid 7 | kind 1 | code 5 | key 3 (the
//     component has at most 32 symbols; a response's key bits are 0), in
//     col16's paired words, so the per-lane indexed reads of a divergent
//     wavefront stay conflict-free and the LDS bytes are model 3's (the
//     element and its staging: ktable_lane.h, shared with kpending.hip).
//
// Pass 2's exact-count state memo (knob "ktable_memo") is
// table.hip's rule (TableDFS::step<MEMO>) on S = (rem, the full 64-bit
// state): the backtrack branch records (S of the node being left, the nodes
// counted since its entry) before rem and state are restored; after a
// descent S of the child is probed, and a hit counts the recorded nodes and
// backtracks at once (or ends as BUDGET when the limit falls inside them).  A
// raising step, a time-limit stop and a budget stop record nothing.  One
// direct-mapped table of "ktable_memo" entries per lane slot of pass 2's
// grid, in HBM.  One entry size for every width class, 48 B = 3 x uint4:
//     [0]  count lo | count hi | epoch (the call's, a full word) | history index
//     [1]  state lo | state hi | rem word 0 | rem word 1
//     [2]  rem word 2 | rem word 3 | 0 | 0        (128-event class only)
// The 32- and 64-event classes read and write [0] and [1] only (their rem
// word 1 / words 2-3 do not exist).  The epoch and the history index stand in
// the same place for every class, so an entry left by another class or
// another call never matches: a hit compares epoch, history, both state
// words and every rem word, never the hash alone.  The slot is a
// multiplicative hash of the rem words and both state words; table.hip's
// 64-bit map of written slots (mod 64) gates the HBM probe.  "table_memo"
// has no effect here: with "ktable_memo" 0 pass 2 is the plain one.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "ktable_lane.h"
#include "lane.h"
#include "mask.h"
#include "table_lane.h"

namespace qsmd {

namespace {

using namespace tlane;
using namespace klane;

struct KTabLds {
    const uint32_t* post;
    const uint32_t* post_err;     // null: none
    const uint8_t* on_inv;
    const uint8_t* on_resp;
};

// One lane's view of pass 2's state memo (the header comment): its table in
// HBM, its LDS column of node counts at entry per level, the map of written
// slots.  tlane::TableMemo with the 64-bit state and the 3 x uint4 entry.
template <class M>
struct KTableMemo {
    static constexpr int NW = TW<M>::NW;
    uint4* tab;             // the lane's table
    uint64_t* entry;        // LDS: [level][lane], this lane's column
    uint32_t mask;          // entries - 1
    uint32_t epoch;         // the call's tag (never 0: cleared tables match nothing)
    uint32_t h;
    uint32_t hits;
    uint64_t wr;
    bool skip;              // the node being left was a hit: recorded already

    __device__ __forceinline__ uint32_t slot_of(const uint32_t* w, uint64_t state) const {
        constexpr uint32_t K[4] = {0x9E3779B1u, 0x85EBCA77u, 0xC2B2AE3Du, 0x27D4EB2Fu};
        uint32_t x = (uint32_t)state * 0x165667B1u ^ (uint32_t)(state >> 32) * 0xD6E8FEB9u;
#pragma unroll
        for (int k = 0; k < NW; ++k) x ^= w[k] * K[k];
        x ^= x >> 16;
        x *= 0x85EBCA6Bu;
        x ^= x >> 13;
        return x & mask;
    }
    __device__ __forceinline__ void begin(uint32_t hist) {
        h = hist;
        wr = 0ull;
        skip = false;
    }
    __device__ __forceinline__ void record(const M& rem, uint64_t state, uint64_t count) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        to_words(rem, w);
        const uint32_t slot = slot_of(w, state);
        uint4* e = tab + 3u * slot;
        e[0] = make_uint4((uint32_t)count, (uint32_t)(count >> 32), epoch, h);
        e[1] = make_uint4((uint32_t)state, (uint32_t)(state >> 32), w[0], w[1]);
        if constexpr (NW > 2) e[2] = make_uint4(w[2], w[3], 0u, 0u);
        wr |= 1ull << (slot & 63u);
    }
    // the whole key is compared: epoch, history, both state words, every rem word
    __device__ __forceinline__ bool probe(const M& rem, uint64_t state, uint64_t& count) const {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        to_words(rem, w);
        const uint32_t slot = slot_of(w, state);
        if (!((wr >> (slot & 63u)) & 1ull)) return false;
        const uint4* e = tab + 3u * slot;
        const uint4 a = e[0], b = e[1];
        count = a.x | ((uint64_t)a.y << 32);
        bool same = a.z == epoch && a.w == h && b.x == (uint32_t)state && b.y == (uint32_t)(state >> 32) &&
                    b.z == w[0] && b.w == w[1];
        if constexpr (NW > 2) {
            const uint4 c = e[2];
            same = same && c.x == w[2] && c.y == w[3];
        }
        return same;
    }
};

// One lane's search state (registers) over its LDS columns: table.hip's
// TableDFS with the keyed step.
template <class M>
struct KTableDFS {
    using MO = MaskOps<M>;
    M INV, RESP, P[7];
    M rem, cand;
    uint64_t state;               // key k's component state in bits 8k .. 8k + 7
    uint32_t depth, found;
    uint64_t nodes;

    __device__ __forceinline__ M same_pid(uint32_t j) const {
        M acc = t_ones<M>();
#pragma unroll
        for (int b = 0; b < 7; ++b) acc = acc & (t_test(P[b], j) ? P[b] : ~P[b]);
        return acc;
    }

    __device__ __forceinline__ void init(uint64_t state0) {
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

    // s[k] from `was` to `now` (shift = 8k): one 64-bit shift and an xor
    __device__ __forceinline__ void put(uint32_t shift, uint32_t was, uint32_t now) {
        state ^= (uint64_t)(was ^ now) << shift;
    }

    // One iteration, as TableDFS::step: an optional backtrack, then one
    // candidate.  -1 = go on, kTerm = the search ended (finish()), or
    // QSMD_STATUS_BUDGET (limit nodes counted; nothing moved) /
    // QSMD_STATUS_MODEL_ERROR.
    // MEMO (pass 2 with "ktable_memo"): a subtree left by a backtrack is
    // recorded with the nodes it counted, a descent into a recorded (rem,
    // state) counts them and backtracks at once.
    // EXPLAIN (the explain calls, never with MEMO): xp records the deepest
    // path into `path` (DeepPath, table_lane.h).
    template <bool MEMO, bool EXPLAIN>
    __device__ __forceinline__ int step(const TableDev& t, const KTabLds& L, const uint16_t* ev, uint16_t* stk,
                                        int lane, uint64_t limit, KTableMemo<M>& mm, DeepPath<uint64_t>& xp,
                                        uint8_t* path) {
        const bool empty = !MO::any(cand);
        if (empty && (found == 0u || depth == 0u)) return kTerm;
        if (empty) {
            // backtrack: the parent's remaining set by Lemma L1, the one
            // component the step changed from the stack
            --depth;
            if constexpr (EXPLAIN) xp.fell_to(depth);
            if constexpr (MEMO) {
                // (rem, state) are still the node's being left
                if (!mm.skip) mm.record(rem, state, nodes - mm.entry[depth * C_LANES]);
                mm.skip = false;
            }
            const uint32_t st = stk[col16(depth, lane)];
            const uint32_t j = st & 0xFFu;
            const uint32_t shift = kev_key(ev[col16(j, lane)]) * 8u;
            put(shift, (uint32_t)(state >> shift) & 0xFFu, st >> 8);
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
        const uint32_t ej = ev[col16(j, lane)];
        const uint32_t i = kev_code(ej), rc = kev_code(ev[col16(r, lane)]);
        const uint32_t shift = kev_key(ej) * 8u;
        const uint32_t sk = (uint32_t)(state >> shift) & 0xFFu;
        const uint32_t idx = sk * t.n_inv + i;
        const uint32_t ok = (L.post[idx] >> rc) & 1u;
        const uint32_t err = L.post_err ? (L.post_err[idx] >> rc) & 1u : 0u;
        ++nodes;
        found = 1u;
        if (err) return QSMD_STATUS_MODEL_ERROR;
        if (ok) {
            stk[col16(depth, lane)] = (uint16_t)(j | (sk << 8));
            ++depth;
            put(shift, sk, L.on_resp[(uint32_t)L.on_inv[idx] * t.n_resp + rc]);
            // the pid's first remaining invocation (quirk Q1: not always j) and response
            rem = rem & ~(MO::lowest(rem & pmj & INV) | MO::bit((int)r));
            cand = t_cands(rem, INV, RESP);
            found = 0u;
            if constexpr (EXPLAIN)
                xp.descended(path, depth, state, [&](uint32_t d) { return stk[col16(d, lane)] & 0xFFu; });
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

// Sort the headers into the three class lists; the histories decided from
// the header alone get their result here.
__global__ __launch_bounds__(C_LANES) void ktable_bin(KTableArgs a) {
    const int lane = threadIdx.x;
    WaveCounters cnt;
    for (uint64_t base = (uint64_t)blockIdx.x * C_LANES; base < a.s.n_hist; base += (uint64_t)gridDim.x * C_LANES) {
        const uint64_t h = base + lane;
        const bool active = h < a.s.n_hist;
        qsmd_hdr H{0, 0, 0, 0, 0, 0};
        if (active) H = a.s.hdr[h];
        const bool enc_ok = H.model_id == QSMD_MODEL_KTABLE && H.n_ev <= QSMD_MAX_EVENTS &&
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

// PASS2 false: the class list with the pass-1 budget; true: the class's
// heavy list, every search to its end.
// MEMO: pass 2 with the state memo (a.memo: one table of a.memo_entries
// entries per lane slot of the grid).
template <class M, bool MEMO, bool EXPLAIN>
__global__ __launch_bounds__(C_LANES) void ktable_search(KTableArgs a, uint32_t pass2) {
    constexpr int EV = TW<M>::EV, K = TW<M>::CLASS;
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const uint32_t* list = pass2 ? a.heavy_list[K] : a.class_list[K];
    const uint32_t total = a.cnt[(pass2 ? TC_HEAVY : TC_CLASS) + K];
    if ((uint64_t)blockIdx.x * C_LANES >= total) return;

    // LDS: events [EV / 2][64] words, stack [EV / 4][64] words, (MEMO: the
    // node counts at entry, [EV / 2][64] u64,) the component's tables
    uint16_t* ev = reinterpret_cast<uint16_t*>(lds);
    uint16_t* stk = reinterpret_cast<uint16_t*>(lds + (EV / 2) * C_LANES);
    uint32_t* tab = lds + (EV / 2 + EV / 4 + (MEMO ? EV : 0)) * C_LANES;
    KTableMemo<M> mm;
    if constexpr (MEMO) {
        mm.entry = reinterpret_cast<uint64_t*>(lds + (EV / 2 + EV / 4) * C_LANES) + lane;
        mm.tab = a.memo + ((uint64_t)blockIdx.x * C_LANES + (uint64_t)lane) * (uint64_t)a.memo_entries * 3ull;
        mm.mask = a.memo_entries - 1u;
        mm.epoch = a.memo_epoch;
        mm.hits = 0u;
    }
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.t.blob);
        uint4* dst = reinterpret_cast<uint4*>(tab);
        for (uint32_t k = lane; k < a.t.blob_words / 4u; k += C_LANES) dst[k] = src[k];
    }
    __syncthreads();
    KTabLds L;
    L.post = tab;
    L.post_err = a.t.has_err ? tab + table_off_err(a.t) : nullptr;
    L.on_inv = reinterpret_cast<const uint8_t*>(tab + table_off_inv(a.t));
    L.on_resp = reinterpret_cast<const uint8_t*>(tab + table_off_resp(a.t));

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
        KTableDFS<M> dfs;
        dfs.depth = 0;
        dfs.nodes = 0;
        dfs.found = 0;
        // -2: no history in this lane
        int status = -2;
        if (active) {
            status = stage_ktable<M>(a, H, ev, lane, dfs) ? -1 : QSMD_STATUS_ENCODE_ERROR;
            if (status == -1) dfs.init(a.state0);
        }
        if constexpr (MEMO) mm.begin(h);
        DeepPath<uint64_t> xp;
        if constexpr (EXPLAIN) xp.begin(H.ev_off, a.state0);
        // the search, the time limit checked every 1024 iterations (a
        // wavefront-uniform counter: the loop runs while any lane searches)
        while (__ballot(status == -1) != 0ull) {
            for (uint32_t k = 0; k < 1024u; ++k) {
                if (status == -1)
                    status = dfs.template step<MEMO, EXPLAIN>(a.t, L, ev, stk, lane, limit, mm, xp, a.path);
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
                for (uint32_t d = 0; d < dfs.depth; ++d) w[d] = (uint8_t)(stk[col16(d, lane)] & 0xFFu);
                if (dfs.depth < H.n_ev) w[dfs.depth] = QSMD_WITNESS_END;
            }
        }
        if constexpr (EXPLAIN) {
            const auto at = [&](uint32_t d) { return stk[col16(d, lane)] & 0xFFu; };
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

// The call's totals from the buckets, the probe for the host.
__global__ __launch_bounds__(C_LANES) void ktable_finish(KTableArgs a) {
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

template <class M, bool MEMO, bool EXPLAIN = false>
hipError_t launch_class(const KTableArgs& p, uint32_t grid, uint32_t pass2, hipStream_t s) {
    const size_t lds = table_lds_bytes(p.t, TW<M>::CLASS, MEMO);
    if (lds > 64u * 1024u) {
        static std::atomic<int> set[kAttrDevices];
        const hipError_t e =
            ensure_dyn_lds(reinterpret_cast<const void*>(&ktable_search<M, MEMO, EXPLAIN>), set, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((ktable_search<M, MEMO, EXPLAIN>), dim3(grid), dim3(C_LANES), lds, s, p, pass2);
    return hipGetLastError();
}

}  // namespace

// The first and the last launch of a keyed call on their own (csrc/kpending.hip).
hipError_t launch_ktable_bin(const KTableArgs& p, hipStream_t s) {
    const uint32_t gb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((p.s.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(ktable_bin, dim3(gb), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ktable_finish(const KTableArgs& p, hipStream_t s) {
    hipLaunchKernelGGL(ktable_finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_table(const KTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                        hipStream_t s) {
    hipError_t e = launch_ktable_bin(p, s);
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
    return launch_ktable_finish(p, s);
}

// The explain call's launches (include/qsmd.h qsmd_explain_batch): launch_table
// with the EXPLAIN instantiations, always the plain search (p.memo null); the
// caller has run launch_explain_prepare on the stream.
hipError_t launch_table_explain(const KTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                                hipStream_t s) {
    const uint32_t gb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((p.s.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(ktable_bin, dim3(gb), dim3(C_LANES), 0, s, p);
    hipError_t e = hipGetLastError();
    for (uint32_t pass2 = 0; pass2 < (p.budget ? 2u : 1u) && e == hipSuccess; ++pass2) {
        const uint32_t* g = pass2 ? grid2 : grid1;
        if (e == hipSuccess && (classes & 1u)) e = launch_class<uint32_t, false, true>(p, g[0], pass2, s);
        if (e == hipSuccess && (classes & 2u)) e = launch_class<uint64_t, false, true>(p, g[1], pass2, s);
        if (e == hipSuccess && (classes & 4u)) e = launch_class<M128, false, true>(p, g[2], pass2, s);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ktable_finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

}  // namespace qsmd
