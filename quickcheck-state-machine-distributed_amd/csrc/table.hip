// table.hip -- QSMD_MODEL_TABLE: the reference search for a finite-state
// model given as tables at run time (include/qsmd.h qsmd_table_model).
//
// The reference's `linearisable` takes any transition / postcondition
// closures (src/Linearisability.hs:52-58); a C ABI cannot.  A model with at
// most 256 states and 32 invocation / response symbols is four tables, and a
// step from state s with invocation i and response r is
//     post  = bit r of post[s][i]            (postcondition m inv resp)
//     raise = bit r of post_err[s][i]        (the postcondition raises)
//     next  = on_resp[on_inv[s][i]][r]       (transition twice, :63-65)
//
// One lane per history runs the reference DFS over the Lemma L1 event bitset
// (SURVEY.md §8a), as the compact stages do (lane.h LaneDFS), but for any
// history the encoding holds: up to 128 events, 128 pids, shared pids.  The
// pids are bit-sliced into seven mask planes (lane.h slices three).  Nothing
// of the hot loop is in global memory:
//   * the tables are copied to LDS by every workgroup (dynamic size: the
//     table actually set; 80 KB at 256 x 32 x 32 with post_err);
//   * a history's events are 16 bits each (pid 7 | kind 1 | code 8: the low
//     half of the event's first word), the DFS stack 16 bits per level
//     (chosen event 8 | state before the step 8).  Both are stored two to a
//     32-bit word, [x / 2][lane][x & 1]: the word a lane touches is in bank
//     lane % 32 whatever x is, so the per-lane indexed 16-bit reads and
//     writes of a divergent wavefront are conflict-free ([x][lane] with
//     16-bit elements would put lanes 2k and 2k + 1 on one bank with
//     different rows: a 2-way conflict);
//   * undo restores the remaining set by Lemma L1 (the last removed events
//     of the pid are the highest removed ones) and the state from the stack.
//
// Three width classes (32-, 64-, 128-event masks) so a batch of short
// histories pays neither M128 masks nor 128-event LDS: table_bin sorts the
// headers into three index lists (wave_append), one launch per class.  Each
// class runs two passes: pass 1 with a node budget ("table_budget"), a search
// over it appended to the class's heavy list; pass 2 grid-stride over that
// list (count read on the device), each history searched again from the root
// -- so the node counts stay the reference's.  With the knob "table_memo"
// pass 2 runs the MEMO instantiation: an exact-count state memo per lane slot
// (TableMemo, table_lane.h; the counts, the verdict and the witness are unchanged).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "lane.h"
#include "mask.h"
#include "table_lane.h"

namespace qsmd {

namespace {

using namespace tlane;     // the width classes, mask helpers, col16, stage_table, TableMemo

struct TabLds {
    const uint32_t* post;
    const uint32_t* post_err;     // null: none
    const uint8_t* on_inv;
    const uint8_t* on_resp;
};

// One lane's search state (registers) over its LDS columns.
template <class M>
struct TableDFS {
    using MO = MaskOps<M>;
    M INV, RESP, P[7];
    M rem, cand;
    uint32_t state, depth, found;
    uint64_t nodes;

    // the events of event j's pid (the bits beyond the history are junk:
    // every use ANDs with INV or RESP)
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

    // One iteration, as LaneDFS::step: an optional backtrack, then one
    // candidate.  -1 = go on, kTerm = the search ended (finish()), or
    // QSMD_STATUS_BUDGET (limit nodes counted; nothing moved) /
    // QSMD_STATUS_MODEL_ERROR.
    // MEMO (pass 2 with "table_memo"): a subtree left by a backtrack is
    // recorded with the nodes it counted, a descent into a recorded state
    // counts them and backtracks at once (the rule of memo.hip's memo_step).
    // EXPLAIN (the explain calls, never with MEMO): xp records the deepest
    // path into `path` (DeepPath, table_lane.h).
    template <bool MEMO, bool EXPLAIN>
    __device__ __forceinline__ int step(const TableDev& t, const TabLds& L, const uint16_t* ev, uint16_t* stk,
                                        int lane, uint64_t limit, TableMemo<M>& mm, DeepPath<uint32_t>& xp,
                                        uint8_t* path) {
        const bool empty = !MO::any(cand);
        // no children: a leaf => True (any' []), the root => False (any [])
        if (empty && (found == 0u || depth == 0u)) return kTerm;
        if (empty) {
            // backtrack: the parent's remaining set by Lemma L1, its state
            // from the stack
            --depth;
            if constexpr (EXPLAIN) xp.fell_to(depth);
            if constexpr (MEMO) {
                // (rem, state) are still the node's being left
                if (!mm.skip) mm.record(rem, state, nodes - mm.entry[depth * C_LANES]);
                mm.skip = false;
            }
            const uint32_t st = stk[col16(depth, lane)];
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
        const uint32_t idx = state * t.n_inv + i;
        const uint32_t ok = (L.post[idx] >> rc) & 1u;
        const uint32_t err = L.post_err ? (L.post_err[idx] >> rc) & 1u : 0u;
        ++nodes;
        found = 1u;
        if (err) return QSMD_STATUS_MODEL_ERROR;
        if (ok) {
            stk[col16(depth, lane)] = (uint16_t)(j | (state << 8));
            ++depth;
            state = L.on_resp[(uint32_t)L.on_inv[idx] * t.n_resp + rc];
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
__global__ __launch_bounds__(C_LANES) void table_bin(TableArgs a) {
    const int lane = threadIdx.x;
    WaveCounters cnt;
    for (uint64_t base = (uint64_t)blockIdx.x * C_LANES; base < a.s.n_hist; base += (uint64_t)gridDim.x * C_LANES) {
        const uint64_t h = base + lane;
        const bool active = h < a.s.n_hist;
        qsmd_hdr H{0, 0, 0, 0, 0, 0};
        if (active) H = a.s.hdr[h];
        const bool enc_ok = H.model_id == QSMD_MODEL_TABLE && H.n_ev <= QSMD_MAX_EVENTS &&
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
__global__ __launch_bounds__(C_LANES) void table_search(TableArgs a, uint32_t pass2) {
    constexpr int EV = TW<M>::EV, K = TW<M>::CLASS;
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const uint32_t* list = pass2 ? a.heavy_list[K] : a.class_list[K];
    const uint32_t total = a.cnt[(pass2 ? TC_HEAVY : TC_CLASS) + K];
    if ((uint64_t)blockIdx.x * C_LANES >= total) return;

    // LDS: events [EV / 2][64] words, stack [EV / 4][64] words, (MEMO: the
    // node counts at entry, [EV / 2][64] u64,) the tables
    uint16_t* ev = reinterpret_cast<uint16_t*>(lds);
    uint16_t* stk = reinterpret_cast<uint16_t*>(lds + (EV / 2) * C_LANES);
    uint32_t* tab = lds + (EV / 2 + EV / 4 + (MEMO ? EV : 0)) * C_LANES;
    TableMemo<M> mm;
    if constexpr (MEMO) {
        mm.entry = reinterpret_cast<uint64_t*>(lds + (EV / 2 + EV / 4) * C_LANES) + lane;
        mm.tab = a.memo + ((uint64_t)blockIdx.x * C_LANES + (uint64_t)lane) * (uint64_t)a.memo_entries * 2ull;
        mm.mask = a.memo_entries - 1u;
        mm.tag = a.memo_epoch << 8;
        mm.hits = 0u;
    }
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.t.blob);
        uint4* dst = reinterpret_cast<uint4*>(tab);
        for (uint32_t k = lane; k < a.t.blob_words / 4u; k += C_LANES) dst[k] = src[k];
    }
    __syncthreads();
    TabLds L;
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
        TableDFS<M> dfs;
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
__global__ __launch_bounds__(C_LANES) void table_finish(TableArgs a) {
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

// The explain call's first launch, for the three table models (a.model_id):
// every history's qsmd_explain record as the binning kernel's verdicts need it
// -- zero, with the initial state for an empty history (depth 0); the search
// kernels overwrite the records of the histories they decide -- and, for an
// ENCODE_ERROR found in the header, the terminator in the first byte of a slot
// that has one inside the events array.
__global__ __launch_bounds__(C_LANES) void explain_prepare(SearchArgs a, uint64_t state0, uint8_t* path,
                                                           uint4* explain) {
    for (uint64_t h = (uint64_t)blockIdx.x * C_LANES + threadIdx.x; h < a.n_hist; h += (uint64_t)gridDim.x * C_LANES) {
        const qsmd_hdr H = a.hdr[h];
        const bool enc_ok = H.model_id == a.model_id && H.n_ev <= QSMD_MAX_EVENTS &&
                            (uint64_t)H.ev_off + H.n_ev <= a.n_events;
        const uint64_t st = enc_ok ? state0 : 0ull;     // (enc_ok and searched: overwritten)
        explain[h] = make_uint4(0u, 0u, (uint32_t)st, (uint32_t)(st >> 32));
        if (!enc_ok && H.n_ev > 0u && (uint64_t)H.ev_off < a.n_events) path[H.ev_off] = QSMD_WITNESS_END;
    }
}

template <class M, bool MEMO, bool EXPLAIN = false>
hipError_t launch_class(const TableArgs& p, uint32_t grid, uint32_t pass2, hipStream_t s) {
    const size_t lds = table_lds_bytes(p.t, TW<M>::CLASS, MEMO);
    if (lds > 64u * 1024u) {
        static std::atomic<int> set[kAttrDevices];
        const hipError_t e =
            ensure_dyn_lds(reinterpret_cast<const void*>(&table_search<M, MEMO, EXPLAIN>), set, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((table_search<M, MEMO, EXPLAIN>), dim3(grid), dim3(C_LANES), lds, s, p, pass2);
    return hipGetLastError();
}

}  // namespace

size_t table_lds_bytes(const TableDev& t, int k, bool memo, bool pending) {
    const size_t ev = k == 0 ? 32 : (k == 1 ? 64 : 128);
    // (pending: csrc/tpending.hip's stack, one 32-bit level per event)
    // (and with the memo its column of counts, one u64 per event)
    const size_t stack = pending ? ev : ev / 4;
    const size_t entry = memo ? (pending ? 2 * ev : ev) : 0;
    return ((ev / 2 + stack + entry) * C_LANES + (size_t)t.blob_words) * 4;
}

// The first and the last launch of a table call on their own (csrc/tpending.hip).
hipError_t launch_table_bin(const TableArgs& p, hipStream_t s) {
    const uint32_t gb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((p.s.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(table_bin, dim3(gb), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_table_finish(const TableArgs& p, hipStream_t s) {
    hipLaunchKernelGGL(table_finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_explain_prepare(const SearchArgs& a, uint64_t state0, uint8_t* path, uint4* explain,
                                  hipStream_t s) {
    const uint32_t gb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((a.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(explain_prepare, dim3(gb), dim3(C_LANES), 0, s, a, state0, path, explain);
    return hipGetLastError();
}

hipError_t launch_table(const TableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                        hipStream_t s) {
    static_assert(sizeof(qsmd_totals) == T_N * 8, "qsmd_totals is T_N x u64 in T_* order");
    const uint32_t gb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((p.s.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(table_bin, dim3(gb), dim3(C_LANES), 0, s, p);
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
    hipLaunchKernelGGL(table_finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

// The explain call's launches (include/qsmd.h qsmd_explain_batch): launch_table
// with the EXPLAIN instantiations, always the plain search (p.memo null); the
// caller has run launch_explain_prepare on the stream.
hipError_t launch_table_explain(const TableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                                hipStream_t s) {
    const uint32_t gb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((p.s.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(table_bin, dim3(gb), dim3(C_LANES), 0, s, p);
    hipError_t e = hipGetLastError();
    for (uint32_t pass2 = 0; pass2 < (p.budget ? 2u : 1u) && e == hipSuccess; ++pass2) {
        const uint32_t* g = pass2 ? grid2 : grid1;
        if (e == hipSuccess && (classes & 1u)) e = launch_class<uint32_t, false, true>(p, g[0], pass2, s);
        if (e == hipSuccess && (classes & 2u)) e = launch_class<uint64_t, false, true>(p, g[1], pass2, s);
        if (e == hipSuccess && (classes & 4u)) e = launch_class<M128, false, true>(p, g[2], pass2, s);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(table_finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

}  // namespace qsmd
