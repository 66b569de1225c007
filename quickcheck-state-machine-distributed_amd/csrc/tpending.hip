// tpending.hip -- qsmd_check_pending_batch: the search of table.hip for
// QSMD_MODEL_TABLE with one change to the reference's rule: an invocation
// whose pid has no remaining response (a crashed client, a timeout) may take
// effect with any response the model allows.
//
// Where findResponse gives [] the candidate (s, i) has one child per response
// symbol r, ascending, with bit r of post[s][i] set and of post_err[s][i]
// clear -- an *assumed* response.  Each is a counted node whose postcondition
// is not evaluated again; its state is on_resp[on_inv[s][i]][r]; its remaining
// set loses the pid's first remaining invocation (filter1, quirk Q1) and no
// response.  A history with no response event at all whose root has no child
// is LINEARISABLE with 0 nodes (every operation dropped).
//
// What differs from table.hip's TableDFS:
//   * a stack level is one 32-bit word, [level][lane] (bank lane % 32 whatever
//     the level: conflict-free): chosen event 8 | state before the step 8 |
//     assumed symbol 5 (bits 16..20) | assumed flag (bit 21);
//   * the stack has one level per event of the class (a history of
//     invocations only descends once per invocation), so one workgroup holds
//     events [EV / 2][64] words | stack [EV][64] words | the tables:
//     48 KB + 80 KB at the 128-event class and the largest table;
//   * the backtrack out of an assumed level restores only the pid's highest
//     removed invocation (the highest removed response of the pid belongs to
//     an earlier, completed operation) and goes on with the next allowed
//     symbol above the one popped, the mask read again at the restored state;
//   * finish(): LINEARISABLE also at depth 0 with no child found and no
//     response in the history;
//   * the witness and the assumed bytes are written from the stack at the end.
// The binning kernel, the class and heavy lists, the two passes, the totals
// and the probe are table.hip's (launch_table_bin, launch_table_finish); the
// explain record has no instantiation here.
//
// With the knob "pending_memo" pass 2 runs pending_search_memo: the exact-count
// state memo of table.hip's pass 2 (TableMemo, table_lane.h)
// under PendingDFS::step.  Below a node the search is a function of (rem,
// state) alone -- observed or assumed is read from rem, the allowed symbols
// from the state -- so a subtree left by a backtrack is recorded with the
// nodes it counted and a descent of either kind into a recorded (rem, state)
// counts them and backtracks at once.  The root rule of finish() concerns the
// root only, which is never recorded.  The column of node counts at entry has
// one 64-bit count per stack level, [EV][64] u64; a class whose columns and
// tables pass the device's LDS limit runs the plain kernel in pass 2 (the
// memo is exact: the same results).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "lane.h"
#include "mask.h"
#include "table_lane.h"

namespace qsmd {

namespace {

using namespace tlane;

constexpr uint32_t kAssumed = 1u << 21;     // the level's response was assumed (symbol: bits 16..20)

struct PendLds {
    const uint32_t* post;
    const uint32_t* post_err;     // null: none
    const uint8_t* on_inv;
    const uint8_t* on_resp;
    uint32_t symbols;             // the bits below n_resp
};

template <class M>
struct PendingDFS {
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
    // a leaf => True; the root without a child => False, but True when the
    // history holds no response (nothing was observed: every operation dropped)
    __device__ __forceinline__ int finish(int status) const {
        if (status != kTerm) return status;
        const bool lin = !found && (depth > 0 || !MO::any(RESP));
        return lin ? QSMD_STATUS_LINEARISABLE : QSMD_STATUS_NONLINEARISABLE;
    }

    // the response symbols the model allows at table entry idx
    static __device__ __forceinline__ uint32_t allowed(const PendLds& L, uint32_t idx) {
        return L.post[idx] & ~(L.post_err ? L.post_err[idx] : 0u) & L.symbols;
    }

    // One iteration: an optional backtrack, then one child.  Returns as
    // TableDFS::step.  stk: this lane's column, level d at stk[d * C_LANES].
    // MEMO (pass 2 with "pending_memo"): TableDFS::step<MEMO>'s rule -- the
    // node left by a backtrack is recorded with the nodes counted below it
    // (not when it was itself a hit), a descent of either kind probes the
    // child's (rem, state).
    template <bool MEMO>
    __device__ __forceinline__ int step(const TableDev& t, const PendLds& L, const uint16_t* ev, uint32_t* stk,
                                        int lane, uint64_t limit, TableMemo<M>& mm) {
        const bool empty = !MO::any(cand);
        if (empty && (found == 0u || depth == 0u)) return kTerm;
        uint32_t am = 0u, j = 0u;       // the assumed symbols still to try for candidate j
        if (empty) {
            --depth;
            if constexpr (MEMO) {
                // (rem, state) are still the node's being left
                if (!mm.skip) mm.record(rem, state, nodes - mm.entry[depth * C_LANES]);
                mm.skip = false;
            }
            const uint32_t st = stk[depth * C_LANES];
            j = st & 0xFFu;
            state = (st >> 8) & 0xFFu;
            const M gone = ~rem & same_pid(j);
            rem = rem | t_topbit<M>(gone & INV);
            if (st & kAssumed) {
                // the symbols above the one popped (2u << 31 == 0: none)
                const uint32_t r = (st >> 16) & 31u;
                am = allowed(L, state * t.n_inv + (ev[col16(j, lane)] >> 8)) & ~((2u << r) - 1u);
            } else {
                rem = rem | t_topbit<M>(gone & RESP);
            }
            cand = t_cands(rem, INV, RESP) & ~MO::below((int)j + 1);
            found = 1u;
            if (am == 0u && !MO::any(cand)) return -1;
        }
        if (am == 0u) {
            j = (uint32_t)MO::ctz(cand);
            cand = MO::clear_lowest(cand);
        }
        const M pmj = same_pid(j);
        const M rr = rem & pmj & RESP;
        const bool observed = am == 0u && MO::any(rr);
        // both event codes and both table words before the branch: the loads
        // of either kind of child are in flight together, as in table.hip's step
        const uint32_t r = observed ? (uint32_t)MO::ctz(rr) : j;
        const uint32_t i = ev[col16(j, lane)] >> 8;
        uint32_t rc = ev[col16(r, lane)] >> 8;
        const uint32_t idx = state * t.n_inv + i;
        const uint32_t pw = L.post[idx], ew = L.post_err ? L.post_err[idx] : 0u;
        uint32_t word;
        if (observed) {
            // an observed response: table.hip's step
            if (nodes >= limit) return QSMD_STATUS_BUDGET;
            ++nodes;
            found = 1u;
            if ((ew >> rc) & 1u) return QSMD_STATUS_MODEL_ERROR;
            if (!((pw >> rc) & 1u)) return -1;
            word = j | (state << 8);
            rem = rem & ~MO::bit((int)r);
        } else {
            // findResponse => []: one child per allowed symbol, none tested
            if (am == 0u) am = pw & ~ew & L.symbols;
            if (am == 0u) return -1;                 // no symbol: no child, no node
            if (nodes >= limit) return QSMD_STATUS_BUDGET;
            rc = (uint32_t)__builtin_ctz(am);
            ++nodes;
            word = j | (state << 8) | (rc << 16) | kAssumed;
        }
        stk[depth * C_LANES] = word;
        ++depth;
        state = L.on_resp[(uint32_t)L.on_inv[idx] * t.n_resp + rc];
        rem = rem & ~MO::lowest(rem & pmj & INV);    // the pid's first remaining invocation (quirk Q1)
        cand = t_cands(rem, INV, RESP);
        found = 0u;
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
                nodes = sum;                         // the subtree's nodes, counted; it failed
                cand = t_zero<M>();
                found = 1u;
                mm.skip = true;
            }
        }
        return -1;
    }
};

// table_search (table.hip) over PendingDFS; assumed: the call's assumed bytes
// (the witness layout) or null.  MEMO: pass 2 with the state memo (a.memo: one
// table of a.memo_entries entries per lane slot of the grid).
template <class M, bool MEMO>
__device__ __forceinline__ void pending_body(TableArgs a, uint32_t pass2, uint8_t* assumed) {
    constexpr int EV = TW<M>::EV, K = TW<M>::CLASS;
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const uint32_t* list = pass2 ? a.heavy_list[K] : a.class_list[K];
    const uint32_t total = a.cnt[(pass2 ? TC_HEAVY : TC_CLASS) + K];
    if ((uint64_t)blockIdx.x * C_LANES >= total) return;

    // LDS: events [EV / 2][64] words, stack [EV][64] words, (MEMO: the node
    // counts at entry, [EV][64] u64,) the tables
    uint16_t* ev = reinterpret_cast<uint16_t*>(lds);
    uint32_t* stk = lds + (EV / 2) * C_LANES + lane;
    uint32_t* tab = lds + (EV / 2 + EV + (MEMO ? 2 * EV : 0)) * C_LANES;
    TableMemo<M> mm;
    if constexpr (MEMO) {
        mm.entry = reinterpret_cast<uint64_t*>(lds + (EV / 2 + EV) * C_LANES) + lane;
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
    PendLds L;
    L.post = tab;
    L.post_err = a.t.has_err ? tab + table_off_err(a.t) : nullptr;
    L.on_inv = reinterpret_cast<const uint8_t*>(tab + table_off_inv(a.t));
    L.on_resp = reinterpret_cast<const uint8_t*>(tab + table_off_resp(a.t));
    L.symbols = a.t.n_resp >= 32u ? ~0u : (1u << a.t.n_resp) - 1u;

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
        PendingDFS<M> dfs;
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
        // the time limit checked every 1024 iterations, as table_search
        while (__ballot(status == -1) != 0ull) {
            for (uint32_t k = 0; k < 1024u; ++k) {
                if (status == -1) status = dfs.template step<MEMO>(a.t, L, ev, stk, lane, limit, mm);
                if (__ballot(status == -1) == 0ull) break;
            }
            if (status == -1 && a.s.time_limit && __builtin_amdgcn_s_memrealtime() - t0 > a.s.time_limit) {
                atomicOr(a.s.timed_out, 1u);
                status = QSMD_STATUS_BUDGET;
            }
        }
        if (status >= 0) status = dfs.finish(status);
        const bool heavy = tiered && status == QSMD_STATUS_BUDGET && dfs.nodes >= limit;
        wave_append(heavy, h, a.heavy_list[K], a.cnt + TC_HEAVY + K, lane);
        const bool out = active && !heavy;
        if (out) {
            a.s.status[h] = (uint8_t)status;
            if (a.s.nodes) a.s.nodes[h] = dfs.nodes;
            if (a.s.witness && status == QSMD_STATUS_LINEARISABLE) {
                // (depth <= the history's invocations <= n_ev: inside the slot)
                uint8_t* w = a.s.witness + H.ev_off;
                uint8_t* as = assumed ? assumed + H.ev_off : nullptr;
                for (uint32_t d = 0; d < dfs.depth; ++d) {
                    const uint32_t st = stk[d * C_LANES];
                    w[d] = (uint8_t)(st & 0xFFu);
                    if (as) as[d] = (st & kAssumed) ? (uint8_t)((st >> 16) & 31u) : (uint8_t)QSMD_ASSUMED_NONE;
                }
                if (dfs.depth < H.n_ev) {
                    w[dfs.depth] = QSMD_WITNESS_END;
                    if (as) as[dfs.depth] = QSMD_ASSUMED_NONE;
                }
            }
        }
        cnt.add(out, status, dfs.nodes);
        if constexpr (MEMO) {
            // the group's hits: one atomic per wavefront
            const uint64_t hits = wave_sum64(mm.hits);
            mm.hits = 0u;
            if (lane == 0 && hits)
                __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a.cnt + TC_PHITS), (unsigned long long)hits,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    cnt.flush(a.s.buckets, lane);
}

template <class M>
__global__ __launch_bounds__(C_LANES) void pending_search(TableArgs a, uint32_t pass2, uint8_t* assumed) {
    pending_body<M, false>(a, pass2, assumed);
}

// pass 2 with the state memo ("pending_memo")
template <class M>
__global__ __launch_bounds__(C_LANES) void pending_search_memo(TableArgs a, uint8_t* assumed) {
    pending_body<M, true>(a, 1u, assumed);
}

// The memo call's hits for the host (table_finish's probe holds the check
// call's, 0 here: the two knobs' counters are apart).
__global__ void pending_hits_probe(TableArgs a) {
    if (threadIdx.x == 0 && a.probe_host) {
        a.probe_host[kProbePendHits] = a.cnt[TC_PHITS];
        a.probe_host[kProbePendHits + 1] = a.cnt[TC_PHITS + 1];
        __threadfence_system();
    }
}

template <class M>
hipError_t launch_pending_class(const TableArgs& p, uint32_t grid, uint32_t pass2, uint8_t* assumed, hipStream_t s) {
    const size_t lds = table_lds_bytes(p.t, TW<M>::CLASS, false, true);
    if (lds > 64u * 1024u) {
        static std::atomic<int> set[kAttrDevices];
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&pending_search<M>), set, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((pending_search<M>), dim3(grid), dim3(C_LANES), lds, s, p, pass2, assumed);
    return hipGetLastError();
}

// Pass 2 of one class with the memo; a class whose memo kernel does not fit
// lds_limit runs the plain kernel.
template <class M>
hipError_t launch_pending_memo_class(const TableArgs& p, uint32_t grid, uint8_t* assumed, size_t lds_limit,
                                     hipStream_t s) {
    const size_t lds = table_lds_bytes(p.t, TW<M>::CLASS, true, true);
    if (lds > lds_limit) return launch_pending_class<M>(p, grid, 1u, assumed, s);
    if (lds > 64u * 1024u) {
        static std::atomic<int> set[kAttrDevices];
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&pending_search_memo<M>), set, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((pending_search_memo<M>), dim3(grid), dim3(C_LANES), lds, s, p, assumed);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_table_pending(const TableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3],
                                uint32_t classes, uint8_t* assumed, size_t lds_limit, hipStream_t s) {
    hipError_t e = launch_table_bin(p, s);
    for (uint32_t pass2 = 0; pass2 < (p.budget ? 2u : 1u) && e == hipSuccess; ++pass2) {
        const uint32_t* g = pass2 ? grid2 : grid1;
        if (pass2 && p.memo) {
            if (e == hipSuccess && (classes & 1u)) e = launch_pending_memo_class<uint32_t>(p, g[0], assumed, lds_limit, s);
            if (e == hipSuccess && (classes & 2u)) e = launch_pending_memo_class<uint64_t>(p, g[1], assumed, lds_limit, s);
            if (e == hipSuccess && (classes & 4u)) e = launch_pending_memo_class<M128>(p, g[2], assumed, lds_limit, s);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(pending_hits_probe, dim3(1), dim3(C_LANES), 0, s, p);
                e = hipGetLastError();
            }
            continue;
        }
        if (e == hipSuccess && (classes & 1u)) e = launch_pending_class<uint32_t>(p, g[0], pass2, assumed, s);
        if (e == hipSuccess && (classes & 2u)) e = launch_pending_class<uint64_t>(p, g[1], pass2, assumed, s);
        if (e == hipSuccess && (classes & 4u)) e = launch_pending_class<M128>(p, g[2], pass2, assumed, s);
    }
    if (e != hipSuccess) return e;
    return launch_table_finish(p, s);
}

}  // namespace qsmd
