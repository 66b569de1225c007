// kpending.hip -- qsmd_check_kpending_batch: the search of ktable.hip for
// QSMD_MODEL_KTABLE with tpending.hip's change to the reference's rule, on the
// product model: an invocation whose pid has no remaining response (a crashed
// client, a timeout) may take effect with any response the component allows
// at its key's state.
//
// Where findResponse gives [] the candidate (s, (k, i)) has one child per
// response symbol r, ascending, with bit r of post[s[k]][i] set and of
// post_err[s[k]][i] clear -- an *assumed* response.  Each is a counted node
// whose postcondition is not evaluated again; its state has
// s[k] := on_resp[on_inv[s[k]][i]][r], every other key unchanged; its
// remaining set loses the pid's first remaining invocation (filter1, quirk
// Q1) and no response.  A history with no response event at all whose root
// has no child is LINEARISABLE with 0 nodes (every operation dropped).
//
// The control flow is tpending.hip's PendingDFS, the state handling
// ktable.hip's KTableDFS:
//   * the state is the 8 component bytes in one 64-bit register pair; s[k] is
//     read and written with 64-bit shifts on the lane's own k (KTableDFS::put);
//   * an event is ktable's 16-bit LDS element, pid 7 | kind 1 | code 5 | key 3,
//     in col16's paired words (ktable_lane.h stage_ktable: a key is validated
//     < n_keys there, so every shift is <= 56);
//   * a stack level is tpending's 32-bit word, [level][lane]: chosen event 8 |
//     the state s[k] had before the step 8 | assumed symbol 5 (bits 16..20) |
//     assumed flag (bit 21), k being the chosen event's key -- read from that
//     event at undo, never from the pid's previous operation;
//   * the stack has one level per event of the class, so one workgroup holds
//     events [EV / 2][64] words | stack [EV][64] words | the component's
//     tables: 48 KB + 80 KB at the 128-event class and the largest component;
//   * the backtrack out of an assumed level restores the one byte of key k and
//     only the pid's highest removed invocation (the highest removed response
//     of the pid belongs to an earlier, completed operation, maybe on another
//     key) and goes on with the next allowed symbol above the one popped, the
//     mask read again at the restored s[k];
//   * the allowed mask is cut to the bits below n_resp, so every on_resp index
//     is in range;
//   * finish(): LINEARISABLE also at depth 0 with no child found and no
//     response in the history;
//   * the witness and the assumed bytes are written from the stack at the end.
// The binning kernel, the class and heavy lists, the two passes, the totals
// and the probe are ktable.hip's (launch_ktable_bin, launch_ktable_finish).
// No memo, no explain record and no local mode have an instantiation here.
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

constexpr uint32_t kAssumed = 1u << 21;     // the level's response was assumed (symbol: bits 16..20)

struct KPendLds {
    const uint32_t* post;
    const uint32_t* post_err;     // null: none
    const uint8_t* on_inv;
    const uint8_t* on_resp;
    uint32_t symbols;             // the bits below n_resp
};

template <class M>
struct KPendingDFS {
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
    // a leaf => True; the root without a child => False, but True when the
    // history holds no response (nothing was observed: every operation dropped)
    __device__ __forceinline__ int finish(int status) const {
        if (status != kTerm) return status;
        const bool lin = !found && (depth > 0 || !MO::any(RESP));
        return lin ? QSMD_STATUS_LINEARISABLE : QSMD_STATUS_NONLINEARISABLE;
    }

    // s[k] from `was` to `now` (shift = 8k): one 64-bit shift and an xor
    __device__ __forceinline__ void put(uint32_t shift, uint32_t was, uint32_t now) {
        state ^= (uint64_t)(was ^ now) << shift;
    }

    // the response symbols the component allows at table entry idx
    static __device__ __forceinline__ uint32_t allowed(const KPendLds& L, uint32_t idx) {
        return L.post[idx] & ~(L.post_err ? L.post_err[idx] : 0u) & L.symbols;
    }

    // One iteration: an optional backtrack, then one child.  Returns as
    // KTableDFS::step.  stk: this lane's column, level d at stk[d * C_LANES].
    __device__ __forceinline__ int step(const TableDev& t, const KPendLds& L, const uint16_t* ev, uint32_t* stk,
                                        int lane, uint64_t limit) {
        const bool empty = !MO::any(cand);
        if (empty && (found == 0u || depth == 0u)) return kTerm;
        uint32_t am = 0u, j = 0u;       // the assumed symbols still to try for candidate j
        if (empty) {
            // backtrack: the one component the step changed from the stack,
            // its key from the chosen event
            --depth;
            const uint32_t st = stk[depth * C_LANES];
            j = st & 0xFFu;
            const uint32_t ej = ev[col16(j, lane)];
            const uint32_t shift = kev_key(ej) * 8u, sk = (st >> 8) & 0xFFu;
            put(shift, (uint32_t)(state >> shift) & 0xFFu, sk);
            const M gone = ~rem & same_pid(j);
            rem = rem | t_topbit<M>(gone & INV);
            if (st & kAssumed) {
                // the symbols above the one popped (2u << 31 == 0: none)
                const uint32_t r = (st >> 16) & 31u;
                am = allowed(L, sk * t.n_inv + kev_code(ej)) & ~((2u << r) - 1u);
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
        // both events and both table words before the branch: the loads of
        // either kind of child are in flight together, as in tpending.hip's step
        const uint32_t r = observed ? (uint32_t)MO::ctz(rr) : j;
        const uint32_t ej = ev[col16(j, lane)];
        uint32_t rc = kev_code(ev[col16(r, lane)]);
        const uint32_t shift = kev_key(ej) * 8u;
        const uint32_t sk = (uint32_t)(state >> shift) & 0xFFu;
        const uint32_t idx = sk * t.n_inv + kev_code(ej);
        const uint32_t pw = L.post[idx], ew = L.post_err ? L.post_err[idx] : 0u;
        uint32_t word;
        if (observed) {
            // an observed response: ktable.hip's step
            if (nodes >= limit) return QSMD_STATUS_BUDGET;
            ++nodes;
            found = 1u;
            if ((ew >> rc) & 1u) return QSMD_STATUS_MODEL_ERROR;
            if (!((pw >> rc) & 1u)) return -1;
            word = j | (sk << 8);
            rem = rem & ~MO::bit((int)r);
        } else {
            // findResponse => []: one child per allowed symbol, none tested
            if (am == 0u) am = pw & ~ew & L.symbols;
            if (am == 0u) return -1;                 // no symbol: no child, no node
            if (nodes >= limit) return QSMD_STATUS_BUDGET;
            rc = (uint32_t)__builtin_ctz(am);
            ++nodes;
            word = j | (sk << 8) | (rc << 16) | kAssumed;
        }
        stk[depth * C_LANES] = word;
        ++depth;
        put(shift, sk, L.on_resp[(uint32_t)L.on_inv[idx] * t.n_resp + rc]);
        rem = rem & ~MO::lowest(rem & pmj & INV);    // the pid's first remaining invocation (quirk Q1)
        cand = t_cands(rem, INV, RESP);
        found = 0u;
        return -1;
    }
};

// ktable_search (ktable.hip) over KPendingDFS; assumed: the call's assumed
// bytes (the witness layout) or null.
template <class M>
__global__ __launch_bounds__(C_LANES) void kpending_search(KTableArgs a, uint32_t pass2, uint8_t* assumed) {
    constexpr int EV = TW<M>::EV, K = TW<M>::CLASS;
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const uint32_t* list = pass2 ? a.heavy_list[K] : a.class_list[K];
    const uint32_t total = a.cnt[(pass2 ? TC_HEAVY : TC_CLASS) + K];
    if ((uint64_t)blockIdx.x * C_LANES >= total) return;

    // LDS: events [EV / 2][64] words, stack [EV][64] words, the component's tables
    uint16_t* ev = reinterpret_cast<uint16_t*>(lds);
    uint32_t* stk = lds + (EV / 2) * C_LANES + lane;
    uint32_t* tab = lds + (EV / 2 + EV) * C_LANES;
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.t.blob);
        uint4* dst = reinterpret_cast<uint4*>(tab);
        for (uint32_t k = lane; k < a.t.blob_words / 4u; k += C_LANES) dst[k] = src[k];
    }
    __syncthreads();
    KPendLds L;
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
        KPendingDFS<M> dfs;
        dfs.depth = 0;
        dfs.nodes = 0;
        dfs.found = 0;
        // -2: no history in this lane
        int status = -2;
        if (active) {
            status = stage_ktable<M>(a, H, ev, lane, dfs) ? -1 : QSMD_STATUS_ENCODE_ERROR;
            if (status == -1) dfs.init(a.state0);
        }
        // the time limit checked every 1024 iterations, as ktable_search
        while (__ballot(status == -1) != 0ull) {
            for (uint32_t k = 0; k < 1024u; ++k) {
                if (status == -1) status = dfs.step(a.t, L, ev, stk, lane, limit);
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
    }
    cnt.flush(a.s.buckets, lane);
}

template <class M>
hipError_t launch_kpending_class(const KTableArgs& p, uint32_t grid, uint32_t pass2, uint8_t* assumed,
                                 hipStream_t s) {
    const size_t lds = table_lds_bytes(p.t, TW<M>::CLASS, false, true);
    if (lds > 64u * 1024u) {
        static std::atomic<int> set[kAttrDevices];
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&kpending_search<M>), set, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((kpending_search<M>), dim3(grid), dim3(C_LANES), lds, s, p, pass2, assumed);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ktable_pending(const KTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3],
                                 uint32_t classes, uint8_t* assumed, hipStream_t s) {
    hipError_t e = launch_ktable_bin(p, s);
    for (uint32_t pass2 = 0; pass2 < (p.budget ? 2u : 1u) && e == hipSuccess; ++pass2) {
        const uint32_t* g = pass2 ? grid2 : grid1;
        if (e == hipSuccess && (classes & 1u)) e = launch_kpending_class<uint32_t>(p, g[0], pass2, assumed, s);
        if (e == hipSuccess && (classes & 2u)) e = launch_kpending_class<uint64_t>(p, g[1], pass2, assumed, s);
        if (e == hipSuccess && (classes & 4u)) e = launch_kpending_class<M128>(p, g[2], pass2, assumed, s);
    }
    if (e != hipSuccess) return e;
    return launch_ktable_finish(p, s);
}

}  // namespace qsmd
