// ksplit.hip -- QSMD_MODEL_KTABLE's local mode (knob "ktable_local",
// include/qsmd.h): a history over independent keys is
// linearisable exactly when each key's sub-history is (Herlihy & Wing,
// Theorem 1), so a *splittable* history is cut into one sub-history per key
// and each is searched on its own by ktable.hip's search, unchanged.
//
//   ksplit_split    per history: decides splittable, writes n_keys sub-headers
//                   (slot h * n_keys + k) and the history's events, grouped by
//                   key, into the workspace copy of the events array.  Key k's
//                   events are contiguous inside the history's own slot
//                   [ev_off, ev_off + n_ev), in history order, bytes unchanged.
//                   A history that is not splittable is copied through: sub-
//                   header 0 is its own header, order kept, the other sub-
//                   headers are empty -- the search then gives it the product's
//                   status and nodes, an encode error included.
//   (launch_table over the sub-headers: api.hip)
//   ksplit_combine  per history: status of the lowest key whose sub-search is
//                   not LINEARISABLE (else LINEARISABLE), nodes the sum; the
//                   call's totals count histories.
//   ksplit_finish   totals from the buckets, the split count for the host.
//
// The keyed pending call's local mode (knob "kpending_local")
// is the same with ksplit_split_pending -- a pid's events may end on an
// invocation -- and launch_ktable_pending over the sub-headers; the split
// count then goes to a probe slot of its own (KSplitArgs::probe_slot).
//
// Splittable = encode-valid by the search's own test (ktable_bin's header test
// and stage_ktable's per event: code < n_inv / n_resp, an invocation's key <
// n_keys) and, per pid, events that alternate invocation, response, ...,
// ending on a response.  A response belongs to the key of the event of its pid
// before it.
//
// One wavefront per history, one lane per event (two rounds past 64 events).
// Pairing is a ballot per pid: the mask of the pid's events gives each of them
// its rank among them (the kind it must have), their number (even) and the
// event before it, whose first word -- read from the LDS copy of the history's
// first words -- carries the key of a response.  The destination is a ballot
// per key: the key's base (the counts of the keys below) plus the lane's rank
// among the key's events.  The events are permuted in LDS and stored in slot
// order, so loads and stores are both contiguous 8-byte-per-lane runs.  Plain
// loads and stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "lane.h"

namespace qsmd {

namespace {

constexpr uint32_t kMaxEv = QSMD_MAX_EVENTS;     // 128: two rounds of 64 lanes
constexpr int kRounds = 2;
constexpr int kMaxKeys = QSMD_KTABLE_MAX_KEYS;

__device__ __forceinline__ qsmd_hdr sub_header(uint32_t off, uint32_t n, const qsmd_hdr& H) {
    qsmd_hdr o;
    o.ev_off = off;
    o.n_ev = (uint16_t)n;
    o.n_pid = H.n_pid;
    o.model_id = (uint8_t)QSMD_MODEL_KTABLE;
    o.tag = H.tag;
    o.reserved = 0;
    return o;
}

// A history's header as the wavefront uses it: the fields in scalar registers,
// ktable_bin's test done.
struct SplitHdr {
    qsmd_hdr H;
    uint32_t ev_off, n_ev;
    bool ok;                                     // (false too for a slot past the batch)
};

__device__ __forceinline__ SplitHdr split_hdr(const KSplitArgs& a, uint64_t h) {
    SplitHdr d;
    d.H = qsmd_hdr{0, 0, 0, 0, 0, 0};
    if (h < a.n_hist) d.H = a.hdr[h];            // every lane the same address
    d.ev_off = __builtin_amdgcn_readfirstlane(d.H.ev_off);
    d.n_ev = __builtin_amdgcn_readfirstlane((uint32_t)d.H.n_ev);
    const uint32_t model = __builtin_amdgcn_readfirstlane((uint32_t)d.H.model_id);
    d.ok = h < a.n_hist && model == QSMD_MODEL_KTABLE && d.n_ev <= kMaxEv &&
           (uint64_t)d.ev_off + d.n_ev <= a.n_events;
    return d;
}

// the lane's events of a history that passed the header test (none otherwise)
__device__ __forceinline__ void split_load(const KSplitArgs& a, const SplitHdr& d, uint32_t lane, uint2 (&w)[kRounds]) {
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t e = (uint32_t)r * C_LANES + lane;
        w[r] = (d.ok && e < d.n_ev) ? a.events[(uint64_t)d.ev_off + e] : make_uint2(0u, 0u);
    }
}

// The loop is pipelined over the workgroup's histories: while history i is
// split, the events of i + 1 and the header of i + 2 are in flight, so a
// wavefront pays neither load's latency per history.
//
// PENDING (the keyed pending call, knob "kpending_local"): a pid's events may
// end on an invocation -- the rank's parity must still match the event's kind,
// the pid's count may be odd.  That last invocation takes its key from its own
// `a` byte like every other one (validated < n_keys by the same test), so the
// destinations are a permutation of the history's slot as before.
template <bool PENDING>
__device__ __forceinline__ void split_histories(const KSplitArgs& a) {
    __shared__ uint32_t lw[kMaxEv];              // the first word of every event
    __shared__ uint2 perm[kMaxEv];               // the events in sub-history order
    const uint32_t lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t stride = gridDim.x;
    uint32_t n_split = 0;                        // (wavefront-uniform)
    SplitHdr cur = split_hdr(a, blockIdx.x);
    uint2 w[kRounds];
    split_load(a, cur, lane, w);
    qsmd_hdr next_raw{0, 0, 0, 0, 0, 0};
    if (blockIdx.x + stride < a.n_hist) next_raw = a.hdr[blockIdx.x + stride];
    for (uint64_t h = blockIdx.x; h < a.n_hist; h += stride) {
        // the next history's events, the header after it
        SplitHdr next;
        next.H = next_raw;
        next.ev_off = __builtin_amdgcn_readfirstlane(next_raw.ev_off);
        next.n_ev = __builtin_amdgcn_readfirstlane((uint32_t)next_raw.n_ev);
        next.ok = h + stride < a.n_hist &&
                  __builtin_amdgcn_readfirstlane((uint32_t)next_raw.model_id) == QSMD_MODEL_KTABLE &&
                  next.n_ev <= kMaxEv && (uint64_t)next.ev_off + next.n_ev <= a.n_events;
        uint2 wn[kRounds];
        split_load(a, next, lane, wn);
        next_raw = qsmd_hdr{0, 0, 0, 0, 0, 0};
        if (h + 2u * stride < a.n_hist) next_raw = a.hdr[h + 2u * stride];

        const qsmd_hdr H = cur.H;
        const uint32_t ev_off = cur.ev_off, n_ev = cur.n_ev;
        qsmd_hdr* sub = a.sub_hdr + h * a.n_keys;
        // a history that fails ktable_bin's test (or is empty) is decided from
        // its header alone there, so its events are not touched here
        if (!cur.ok || n_ev == 0u) {
            if (lane < a.n_keys) sub[lane] = lane == 0u ? H : sub_header(0u, 0u, H);
            n_split += cur.ok ? 1u : 0u;         // (an empty history is split into no part)
        } else {
            bool act[kRounds];
#pragma unroll
            for (int r = 0; r < kRounds; ++r) {
                const uint32_t e = (uint32_t)r * C_LANES + lane;
                act[r] = e < n_ev;
                if (act[r]) lw[e] = w[r].x;
            }
            __syncthreads();
            // per pid (one pass of the loop each): the ballot of its events
            // gives every one of them its rank among them, their number and
            // the event before it
            const bool two = n_ev > (uint32_t)C_LANES;       // (uniform)
            const uint32_t pid[kRounds] = {w[0].x & QSMD_EV_PID_MASK, w[1].x & QSMD_EV_PID_MASK};
            uint32_t rank[kRounds] = {0u, 0u}, cnt[kRounds] = {0u, 0u};
            int before[kRounds] = {-1, -1};                  // the pid's previous event (history-local), or none
            uint64_t todo0 = __ballot(act[0]), todo1 = __ballot(act[1]);
            while ((todo0 | todo1) != 0ull) {
                const uint32_t p = todo0 ? __builtin_amdgcn_readlane(pid[0], __builtin_ctzll(todo0))
                                         : __builtin_amdgcn_readlane(pid[1], __builtin_ctzll(todo1));
                const bool in0 = act[0] && pid[0] == p, in1 = two && act[1] && pid[1] == p;
                const uint64_t m0 = __ballot(in0), m1 = two ? __ballot(in1) : 0ull;
                const uint32_t c0 = (uint32_t)__builtin_popcountll(m0), c1 = (uint32_t)__builtin_popcountll(m1);
                if (in0) {
                    const uint64_t b = m0 & below;
                    rank[0] = (uint32_t)__builtin_popcountll(b);
                    cnt[0] = c0 + c1;
                    before[0] = b ? 63 - __builtin_clzll(b) : -1;
                }
                if (in1) {
                    const uint64_t b = m1 & below;
                    rank[1] = c0 + (uint32_t)__builtin_popcountll(b);
                    cnt[1] = c0 + c1;
                    before[1] = b ? 127 - __builtin_clzll(b) : (m0 ? 63 - __builtin_clzll(m0) : -1);
                }
                todo0 &= ~m0;
                todo1 &= ~m1;
            }
            bool bad = false;
            uint32_t key[kRounds];
#pragma unroll
            for (int r = 0; r < kRounds; ++r) {
                const uint32_t me = w[r].x;
                const bool resp = (me & QSMD_EV_RESP) != 0u;
                const uint32_t prev = (act[r] && before[r] >= 0) ? lw[before[r]] : 0u;
                const uint32_t code = (me >> 8) & 0xFFu, ka = (me >> 16) & 0xFFu;
                // stage_ktable's test
                const bool valid = resp ? code < a.n_resp : (code < a.n_inv && ka < a.n_keys);
                // the pid's events alternate from an invocation and end on a response
                // (PENDING: or on an invocation)
                const bool paired = ((rank[r] & 1u) != 0u) == resp && (PENDING || (cnt[r] & 1u) == 0u);
                bad = bad || (act[r] && !(valid && paired));
                key[r] = (resp ? (prev >> 16) : ka) & 7u;
            }
            if (__ballot(bad) != 0ull) {
                // the product route: one sub-history, the whole history in order
#pragma unroll
                for (int r = 0; r < kRounds; ++r)
                    if (act[r]) a.sub_events[(uint64_t)ev_off + (uint32_t)r * C_LANES + lane] = w[r];
                if (lane < a.n_keys) sub[lane] = lane == 0u ? H : sub_header(0u, 0u, H);
            } else {
                ++n_split;
                uint32_t base = 0u, my_off = 0u, my_cnt = 0u, dst[kRounds] = {0u, 0u};
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)kMaxKeys; ++k) {
                    if (k >= a.n_keys) break;    // (every key here is < n_keys)
                    const uint64_t m0 = __ballot(act[0] && key[0] == k);
                    const uint64_t m1 = two ? __ballot(act[1] && key[1] == k) : 0ull;
                    const uint32_t c0 = (uint32_t)__builtin_popcountll(m0), c1 = (uint32_t)__builtin_popcountll(m1);
                    if (key[0] == k) dst[0] = base + (uint32_t)__builtin_popcountll(m0 & below);
                    if (two && key[1] == k) dst[1] = base + c0 + (uint32_t)__builtin_popcountll(m1 & below);
                    if (lane == k) {
                        my_off = base;
                        my_cnt = c0 + c1;
                    }
                    base += c0 + c1;
                }
                // (every event is counted once under its key: dst < n_ev)
#pragma unroll
                for (int r = 0; r < kRounds; ++r)
                    if (act[r]) perm[dst[r]] = w[r];
                __syncthreads();
#pragma unroll
                for (int r = 0; r < kRounds; ++r) {
                    const uint32_t e = (uint32_t)r * C_LANES + lane;
                    if (act[r]) a.sub_events[(uint64_t)ev_off + e] = perm[e];
                }
                if (lane < a.n_keys) sub[lane] = sub_header(my_cnt ? ev_off + my_off : 0u, my_cnt, H);
            }
            __syncthreads();                     // the next history writes lw and perm
        }
        cur = next;
#pragma unroll
        for (int r = 0; r < kRounds; ++r) w[r] = wn[r];
    }
    if (lane == 0u && n_split) atomicAdd(a.n_split, n_split);
}

__global__ __launch_bounds__(C_LANES) void ksplit_split(KSplitArgs a) { split_histories<false>(a); }

__global__ __launch_bounds__(C_LANES) void ksplit_split_pending(KSplitArgs a) { split_histories<true>(a); }

// One lane per history: the results of its n_keys sub-searches, folded.
__global__ __launch_bounds__(C_LANES) void ksplit_combine(KSplitArgs a) {
    const int lane = threadIdx.x;
    WaveCounters cnt;
    for (uint64_t base = (uint64_t)blockIdx.x * C_LANES; base < a.n_hist; base += (uint64_t)gridDim.x * C_LANES) {
        const uint64_t h = base + lane;
        const bool active = h < a.n_hist;
        int status = QSMD_STATUS_LINEARISABLE;
        uint64_t nodes = 0;
        if (active) {
            for (uint32_t k = 0; k < a.n_keys; ++k) {
                const uint64_t i = h * a.n_keys + k;
                const int s = a.sub_status[i];
                nodes += a.sub_nodes[i];
                if (status == (int)QSMD_STATUS_LINEARISABLE && s != (int)QSMD_STATUS_LINEARISABLE) status = s;
            }
            a.status[h] = (uint8_t)status;
            if (a.nodes) a.nodes[h] = nodes;
        }
        cnt.add(active, status, nodes);
    }
    cnt.flush(a.buckets, lane);
}

__global__ __launch_bounds__(C_LANES) void ksplit_finish(KSplitArgs a) {
    const uint32_t k = threadIdx.x;
    if (k < (uint32_t)T_N) {
        uint64_t v = 0;
        for (uint32_t b = 0; b < kBuckets; ++b) v += a.buckets[(uint64_t)b * kBucketWords + k];
        reinterpret_cast<uint64_t*>(a.totals)[k] = v;
    }
    if (k == 0 && a.probe_host) {
        a.probe_host[a.probe_slot] = *a.n_split;
        __threadfence_system();
    }
}

}  // namespace

hipError_t launch_ksplit(const KSplitArgs& p, uint32_t grid, hipStream_t s, bool pending) {
    if (pending)
        hipLaunchKernelGGL(ksplit_split_pending, dim3(std::max(grid, 1u)), dim3(C_LANES), 0, s, p);
    else
        hipLaunchKernelGGL(ksplit_split, dim3(std::max(grid, 1u)), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_kcombine(const KSplitArgs& p, hipStream_t s) {
    const uint32_t g = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((p.n_hist + 63) / 64, 1), 4096);
    hipLaunchKernelGGL(ksplit_combine, dim3(g), dim3(C_LANES), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ksplit_finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

}  // namespace qsmd
