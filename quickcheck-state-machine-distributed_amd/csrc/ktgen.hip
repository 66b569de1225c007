// ktgen.hip -- on-device history generation for the keyed table models
// (qsmd_gen_ktable_batch_device; the stream is defined in include/qsmd_gen.h
// and csrc/gen/ktgen.cpp is its host form: the two write the same bytes).
//
// tgen.hip's narrow kernel on the product model, kept factored.  The layout
// is tgen.hip's: one history per lane, 64 to a one-wavefront workgroup, the
// clients' phases in two masks, byte columns [x / 4][lane], 16-bit staged
// events at a row stride of 65 words, transposed 16-byte stores, the
// component's blob and its states' accept masks in LDS.  What differs:
//   - the state is one uint64_t per lane, key k in bits 8k .. 8k + 7 (as
//     ktable.hip); a key's state is read and written by a shift, so nothing
//     is indexed in private memory and the kernel has no scratch;
//   - an invocation symbol is a byte, key << 5 | i; a staged event is
//     kp (pid 5 bits, kind bit 7) | code << 8 | key << 13, and the store path
//     moves the key into the event's `a`;
//   - request() with weights of 0 and 1 only sums the popcounts of the keys'
//     enabled masks (accepts[s[k]] & w_mask, nothing for a key of weight 0)
//     in a loop of n_keys trips, a byte of one 64-bit word per key, draws
//     once, finds the key by running sum -- one multiplication gives all of
//     them -- and then the n-th set bit of that key's mask: nothing is
//     scanned per invocation.  Other weights take two n_keys x n_inv scans
//     over launch arguments, with uniform trip counts.
// No floating point: unit() < p_bug is an integer compare (api.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ktgen.h"
#include "tgen_lane.h"

namespace qsmd {

namespace {

// the component in LDS
struct KTab {
    const uint32_t* post;
    const uint32_t* err;          // null: none
    const uint8_t* on_inv;
    const uint8_t* on_resp;
    const uint32_t* accepts;      // [n_states]: bit i set <=> acc(s, i) != 0 (built once per workgroup)
    uint32_t n_inv, n_resp, resp_mask;
    __device__ __forceinline__ uint32_t acc(uint32_t s, uint32_t i) const {
        const uint32_t k = s * n_inv + i;
        return (err ? post[k] & ~err[k] : post[k]) & resp_mask;
    }
    __device__ __forceinline__ uint32_t to(uint32_t s, uint32_t i) const { return on_inv[s * n_inv + i]; }
    __device__ __forceinline__ uint32_t after(uint32_t mid, uint32_t r) const { return on_resp[mid * n_resp + r]; }
};

// request(s): the pair drawn among those whose key's state accepts a
// response, as key << 5 | i.  One draw.
// cnt_all: the fallback's counts, byte k = popcount(w_mask) for a key of
// positive weight (uniform).
__device__ __forceinline__ uint32_t request(const KTGenArgs& a, const KTab& T, TRng& r, uint64_t state,
                                            uint64_t cnt_all) {
    const uint32_t nk = a.n_keys;
    if (a.w_unit && nk == 1u) {
        // one key (of weight 1: the weights are not all zero): tgen.hip's request()
        uint32_t e = T.accepts[(uint32_t)state] & a.w_mask;
        e = e ? e : a.w_mask;
        return nth_bit(e, r.below((uint32_t)__popc(e)));
    }
    if (a.w_unit) {
        // The enabled set of key k is one word; W is the sum of the popcounts.
        // A key's count is at most 32, so the counts are a byte each of one
        // 64-bit word, and one multiplication gives every running sum: byte k
        // of cnt * 0x0101..01 is count[0] + .. + count[k] (at most 224 below
        // the top byte, which is not read).
        uint32_t total = 0u;
        uint64_t cnt = 0ull, v = state;
        for (uint32_t k = 0; k < nk; ++k) {
            const uint32_t m = ((a.k_mask >> k) & 1u) ? T.accepts[(uint32_t)v & 0xFFu] & a.w_mask : 0u;
            const uint32_t c = (uint32_t)__popc(m);
            total += c;
            cnt |= (uint64_t)c << (8u * k);
            v >>= 8;
        }
        const bool all = total == 0u;       // nothing accepted here: every pair of positive weight counts
        const uint32_t w = r.below(all ? a.w_all : total);      // < 256
        const uint64_t sums = (all ? cnt_all : cnt) * 0x0101010101010101ull;
        // the key: the first whose running sum exceeds w, i.e. how many of the
        // sums 0 .. 6 do not (a byte at or above n_keys holds the total, which does)
        uint32_t key = 0u;
#pragma unroll
        for (uint32_t k = 0; k + 1u < QSMD_KTABLE_MAX_KEYS; ++k) key += ((uint32_t)(sums >> (8u * k)) & 0xFFu) <= w;
        const uint32_t before = (uint32_t)((sums << 8) >> (8u * key)) & 0xFFu;      // the sum below the key
        const uint32_t own = all ? a.w_mask : T.accepts[(uint32_t)(state >> (8u * key)) & 0xFFu] & a.w_mask;
        return key << 5 | nth_bit(own, w - before);
    }
    // (every product is at most 2^32 - 1 and so is their sum: api.hip)
    const uint32_t n_inv = T.n_inv;
    uint32_t W = 0u;
    uint64_t v = state;
    for (uint32_t k = 0; k < nk; ++k) {
        const uint32_t kw = a.key_weight[k], e = T.accepts[(uint32_t)v & 0xFFu];
        for (uint32_t i = 0; i < n_inv; ++i) W += ((e >> i) & 1u) ? kw * a.inv_weight[i] : 0u;
        v >>= 8;
    }
    const bool all = W == 0u;
    const uint32_t w = r.below(all ? a.w_all : W);
    uint32_t run = 0u, pick = 0u;
    bool found = false;
    v = state;
    for (uint32_t k = 0; k < nk; ++k) {
        const uint32_t kw = a.key_weight[k], e = all ? ~0u : T.accepts[(uint32_t)v & 0xFFu];
        for (uint32_t i = 0; i < n_inv; ++i) {
            const bool on = !found && ((e >> i) & 1u);
            run += on ? kw * a.inv_weight[i] : 0u;
            const bool take = on && run > w;      // (a pair of weight 0 leaves run <= w)
            pick = take ? (k << 5 | i) : pick;
            found = found || take;
        }
        v >>= 8;
    }
    return pick;
}

// execute(s, (k, i)): the response drawn among those the component accepts at
// s[k]; s[k] moves, by the lane's own 64-bit shift.
__device__ __forceinline__ uint32_t execute(const KTab& T, TRng& r, uint64_t& state, uint32_t sym, uint32_t& flags) {
    const uint32_t shift = (sym >> 5) * 8u, i = sym & 31u;
    const uint32_t sk = (uint32_t)(state >> shift) & 0xFFu;
    const uint32_t word = T.acc(sk, i), mid = T.to(sk, i);
    const uint32_t n = (uint32_t)__popc(word);
    uint32_t resp;
    if (n) {
        resp = nth_bit(word, r.below(n));
    } else {
        resp = r.below(T.n_resp);
        flags |= 2u;
    }
    state = (state & ~(0xFFull << shift)) | ((uint64_t)T.after(mid, resp) << shift);
    return resp;
}

// a staged invocation: pid | code << 8 | key << 13 from the symbol key << 5 | i
__device__ __forceinline__ uint32_t staged_inv(uint32_t pid, uint32_t sym) { return pid | (sym << 8); }
// a staged event as the first word of a qsmd_event: {kp, code, a = key, b = 0}
__device__ __forceinline__ uint32_t stored(uint32_t x) { return (x & 0x1FFFu) | ((x >> 13) << 16); }

__global__ __launch_bounds__(kLanes) void ktgen_kernel(KTGenArgs a) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t C = a.n_clients, K = a.n_ops, P = a.prefix, S = K - P, per = 2u * K;
    // LDS: staged events [K][65] words | queued, pending inv, pending resp:
    // [ceil(C / 4)][64] words each | the accept masks [n_states] | the
    // component's blob, 16-byte aligned
    const uint32_t cw = (C + 3u) / 4u * kLanes;
    uint16_t* ev = reinterpret_cast<uint16_t*>(lds);
    uint32_t* qw = lds + K * kEvStride;
    uint8_t* queued = reinterpret_cast<uint8_t*>(qw);
    uint8_t* pinv = reinterpret_cast<uint8_t*>(qw + cw);
    uint8_t* presp = reinterpret_cast<uint8_t*>(qw + 2u * cw);
    uint32_t* accepts = qw + 3u * cw;

    KTab T;
    {
        uint32_t* tab = lds + (K * kEvStride + 3u * cw + a.t.n_states + 3u) / 4u * 4u;
        const uint4* src = reinterpret_cast<const uint4*>(a.t.blob);
        uint4* dst = reinterpret_cast<uint4*>(tab);
        for (uint32_t k = lane; k < a.t.blob_words / 4u; k += kLanes) dst[k] = src[k];
        __syncthreads();
        T.post = tab;
        T.err = a.t.has_err ? tab + table_off_err(a.t) : nullptr;
        T.on_inv = reinterpret_cast<const uint8_t*>(tab + table_off_inv(a.t));
        T.on_resp = reinterpret_cast<const uint8_t*>(tab + table_off_resp(a.t));
        T.n_inv = a.t.n_inv;
        T.n_resp = a.t.n_resp;
        T.resp_mask = a.t.n_resp >= 32u ? ~0u : (1u << a.t.n_resp) - 1u;
        for (uint32_t st = lane; st < a.t.n_states; st += kLanes) {
            uint32_t m = 0u;
            for (uint32_t i = 0; i < T.n_inv; ++i) m |= T.acc(st, i) ? 1u << i : 0u;
            accepts[st] = m;
        }
        T.accepts = accepts;
        __syncthreads();
    }
    const uint32_t n_resp = T.n_resp;
    const uint32_t cmask = C >= 32u ? ~0u : (1u << C) - 1u;
    const uint32_t ticks = S * (a.in_window ? 3u : 2u);   // one action per tick, the same count in every lane
    const uint64_t groups = (a.n_hist + kLanes - 1u) / kLanes;
    uint64_t init = 0ull, cnt_all = 0ull;
    for (uint32_t k = 0; k < a.n_keys; ++k) {
        init = init << 8 | a.state0;
        cnt_all |= (uint64_t)(((a.k_mask >> k) & 1u) ? __popc(a.w_mask) : 0) << (8u * k);
    }

    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        // (a lane past the batch's end generates like the others and stores nothing)
        const uint64_t i = g * kLanes + lane;
        TRng r(a.seed, a.first + i);
        uint64_t s = init;
        uint32_t flags = 0u, ne = 0u;
        for (uint32_t x = 0; x < cw; x += kLanes) qw[x + lane] = 0u;

        // ---- sequential prefix
        for (uint32_t k = 0; k < P; ++k) {
            const uint32_t c = r.below(C);
            const uint32_t inv = request(a, T, r, s, cnt_all);
            const uint32_t resp = execute(T, r, s, inv, flags);
            const uint32_t pid = a.shared ? 0u : c;
            ev[ev16(ne++, lane)] = (uint16_t)staged_inv(pid, inv);
            ev[ev16(ne++, lane)] = (uint16_t)(QSMD_EV_RESP | pid | (resp << 8));
        }

        // ---- concurrent suffix: the clients' operation counts, then one
        //      uniformly chosen ready action per tick
        for (uint32_t k = 0; k < S; ++k) queued[col8(r.below(C), lane)]++;
        uint32_t has_q = 0u;
        for (uint32_t c = 0; c < C; ++c) has_q |= queued[col8(c, lane)] ? 1u << c : 0u;
        uint32_t invoked = 0u, executed = 0u, outstanding = 0u;
        for (uint32_t t = 0; t < ticks; ++t) {
            const uint32_t ready = (outstanding < a.overlap ? ~invoked & has_q & cmask : 0u) | invoked;
            const uint32_t c = nth_bit(ready, r.below((uint32_t)__popc(ready)));
            const uint32_t bit = 1u << c, pid = a.shared ? 0u : c;
            const bool send = !(invoked & bit), respond = (executed & bit) != 0u;
            uint32_t inv;
            if (send) {
                inv = request(a, T, r, s, cnt_all);
                ev[ev16(ne++, lane)] = (uint16_t)staged_inv(pid, inv);
                pinv[col8(c, lane)] = (uint8_t)inv;
                const uint32_t left = queued[col8(c, lane)] - 1u;
                queued[col8(c, lane)] = (uint8_t)left;
                has_q &= left ? ~0u : ~bit;
                invoked |= bit;
                outstanding++;
            } else {
                inv = pinv[col8(c, lane)];
            }
            if (send ? !a.in_window : !respond) {
                presp[col8(c, lane)] = (uint8_t)execute(T, r, s, inv, flags);
                executed |= bit;
            }
            if (respond) {
                ev[ev16(ne++, lane)] = (uint16_t)(QSMD_EV_RESP | pid | ((uint32_t)presp[col8(c, lane)] << 8));
                invoked &= ~bit;
                executed &= ~bit;
                outstanding--;
            }
        }

        // ---- the bug, on the staged copy (a response's staged key bits are 0)
        if (a.bug_draw && (r.next() >> 11) < a.bug_below && S >= 1u) {
            const bool two = n_resp >= 2u;
            const uint32_t coin = two && S >= 2u ? r.below(2u) : 0u;
            const bool change = two && (S < 2u || coin == 0u);
            if (change || S >= 2u) {
                const uint32_t k1 = r.below(S);
                uint32_t k2 = r.below(change ? n_resp - 1u : S);     // change: the code's offset
                if (!change && k2 == k1) k2 = k1 + 1u == S ? 0u : k1 + 1u;
                uint32_t e1 = 0u, e2 = 0u, seen = 0u;
                for (uint32_t e = 2u * P; e < per; ++e) {
                    if (!(ev[ev16(e, lane)] & QSMD_EV_RESP)) continue;
                    e1 = seen == k1 ? e : e1;
                    e2 = seen == k2 ? e : e2;
                    seen++;
                }
                const uint32_t x1 = ev[ev16(e1, lane)];
                if (change) {
                    ev[ev16(e1, lane)] = (uint16_t)((x1 & 0xFFu) | ((((x1 >> 8) + 1u + k2) % n_resp) << 8));
                } else {
                    const uint32_t x2 = ev[ev16(e2, lane)];
                    ev[ev16(e1, lane)] = (uint16_t)((x1 & 0xFFu) | (x2 & 0xFF00u));
                    ev[ev16(e2, lane)] = (uint16_t)((x2 & 0xFFu) | (x1 & 0xFF00u));
                }
                flags |= 1u;
            }
        }

        // ---- headers and flags: a lane's own, 16 B and 1 B apart
        if (i < a.n_hist) {
            qsmd_hdr H;
            H.ev_off = a.ev_base + (uint32_t)(i * per);
            H.n_ev = (uint16_t)per;
            H.n_pid = (uint8_t)(a.shared ? 1u : C);
            H.model_id = (uint8_t)QSMD_MODEL_KTABLE;
            H.tag = (uint32_t)(a.first + i);
            H.reserved = 0u;
            a.hdr[i] = H;
            if (a.bug) a.bug[i] = (uint8_t)flags;
        }

        // ---- events: the group's histories are one contiguous range of
        //      valid * 2K events; pair q = (history q / K, events 2 (q % K) and
        //      the next) is one staged word and 16 bytes out
        __syncthreads();
        const uint32_t valid = (uint32_t)min((uint64_t)kLanes, a.n_hist - g * kLanes);
        EvPair* out = reinterpret_cast<EvPair*>(a.events + g * kLanes * per);
        const uint32_t pairs = valid * K;
        for (uint32_t q = lane; q < pairs; q += kLanes) {
            const uint32_t h = q / K, e2 = q - h * K;
            const uint32_t w = lds[e2 * kEvStride + h];
            out[q] = EvPair{{stored(w & 0xFFFFu), 0u, stored(w >> 16), 0u}};
        }
        __syncthreads();     // the staged words are read before the next group writes them
    }
}

}  // namespace

// LDS at the largest launch (K = 64, C = 32, a 256 x 32 x 32 component with
// post_err): 64 * 65 * 4 = 16,640 B of staged events, 3 * 8 * 64 * 4 = 6,144 B
// of byte columns, 1,024 B of accept masks and the 81,920 B blob: 105,728 B of
// the CU's 160 KB, one workgroup to a CU there.  Past 64 KB the kernel's
// dynamic-LDS limit is raised first.
hipError_t launch_ktgen(const KTGenArgs& a, uint32_t n_cu, hipStream_t s) {
    static_assert(sizeof(KTGenArgs) < 4096, "kernel arguments: 4 KB at most");
    const uint64_t groups = (a.n_hist + kLanes - 1u) / kLanes;
    const size_t stage = ((size_t)a.n_ops * kEvStride + 3u * ((a.n_clients + 3u) / 4u * kLanes) +
                          (size_t)a.t.n_states + 3u) / 4u * 4u;
    const size_t lds = (stage + a.t.blob_words) * 4u;
    // a blob every workgroup copies: a few workgroups per CU take the groups in turn
    const uint64_t cap = a.t.blob_words * 4u > 4096u ? 8ull * n_cu : 65536ull;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(groups, cap), 1);
    if (lds > 64u * 1024u) {
        static std::atomic<int> set[kAttrDevices];
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&ktgen_kernel), set, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ktgen_kernel, dim3(grid), dim3(kLanes), lds, s, a);
    return hipGetLastError();
}

}  // namespace qsmd
