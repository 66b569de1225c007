// tgen.hip -- on-device history generation for the table models
// (qsmd_gen_table_batch_device; the stream is defined in include/qsmd_gen.h
// and csrc/gen/tgen.cpp is its host form: the two write the same bytes).
//
// One history per lane, 64 to a one-wavefront workgroup.  Unlike gen.hip
// nothing is indexed in private memory, so the kernel has no scratch:
//   - a client's phase is a bit in each of two 32-bit masks (invoked,
//     executed); a client has at most one ready action, so a tick's pick is
//     the below(n)-th set bit of the ready mask;
//   - the per-client queue counts and the pending invocation / response
//     symbols are bytes in LDS, [x / 4][lane] words (a lane's word in bank
//     lane mod 32, as table.hip's col16 columns);
//   - an event is 16 bits (kp, code) while it is built -- a, b and val are
//     zero -- staged in LDS two to a word, [e / 2][lane] with a row stride of
//     65 words.  The bug edits the staged copy.  After generation the
//     wavefront stores the group's 64 x 2K events, one contiguous range, as
//     16-byte pairs, consecutive lanes to consecutive addresses (the odd
//     stride keeps the transposed read off one bank); the headers and flag
//     bytes are contiguous too.
// The narrow table is copied to LDS by every workgroup (table.hip's blob);
// the wide table is read from device memory by record (wtable.hip's).
// request() for the narrow table reads the state's accept mask, tabulated
// once per workgroup; for the wide table its scan over the invocations has a
// uniform trip count.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tgen.h"
#include "tgen_lane.h"

namespace qsmd {

namespace {

// The model behind one face: acc(s, i) by 32-bit word.
template <bool WIDE> struct Tab;

template <> struct Tab<false> {
    const uint32_t* post;
    const uint32_t* err;          // null: none
    const uint8_t* on_inv;
    const uint8_t* on_resp;
    const uint32_t* accepts;      // [n_states]: bit i set <=> acc(s, i) != 0 (built once per workgroup)
    uint32_t n_inv, n_resp, resp_mask;
    __device__ __forceinline__ uint32_t words() const { return 1u; }
    __device__ __forceinline__ uint32_t word(uint32_t s, uint32_t i, uint32_t) const {
        const uint32_t k = s * n_inv + i;
        return (err ? post[k] & ~err[k] : post[k]) & resp_mask;
    }
    __device__ __forceinline__ uint32_t to(uint32_t s, uint32_t i) const { return on_inv[s * n_inv + i]; }
    __device__ __forceinline__ uint32_t after(uint32_t mid, uint32_t r) const { return on_resp[mid * n_resp + r]; }
};

template <> struct Tab<true> {
    const uint32_t* blob;
    const uint16_t* on_resp;
    uint32_t n_inv, n_resp, pw, rec_words, has_err, last_mask;
    __device__ __forceinline__ uint32_t words() const { return pw; }
    __device__ __forceinline__ uint32_t word(uint32_t s, uint32_t i, uint32_t k) const {
        const uint32_t* rec = blob + ((uint64_t)s * n_inv + i) * rec_words;
        uint32_t x = rec[1u + k];
        if (has_err) x &= ~rec[1u + pw + k];
        return k + 1u == pw ? x & last_mask : x;
    }
    __device__ __forceinline__ uint32_t to(uint32_t s, uint32_t i) const {
        return blob[((uint64_t)s * n_inv + i) * rec_words];
    }
    __device__ __forceinline__ uint32_t after(uint32_t mid, uint32_t r) const {
        return on_resp[(uint64_t)mid * n_resp + r];
    }
};

// request(s): the invocation drawn among those the state accepts a response
// for.
// Narrow table: the enabled set is one word -- the state's accept mask, which
// the workgroup tabulated in LDS, under the mask of positive weights -- so
// with weights of 0 and 1 only (NULL weights included) the pick is the
// below(popcount)-th set bit and nothing is scanned; other weights take two
// scans over registers and launch arguments, no table read.
__device__ __forceinline__ uint32_t request(const TGenArgs& a, const Tab<false>& T, TRng& r, uint32_t s,
                                            uint32_t*, uint32_t) {
    uint32_t e = T.accepts[s] & a.w_mask;
    e = e ? e : a.w_mask;           // nothing accepted here: every positive weight counts
    if (a.w_unit) return nth_bit(e, r.below((uint32_t)__popc(e)));
    const uint32_t n_inv = T.n_inv;
    uint32_t W = 0u;
    for (uint32_t i = 0; i < n_inv; ++i) W += ((e >> i) & 1u) ? a.weight[i] : 0u;
    const uint32_t w = r.below(W);
    uint32_t run = 0u, pick = 0u;
    bool found = false;
    for (uint32_t i = 0; i < n_inv; ++i) {
        const bool on = !found && ((e >> i) & 1u);
        run += on ? a.weight[i] : 0u;
        const bool take = on && run > w;
        pick = take ? i : pick;
        found = found || take;
    }
    return pick;
}

// Wide table: the first scan reads the records, sums the enabled weights and
// keeps the enabled set for the second, which finds the pick, in the lane's
// column of enw ([8][64] words of LDS).  Both trip counts are n_inv in every
// lane.
__device__ __forceinline__ uint32_t request(const TGenArgs& a, const Tab<true>& T, TRng& r, uint32_t s,
                                            uint32_t* enw, uint32_t lane) {
    const uint32_t n_inv = T.n_inv, pw = T.words();
    uint32_t W = 0u, e = 0u;
    for (uint32_t i = 0; i < n_inv; ++i) {
        const uint32_t wgt = a.weight[i];
        if (wgt != 0u) {                                  // (uniform)
            uint32_t any = 0u;
            for (uint32_t k = 0; k < pw; ++k) any |= T.word(s, i, k);
            e |= any ? 1u << (i & 31u) : 0u;
            W += any ? wgt : 0u;
        }
        if ((i & 31u) == 31u || i + 1u == n_inv) {
            enw[(i >> 5) * kLanes + lane] = e;
            e = 0u;
        }
    }
    const bool all = W == 0u;       // nothing accepted here: every positive weight counts
    const uint32_t w = r.below(all ? a.w_all : W);
    uint32_t run = 0u, pick = 0u;
    bool found = false;
    for (uint32_t i = 0; i < n_inv; ++i) {
        if ((i & 31u) == 0u) e = enw[(i >> 5) * kLanes + lane];
        const uint32_t wgt = a.weight[i];
        const bool on = !found && wgt != 0u && (all || ((e >> (i & 31u)) & 1u));
        run += on ? wgt : 0u;
        const bool take = on && run > w;
        pick = take ? i : pick;
        found = found || take;
    }
    return pick;
}

// execute(s, i): the response drawn among the accepted ones, the next state.
// The wide table's record is read twice (count, then locate): the second
// read finds it in cache, and no word of it is held in an indexed array.
template <bool WIDE>
__device__ __forceinline__ uint32_t execute(const Tab<WIDE>& T, TRng& r, uint32_t& s, uint32_t i, uint32_t& flags) {
    const uint32_t pw = T.words(), mid = T.to(s, i);
    uint32_t n = 0u;
    for (uint32_t k = 0; k < pw; ++k) n += (uint32_t)__popc(T.word(s, i, k));
    uint32_t resp;
    if (n) {
        uint32_t k = r.below(n), word = 0u, base = 0u;
        bool found = false;
        for (uint32_t q = 0; q < pw; ++q) {
            const uint32_t x = T.word(s, i, q), c = (uint32_t)__popc(x);
            const bool here = !found && k < c;
            word = here ? x : word;
            base = here ? q * 32u : base;
            k -= (!found && !here) ? c : 0u;
            found = found || here;
        }
        resp = base + nth_bit(word, k);
    } else {
        resp = r.below(T.n_resp);
        flags |= 2u;
    }
    s = T.after(mid, resp);
    return resp;
}

template <bool WIDE>
__global__ __launch_bounds__(kLanes) void tgen_kernel(TGenArgs a) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t C = a.n_clients, K = a.n_ops, P = a.prefix, S = K - P, per = 2u * K;
    // LDS: staged events [K][65] words | queued, pending inv, pending resp:
    // [ceil(C / 4)][64] words each | (wide) the enabled set, (narrow) the
    // accept masks | (narrow) the table blob, 16-byte aligned
    const uint32_t cw = (C + 3u) / 4u * kLanes;
    uint16_t* ev = reinterpret_cast<uint16_t*>(lds);
    uint32_t* qw = lds + K * kEvStride;
    uint8_t* queued = reinterpret_cast<uint8_t*>(qw);
    uint8_t* pinv = reinterpret_cast<uint8_t*>(qw + cw);
    uint8_t* presp = reinterpret_cast<uint8_t*>(qw + 2u * cw);
    // (wide) request()'s enabled set, [8][64] words; (narrow) the states' accept masks, [n_states]
    uint32_t* enw = qw + 3u * cw;
    const uint32_t ew = WIDE ? (uint32_t)(QSMD_WTABLE_MAX_INV / 32) * kLanes : a.t.n_states;

    Tab<WIDE> T;
    if constexpr (WIDE) {
        T.blob = a.wt.blob;
        T.on_resp = reinterpret_cast<const uint16_t*>(a.wt.blob + a.wt.on_resp_off);
        T.n_inv = a.wt.n_inv;
        T.n_resp = a.wt.n_resp;
        T.pw = a.wt.post_words;
        T.rec_words = a.wt.rec_words;
        T.has_err = a.wt.has_err;
        const uint32_t left = a.wt.n_resp - 32u * (a.wt.post_words - 1u);      // 1..32
        T.last_mask = left >= 32u ? ~0u : (1u << left) - 1u;
    } else {
        uint32_t* tab = lds + (K * kEvStride + 3u * cw + ew + 3u) / 4u * 4u;
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
            for (uint32_t i = 0; i < T.n_inv; ++i) m |= T.word(st, i, 0u) ? 1u << i : 0u;
            enw[st] = m;
        }
        T.accepts = enw;
        __syncthreads();
    }
    const uint32_t n_resp = T.n_resp;
    const uint32_t cmask = C >= 32u ? ~0u : (1u << C) - 1u;
    const uint32_t ticks = S * (a.in_window ? 3u : 2u);   // one action per tick, the same count in every lane
    const uint64_t groups = (a.n_hist + kLanes - 1u) / kLanes;

    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        // (a lane past the batch's end generates like the others and stores nothing)
        const uint64_t i = g * kLanes + lane;
        TRng r(a.seed, a.first + i);
        uint32_t s = a.state0, flags = 0u, ne = 0u;
        for (uint32_t x = 0; x < cw; x += kLanes) qw[x + lane] = 0u;

        // ---- sequential prefix
        for (uint32_t k = 0; k < P; ++k) {
            const uint32_t c = r.below(C);
            const uint32_t inv = request(a, T, r, s, enw, lane);
            const uint32_t resp = execute<WIDE>(T, r, s, inv, flags);
            const uint32_t pid = a.shared ? 0u : c;
            ev[ev16(ne++, lane)] = (uint16_t)(pid | (inv << 8));
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
                inv = request(a, T, r, s, enw, lane);
                ev[ev16(ne++, lane)] = (uint16_t)(pid | (inv << 8));
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
                presp[col8(c, lane)] = (uint8_t)execute<WIDE>(T, r, s, inv, flags);
                executed |= bit;
            }
            if (respond) {
                ev[ev16(ne++, lane)] = (uint16_t)(QSMD_EV_RESP | pid | ((uint32_t)presp[col8(c, lane)] << 8));
                invoked &= ~bit;
                executed &= ~bit;
                outstanding--;
            }
        }

        // ---- the bug, on the staged copy
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
            H.model_id = (uint8_t)a.model_id;
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
            out[q] = EvPair{{w & 0xFFFFu, 0u, w >> 16, 0u}};
        }
        __syncthreads();     // the staged words are read before the next group writes them
    }
}

template <bool WIDE>
hipError_t launch(const TGenArgs& a, uint32_t grid, size_t lds, hipStream_t s) {
    if (lds > 64u * 1024u) {
        static std::atomic<int> set[kAttrDevices];
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&tgen_kernel<WIDE>), set, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(tgen_kernel<WIDE>, dim3(grid), dim3(kLanes), lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tgen(const TGenArgs& a, uint32_t n_cu, hipStream_t s) {
    static_assert(sizeof(TGenArgs) < 4096, "kernel arguments: 4 KB at most");
    const bool wide = a.model_id == QSMD_MODEL_WTABLE;
    const uint64_t groups = (a.n_hist + kLanes - 1u) / kLanes;
    const size_t stage = ((size_t)a.n_ops * kEvStride + 3u * ((a.n_clients + 3u) / 4u * kLanes) +
                          (wide ? (size_t)(QSMD_WTABLE_MAX_INV / 32) * kLanes : (size_t)a.t.n_states) + 3u) / 4u * 4u;
    const size_t blob = wide ? 0u : a.t.blob_words;
    // a table every workgroup copies: a few workgroups per CU take the groups in turn
    const uint64_t cap = blob * 4u > 4096u ? 8ull * n_cu : 65536ull;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(groups, cap), 1);
    return wide ? launch<true>(a, grid, (stage + blob) * 4u, s) : launch<false>(a, grid, (stage + blob) * 4u, s);
}

}  // namespace qsmd
