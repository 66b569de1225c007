// table_lane.h -- what the two table-driven searches share (csrc/table.hip,
// QSMD_MODEL_TABLE; csrc/wtable.hip, QSMD_MODEL_WTABLE): the width classes,
// the mask helpers of the one-lane-per-history DFS, the paired 16-bit LDS
// column, the staging of a history's events and pass 2's state memo.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.h"
#include "lane.h"
#include "mask.h"

namespace qsmd {
namespace tlane {

template <class M> struct TW;
template <> struct TW<uint32_t> { static constexpr int EV = 32, NW = 1, CLASS = 0; };
template <> struct TW<uint64_t> { static constexpr int EV = 64, NW = 2, CLASS = 1; };
template <> struct TW<M128> { static constexpr int EV = 128, NW = 4, CLASS = 2; };

// a mask from its 32-bit words
__device__ __forceinline__ void from_words(const uint32_t* w, uint32_t& m) { m = w[0]; }
__device__ __forceinline__ void from_words(const uint32_t* w, uint64_t& m) { m = w[0] | ((uint64_t)w[1] << 32); }
__device__ __forceinline__ void from_words(const uint32_t* w, M128& m) {
    m = mk128(w[0] | ((uint64_t)w[1] << 32), w[2] | ((uint64_t)w[3] << 32));
}
__device__ __forceinline__ bool t_test(uint32_t m, uint32_t j) { return (m >> j) & 1u; }
__device__ __forceinline__ bool t_test(uint64_t m, uint32_t j) { return (m >> j) & 1ull; }
__device__ __forceinline__ bool t_test(const M128& m, uint32_t j) {
    return ((j < 64u ? m.lo >> j : m.hi >> (j - 64u)) & 1ull) != 0ull;
}
template <class M> __device__ __forceinline__ M t_zero() { return M{}; }
template <class M> __device__ __forceinline__ M t_ones() { return ~M{}; }
template <> __device__ __forceinline__ M128 t_ones<M128>() { return mk128(~0ull, ~0ull); }
template <> __device__ __forceinline__ M128 t_zero<M128>() { return mk128(0ull, 0ull); }
// the highest set bit of x as a mask (zero for x == 0)
template <class M> __device__ __forceinline__ M t_topbit(const M& x) {
    return MaskOps<M>::any(x) ? MaskOps<M>::bit(MaskOps<M>::msb(x)) : t_zero<M>();
}
// takeInvocations (src/Linearisability.hs:25-28): the remaining invocations
// below the first remaining response
template <class M> __device__ __forceinline__ M t_cands(const M& rem, const M& INV, const M& RESP) {
    const M rr = rem & RESP;
    const M c = rem & INV;
    return MaskOps<M>::any(rr) ? c & MaskOps<M>::below(MaskOps<M>::ctz(rr)) : c;
}

// the 16-bit element x of a lane's column (two to a word, [x / 2][lane][x & 1]:
// see table.hip)
__device__ __forceinline__ uint32_t col16(uint32_t x, int lane) {
    return (((x >> 1) * (uint32_t)C_LANES + (uint32_t)lane) << 1) | (x & 1u);
}

__device__ __forceinline__ void to_words(uint32_t m, uint32_t* w) { w[0] = m; }
__device__ __forceinline__ void to_words(uint64_t m, uint32_t* w) { w[0] = (uint32_t)m; w[1] = (uint32_t)(m >> 32); }
__device__ __forceinline__ void to_words(const M128& m, uint32_t* w) {
    w[0] = (uint32_t)m.lo; w[1] = (uint32_t)(m.lo >> 32); w[2] = (uint32_t)m.hi; w[3] = (uint32_t)(m.hi >> 32);
}

// The exact-count state memo of pass 2 (knob "table_memo").
// By Lemma L1 the subtree below a node depends only on (rem, state), and a
// subtree the search backtracks out of has failed after counting a fixed
// number of nodes.  One lane's view: its private direct-mapped table in HBM
// (32 B per entry: count lo | count hi | tag | state | history index, then
// the rem words, zero-padded to four), its LDS column of node counts at
// entry per level, and a 64-bit map of the slots (mod 64) it has written for
// this history, which gates the HBM probe.  `tag` is the call's epoch above
// the state's bits: epoch << 8 for table.hip's 8-bit states, epoch << 16 for
// wtable.hip's 16-bit ones.
template <class M>
struct TableMemo {
    static constexpr int NW = TW<M>::NW;
    uint4* tab;             // the lane's table
    uint64_t* entry;        // LDS: [level][lane], this lane's column
    uint32_t mask;          // entries - 1
    uint32_t tag;           // the epoch, shifted above the state
    uint32_t h;
    uint32_t hits;
    uint64_t wr;
    bool skip;              // the node being left was a hit: recorded already

    __device__ __forceinline__ uint32_t slot_of(const uint32_t* w, uint32_t state) const {
        constexpr uint32_t K[4] = {0x9E3779B1u, 0x85EBCA77u, 0xC2B2AE3Du, 0x27D4EB2Fu};
        uint32_t x = state * 0x165667B1u;
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
    __device__ __forceinline__ void record(const M& rem, uint32_t state, uint64_t count) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        to_words(rem, w);
        const uint32_t slot = slot_of(w, state);
        tab[2u * slot] = make_uint4((uint32_t)count, (uint32_t)(count >> 32), tag | state, h);
        tab[2u * slot + 1u] = make_uint4(w[0], w[1], w[2], w[3]);
        wr |= 1ull << (slot & 63u);
    }
    // the whole key is compared: epoch, state, history, every rem word
    __device__ __forceinline__ bool probe(const M& rem, uint32_t state, uint64_t& count) const {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        to_words(rem, w);
        const uint32_t slot = slot_of(w, state);
        if (!((wr >> (slot & 63u)) & 1ull)) return false;
        const uint4 a = tab[2u * slot], b = tab[2u * slot + 1u];
        count = a.x | ((uint64_t)a.y << 32);
        return a.z == (tag | state) && a.w == h && b.x == w[0] && b.y == w[1] && b.z == w[2] && b.w == w[3];
    }
};

// One lane's record of the deepest path of its search (the explain calls,
// include/qsmd.h qsmd_explain_batch; the EXPLAIN instantiations of the three
// steps).  `best` is the depth of the first node of maximal depth so far,
// `state` the model state after that node's operation (S: uint32_t, keyed
// uint64_t), `common` the lowest depth the stack has fallen back to since the
// last record: the path bytes below it are still the stack's.  A descent that
// passes `best` stores the stack's chosen events of levels [common, depth) --
// at most once per operation of the history, so the divergent byte stores are
// rare and the step pays one compare per descent.  at(d): the chosen event of
// stack level d.
template <class S>
struct DeepPath {
    uint32_t off;           // the history's slot in the path array: ev_off (the base pointer is uniform)
    uint32_t best, common;
    S state;

    __device__ __forceinline__ void begin(uint32_t ev_off, S state0) {
        off = ev_off;
        best = 0u;
        common = 0u;
        state = state0;
    }
    __device__ __forceinline__ void fell_to(uint32_t depth) { common = min(common, depth); }
    template <class At>
    __device__ __forceinline__ void descended(uint8_t* base, uint32_t depth, S now, At at) {
        if (depth > best) {
            uint8_t* path = base + off;
            for (uint32_t d = common; d < depth; ++d) path[d] = (uint8_t)at(d);
            best = depth;
            common = depth;
            state = now;
        }
    }
    // The end of a search: LINEARISABLE and MODEL_ERROR report the current
    // stack (depth, now), the others the record; then the terminator and the
    // qsmd_explain record (depth 16 | 0 16, 0, state lo, state hi).  An
    // ENCODE_ERROR found while staging: the terminator first, the record zero.
    template <class At>
    __device__ __forceinline__ void finish(uint8_t* base, int status, uint32_t n_ev, uint32_t depth, S now, At at,
                                           uint4* rec) {
        uint8_t* path = base + off;
        if (status == QSMD_STATUS_ENCODE_ERROR) {
            path[0] = QSMD_WITNESS_END;
            *rec = make_uint4(0u, 0u, 0u, 0u);
            return;
        }
        if (status == QSMD_STATUS_LINEARISABLE || status == QSMD_STATUS_MODEL_ERROR) {
            for (uint32_t d = 0; d < depth; ++d) path[d] = (uint8_t)at(d);
            best = depth;
            state = now;
        }
        if (best < n_ev) path[best] = QSMD_WITNESS_END;
        const uint64_t st = (uint64_t)state;
        *rec = make_uint4(best, 0u, (uint32_t)st, (uint32_t)(st >> 32));
    }
};

// The lane stages its own history: 8 loads in flight (the index clamped into
// the history), the 16-bit events into its LDS column, the kind and the seven
// pid bits into mask planes one 32-bit word at a time.  Returns false for an
// event the table cannot index (ENCODE_ERROR).  Args: TableArgs / WTableArgs;
// DFS: the lane's search state (INV, RESP, P[7]).
template <class M, class Args, class DFS>
__device__ __forceinline__ bool stage_table(const Args& a, const qsmd_hdr& H, uint16_t* ev, int lane, DFS& dfs) {
    constexpr int NW = TW<M>::NW;
    const uint32_t n_ev = H.n_ev;
    const uint2* evp = a.s.events + H.ev_off;
    const uint32_t last = n_ev - 1u;                 // (n_ev >= 1: the binning kernel)
    uint32_t pl[8][NW];
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int q = 0; q < NW; ++q) pl[b][q] = 0u;
    uint32_t bad = 0u;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
#pragma unroll 1
        for (uint32_t c0 = 0; c0 < 32u; c0 += 8u) {
            const uint32_t e0 = (uint32_t)q * 32u + c0;
            if (e0 >= n_ev) break;
            uint32_t x[8];
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) x[k] = evp[min(e0 + k, last)].x;
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {
                const uint32_t e = e0 + k;
                const bool in = e < n_ev;
                const uint32_t lo = x[k];
                if (in) ev[col16(e, lane)] = (uint16_t)lo;
                const uint32_t bit = in ? 1u << (c0 + k) : 0u;
#pragma unroll
                for (int b = 0; b < 8; ++b) pl[b][q] |= ((lo >> b) & 1u) ? bit : 0u;
                const uint32_t code = (lo >> 8) & 0xFFu;
                bad |= (in && code >= ((lo & QSMD_EV_RESP) ? a.t.n_resp : a.t.n_inv)) ? 1u : 0u;
            }
        }
    }
    const M ALL = MaskOps<M>::below((int)n_ev);
    M resp;
    from_words(pl[7], resp);
    dfs.RESP = resp & ALL;
    dfs.INV = ALL & ~resp;
#pragma unroll
    for (int b = 0; b < 7; ++b) from_words(pl[b], dfs.P[b]);
    return bad == 0u;
}

}  // namespace tlane
}  // namespace qsmd
