// table_search.h -- the one-lane-per-history search of the table models, once.
//
// Five translation units instantiate it: table.hip (QSMD_MODEL_TABLE),
// wtable.hip (QSMD_MODEL_WTABLE) and ktable.hip (QSMD_MODEL_KTABLE) with the
// reference's rule, tpending.hip and kpending.hip with the pending rule on the
// narrow and the keyed model.  Each holds its model policy, its __global__
// entry points and its launch_* functions; everything else is here.
//
// One lane per history runs the reference DFS over the Lemma L1 event bitset
//  for any history the encoding holds: up to 128 events, 128
// pids (bit-sliced into seven mask planes), shared pids.  Three width classes
// (32-, 64-, 128-event masks): a bin kernel sorts the headers into three index
// lists, one launch per class and pass.  Pass 1 runs under a node budget
// ("table_budget"); a search over it goes to the class's heavy list, which
// pass 2 searches again from the root, so the node counts stay the
// reference's.  A finish kernel sums the totals.
//
// The three axes:
//   * Model (MD): the argument and state types, the staged 16-bit event, the
//     lookup of one step (look / next / moved / undone), the stack of the
//     check rule, whether a workgroup copies the tables to LDS, the memo's
//     entry.  NarrowTables below serves the narrow and the keyed model;
//   * Rule (CheckRule / PendingRule): the step, the root rule of finish(), the
//     stack, the witness writer, the hits counter;
//   * Options: M (the width class), MEMO (pass 2's exact-count state memo),
//     EXPLAIN (the deepest-path record; check rule only).
//
// LDS of one workgroup: events [EV / 2][64] words | stack | (MEMO: the node
// counts at entry, one u64 per stack level and lane) | (the tables).  The
// 16-bit events, and the 16-bit stack levels of the narrow and keyed check
// searches, are stored two to a 32-bit word, [x / 2][lane][x & 1]: the word a
// lane touches is in bank lane % 32 whatever x is, so the per-lane indexed
// reads and writes of a divergent wavefront are conflict-free ([x][lane] with
// 16-bit elements would put lanes 2k and 2k + 1 on one bank with different
// rows).  A 32-bit stack is [level][lane].  The check rule descends at most
// EV / 2 levels (a level removes an invocation and a response), the pending
// rule EV (a history of invocations only descends once per invocation).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "lane.h"
#include "mask.h"

namespace qsmd {
namespace tsearch {

template <class M> struct TW;
template <> struct TW<uint32_t> { using Mask = uint32_t; static constexpr int EV = 32, NW = 1, CLASS = 0; };
template <> struct TW<uint64_t> { using Mask = uint64_t; static constexpr int EV = 64, NW = 2, CLASS = 1; };
template <> struct TW<M128> { using Mask = M128; static constexpr int EV = 128, NW = 4, CLASS = 2; };

// a mask from its 32-bit words
__device__ __forceinline__ void from_words(const uint32_t* w, uint32_t& m) { m = w[0]; }
__device__ __forceinline__ void from_words(const uint32_t* w, uint64_t& m) { m = w[0] | ((uint64_t)w[1] << 32); }
__device__ __forceinline__ void from_words(const uint32_t* w, M128& m) {
    m = mk128(w[0] | ((uint64_t)w[1] << 32), w[2] | ((uint64_t)w[3] << 32));
}
__device__ __forceinline__ void to_words(uint32_t m, uint32_t* w) { w[0] = m; }
__device__ __forceinline__ void to_words(uint64_t m, uint32_t* w) { w[0] = (uint32_t)m; w[1] = (uint32_t)(m >> 32); }
__device__ __forceinline__ void to_words(const M128& m, uint32_t* w) {
    w[0] = (uint32_t)m.lo; w[1] = (uint32_t)(m.lo >> 32); w[2] = (uint32_t)m.hi; w[3] = (uint32_t)(m.hi >> 32);
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

// the 16-bit element x of a lane's column (two to a word: the header comment)
__device__ __forceinline__ uint32_t col16(uint32_t x, int lane) {
    return (((x >> 1) * (uint32_t)C_LANES + (uint32_t)lane) << 1) | (x & 1u);
}

// A workgroup's DFS stacks.  Stack16: 16-bit levels in col16's paired words;
// Stack32: [level][lane], `col` being the lane's own column.
struct Stack16 {
    static constexpr int kBytes = 2;
    uint16_t* base;
    __device__ __forceinline__ Stack16(uint32_t* words, int) : base(reinterpret_cast<uint16_t*>(words)) {}
    __device__ __forceinline__ uint32_t get(uint32_t d, int lane) const { return base[col16(d, lane)]; }
    __device__ __forceinline__ void put(uint32_t d, int lane, uint32_t v) const { base[col16(d, lane)] = (uint16_t)v; }
};
struct Stack32 {
    static constexpr int kBytes = 4;
    uint32_t* col;
    __device__ __forceinline__ Stack32(uint32_t* words, int lane) : col(words + lane) {}
    __device__ __forceinline__ uint32_t get(uint32_t d, int) const { return col[d * C_LANES]; }
    __device__ __forceinline__ void put(uint32_t d, int, uint32_t v) const { col[d * C_LANES] = v; }
};

// The memo's entry in HBM.  MemoEntry32<SHIFT>, the 32-bit states: 32 B =
// 2 x uint4, count lo | count hi | tag | history index, then the rem words
// zero-padded to four; the tag word is the call's epoch above the state's
// bits (SHIFT 8: narrow, 24 | 8; SHIFT 16: wide, 16 | 16).
template <int SHIFT>
struct MemoEntry32 {
    static constexpr uint32_t kQuads = 2;
    static __device__ __forceinline__ uint32_t tag_of(uint32_t epoch) { return epoch << SHIFT; }
    template <int NW>
    static __device__ __forceinline__ void store(uint4* e, uint64_t count, uint32_t tag, uint32_t h, uint32_t state,
                                                 const uint32_t* w) {
        e[0] = make_uint4((uint32_t)count, (uint32_t)(count >> 32), tag | state, h);
        e[1] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    template <int NW>
    static __device__ __forceinline__ bool load(const uint4* e, uint64_t& count, uint32_t tag, uint32_t h,
                                                uint32_t state, const uint32_t* w) {
        const uint4 a = e[0], b = e[1];
        count = a.x | ((uint64_t)a.y << 32);
        return a.z == (tag | state) && a.w == h && b.x == w[0] && b.y == w[1] && b.z == w[2] &&
               b.w == w[3];
    }
};
// MemoEntry48, the keyed 64-bit state: one size for every width class, 48 B =
// 3 x uint4,
//     [0]  count lo | count hi | epoch (a full word) | history index
//     [1]  state lo | state hi | rem word 0 | rem word 1
//     [2]  rem word 2 | rem word 3 | 0 | 0        (128-event class only)
// The 32- and 64-event classes read and write [0] and [1] only.  The epoch and
// the history index stand in the same place for every class, so an entry left
// by another class or another call never matches.
struct MemoEntry48 {
    static constexpr uint32_t kQuads = 3;
    static __device__ __forceinline__ uint32_t tag_of(uint32_t epoch) { return epoch; }
    template <int NW>
    static __device__ __forceinline__ void store(uint4* e, uint64_t count, uint32_t epoch, uint32_t h, uint64_t state,
                                                 const uint32_t* w) {
        e[0] = make_uint4((uint32_t)count, (uint32_t)(count >> 32), epoch, h);
        e[1] = make_uint4((uint32_t)state, (uint32_t)(state >> 32), w[0], w[1]);
        if constexpr (NW > 2) e[2] = make_uint4(w[2], w[3], 0u, 0u);
    }
    template <int NW>
    static __device__ __forceinline__ bool load(const uint4* e, uint64_t& count, uint32_t epoch, uint32_t h,
                                                uint64_t state, const uint32_t* w) {
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

// The exact-count state memo of pass 2.  By Lemma L1 the
// subtree below a node depends only on (rem, state), and a subtree the search
// backtracks out of has failed after counting a fixed number of nodes.  One
// lane's view: its private direct-mapped table in HBM (entries of E), its LDS
// column of node counts at entry per level, and a 64-bit map of the slots
// (mod 64) it has written for this history, which gates the HBM probe.  A hit
// compares the whole key -- epoch, history, state, every rem word -- never the
// hash alone.  S: the model's state type.
template <class M, class S, class E>
struct TableMemo {
    static constexpr int NW = TW<M>::NW;
    uint4* tab;             // the lane's table
    uint64_t* entry;        // LDS: [level][lane], this lane's column
    uint32_t mask;          // entries - 1
    uint32_t tag;           // the call's epoch as the entry holds it (E::tag_of)
    uint32_t h;
    uint32_t hits;
    uint64_t wr;
    bool skip;              // the node being left was a hit: recorded already

    // (the high state word is 0 for a 32-bit state)
    __device__ __forceinline__ uint32_t slot_of(const uint32_t* w, S state) const {
        constexpr uint32_t K[4] = {0x9E3779B1u, 0x85EBCA77u, 0xC2B2AE3Du, 0x27D4EB2Fu};
        uint32_t x = (uint32_t)state * 0x165667B1u;
        if constexpr (sizeof(S) > 4) x ^= (uint32_t)((uint64_t)state >> 32) * 0xD6E8FEB9u;
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
    __device__ __forceinline__ void record(const M& rem, S state, uint64_t count) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        to_words(rem, w);
        const uint32_t slot = slot_of(w, state);
        E::template store<NW>(tab + E::kQuads * slot, count, tag, h, state, w);
        wr |= 1ull << (slot & 63u);
    }
    __device__ __forceinline__ bool probe(const M& rem, S state, uint64_t& count) const {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        to_words(rem, w);
        const uint32_t slot = slot_of(w, state);
        if (!((wr >> (slot & 63u)) & 1ull)) return false;
        return E::template load<NW>(tab + E::kQuads * slot, count, tag, h, state, w);
    }
};

// One lane's record of the deepest path of its search (the explain calls,
// include/qsmd.h qsmd_explain_batch; the EXPLAIN instantiations of the check
// step).  `best` is the depth of the first node of maximal depth so far,
// `state` the model state after that node's operation, `common` the lowest
// depth the stack has fallen back to since the last record: the path bytes
// below it are still the stack's.  A descent that passes `best` stores the
// stack's chosen events of levels [common, depth) -- at most once per
// operation of the history, so the divergent byte stores are rare and the step
// pays one compare per descent.  at(d): the chosen event of stack level d.
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

// ------------------------------------------------------------------ models
// The tables of a narrow model (internal.h TableDev) in LDS, as the narrow and
// the keyed model read them: a step from component state c with invocation
// symbol i and response symbol r is
//     post  = bit r of post[c][i]            (postcondition m inv resp)
//     raise = bit r of post_err[c][i]        (the postcondition raises; wins)
//     next  = on_resp[on_inv[c][i]][r]       (transition twice, src/Linearisability.hs:63-65)
// A model adds how the component is found in its state and its event element.
struct NarrowTables {
    static constexpr bool kLdsBlob = true;
    using CheckStack = Stack16;

    const uint32_t* post;
    const uint32_t* post_err;     // null: none
    const uint8_t* on_inv;
    const uint8_t* on_resp;
    uint32_t n_inv, n_resp;
    uint32_t symbols;             // the bits below n_resp (the pending rule's allowed mask)

    __device__ __forceinline__ void bind(const TableDev& t, const uint32_t* tab) {
        post = tab;
        post_err = t.has_err ? tab + table_off_err(t) : nullptr;
        on_inv = reinterpret_cast<const uint8_t*>(tab + table_off_inv(t));
        on_resp = reinterpret_cast<const uint8_t*>(tab + table_off_resp(t));
        n_inv = t.n_inv;
        n_resp = t.n_resp;
        symbols = t.n_resp >= 32u ? ~0u : (1u << t.n_resp) - 1u;
    }
    // What a step reads for (component state c, invocation i, response rc):
    // post and raise (ok, err), the two postcondition words whole (the pending
    // rule's; bit rc of each), `save` for the stack level.
    struct Look {
        uint32_t idx, rc, ok, err, pw, ew, save, shift;
    };
    __device__ __forceinline__ Look look_at(uint32_t c, uint32_t i, uint32_t rc, uint32_t shift) const {
        const uint32_t idx = c * n_inv + i;
        const uint32_t ok = (post[idx] >> rc) & 1u;
        const uint32_t err = post_err ? (post_err[idx] >> rc) & 1u : 0u;
        return {idx, rc, ok, err, post[idx], post_err ? post_err[idx] : 0u, c, shift};
    }
    // the same entry with response symbol rc (the pending rule's assumed response)
    static __device__ __forceinline__ Look with_response(Look k, uint32_t rc) {
        k.rc = rc;
        return k;
    }
    __device__ __forceinline__ uint32_t next(const Look& k) const {
        return on_resp[(uint32_t)on_inv[k.idx] * n_resp + k.rc];
    }
    // the response symbols the model allows at (c, i): the pending rule
    __device__ __forceinline__ uint32_t allowed(uint32_t c, uint32_t i) const {
        const uint32_t idx = c * n_inv + i;
        return post[idx] & ~(post_err ? post_err[idx] : 0u) & symbols;
    }
};

// QSMD_MODEL_TABLE (table.hip, tpending.hip): the state is the component.  An
// event is the low half of its first word, pid 7 | kind 1 | code 8; a stack
// level saves the whole state.
struct NarrowModel : NarrowTables {
    using Args = TableArgs;
    using State = uint32_t;
    using MemoEntry = MemoEntry32<8>;
    static constexpr uint32_t kModelId = QSMD_MODEL_TABLE;

    static __device__ __forceinline__ uint32_t code(uint32_t e) { return e >> 8; }
    // an event's first word as it is staged: the 16-bit element, and whether
    // the tables cannot index it
    struct Staged {
        uint32_t lo;
        template <class A>
        __device__ __forceinline__ Staged(const A&, uint32_t w) : lo(w) {}
        __device__ __forceinline__ uint16_t element() const { return (uint16_t)lo; }
        template <class A>
        __device__ __forceinline__ uint32_t invalid(const A& a) const {
            return ((lo >> 8) & 0xFFu) >= ((lo & QSMD_EV_RESP) ? a.t.n_resp : a.t.n_inv) ? 1u : 0u;
        }
    };
    __device__ __forceinline__ Look look(State state, uint32_t ej, uint32_t er) const {
        return look_at(state, code(ej), code(er), 0u);
    }
    static __device__ __forceinline__ State moved(State, const Look&, uint32_t next) { return next; }
    static __device__ __forceinline__ State undone(State, uint32_t saved, const uint16_t*, uint32_t, int) {
        return saved;
    }
};

// QSMD_MODEL_KTABLE (ktable.hip, kpending.hip): the product of n_keys copies
// of one narrow component.  The state is the 8 component bytes in one 64-bit
// register pair; s[k] is read and written with 64-bit shifts on the lane's own
// k, so the model is never in memory.  An event stays 16 bits: pid 7 | kind 1 |
// code 5 | key 3 (the component has at most 32 symbols; a response's key bits
// are 0; an invocation's key is validated < n_keys, so every shift is <= 56).
// A stack level saves the one byte s[k] had before the step, k being the
// chosen event's key: undo reads the key from that event, never from the
// pid's previous operation, and restores that byte.
struct KeyedModel : NarrowTables {
    using Args = KTableArgs;
    using State = uint64_t;
    using MemoEntry = MemoEntry48;
    static constexpr uint32_t kModelId = QSMD_MODEL_KTABLE;

    static __device__ __forceinline__ uint32_t code(uint32_t e) { return (e >> 8) & 31u; }
    static __device__ __forceinline__ uint32_t key_shift(uint32_t e) { return (e >> 13) * 8u; }
    // (a response carries no key; an invocation's must be < n_keys)
    struct Staged {
        uint32_t elem, bad;
        __device__ __forceinline__ Staged(const Args& a, uint32_t lo) {
            const bool resp = (lo & QSMD_EV_RESP) != 0u;
            const uint32_t c = (lo >> 8) & 0xFFu, key = resp ? 0u : (lo >> 16) & 0xFFu;
            bad = (c >= (resp ? a.t.n_resp : a.t.n_inv) || key >= a.n_keys) ? 1u : 0u;
            elem = (lo & 0xFFu) | ((c & 31u) << 8) | ((key & 7u) << 13);
        }
        __device__ __forceinline__ uint16_t element() const { return (uint16_t)elem; }
        __device__ __forceinline__ uint32_t invalid(const Args&) const { return bad; }
    };
    __device__ __forceinline__ Look look(State state, uint32_t ej, uint32_t er) const {
        const uint32_t shift = key_shift(ej);
        return look_at((uint32_t)(state >> shift) & 0xFFu, code(ej), code(er), shift);
    }
    // s[k] from `was` to `now` (shift = 8k): one 64-bit shift and an xor
    static __device__ __forceinline__ State put(State state, uint32_t shift, uint32_t was, uint32_t now) {
        return state ^ ((uint64_t)(was ^ now) << shift);
    }
    static __device__ __forceinline__ State moved(State state, const Look& k, uint32_t next) {
        return put(state, k.shift, k.save, next);
    }
    static __device__ __forceinline__ State undone(State state, uint32_t saved, const uint16_t* ev, uint32_t j,
                                                   int lane) {
        const uint32_t shift = key_shift(ev[col16(j, lane)]);
        return put(state, shift, (uint32_t)(state >> shift) & 0xFFu, saved);
    }
};

// ------------------------------------------------------------- the lane
// One lane's search state (registers) over its LDS columns.  S: the model's
// state type.
template <class M, class S>
struct TableLane {
    using MO = MaskOps<M>;
    M INV, RESP, P[7];
    M rem, cand;
    S state;
    uint32_t depth, found;
    uint64_t nodes;

    // the events of event j's pid (the bits beyond the history are junk:
    // every use ANDs with INV or RESP)
    __device__ __forceinline__ M same_pid(uint32_t j) const {
        M acc = t_ones<M>();
#pragma unroll
        for (int b = 0; b < 7; ++b) acc = acc & (t_test(P[b], j) ? P[b] : ~P[b]);
        return acc;
    }

    __device__ __forceinline__ void init(S state0) {
        rem = INV | RESP;
        cand = t_cands(rem, INV, RESP);
        state = state0;
        depth = 0;
        found = 0;
        nodes = 0;
    }

    // A step returns -1 = go on, kTerm = the search ended (finish()), or
    // QSMD_STATUS_BUDGET (limit nodes counted; nothing moved) /
    // QSMD_STATUS_MODEL_ERROR.
    static constexpr int kTerm = 64;
    // a leaf => True (any' []), the root without a child => False (any []);
    // PENDING: but True when the history holds no response (nothing was
    // observed: every operation dropped)
    template <bool PENDING>
    __device__ __forceinline__ int finish(int status) const {
        if (status != kTerm) return status;
        const bool lin = !found && (depth > 0 || (PENDING && !MO::any(RESP)));
        return lin ? QSMD_STATUS_LINEARISABLE : QSMD_STATUS_NONLINEARISABLE;
    }

    // MEMO, in a backtrack: (rem, state) are still the node's being left; it
    // is recorded with the nodes counted below it (not when it was itself a hit)
    template <class Memo>
    __device__ __forceinline__ void memo_leave(Memo& mm) {
        if (!mm.skip) mm.record(rem, state, nodes - mm.entry[depth * C_LANES]);
        mm.skip = false;
    }
    // MEMO, after a descent: the child's (rem, state) is probed; a hit counts
    // the recorded nodes and backtracks at once (the rule of memo.hip's
    // memo_step).  Returns the step's result.
    template <class Memo>
    __device__ __forceinline__ int memo_enter(Memo& mm, uint64_t limit) {
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
        return -1;
    }

    // One iteration of the reference's rule, as LaneDFS::step (lane.h): an
    // optional backtrack, then one candidate.  A stack level is chosen event
    // 8 | what MD saves of the state before the step (Look::save).
    // EXPLAIN (never with MEMO): xp records the deepest path into `path`.
    template <class MD, bool MEMO, bool EXPLAIN, class Stk, class Memo>
    __device__ __forceinline__ int check_step(const MD& md, const uint16_t* ev, const Stk& stk, int lane,
                                              uint64_t limit, Memo& mm, DeepPath<S>& xp, uint8_t* path) {
        const bool empty = !MO::any(cand);
        // no children: a leaf => True, the root => False
        if (empty && (found == 0u || depth == 0u)) return kTerm;
        if (empty) {
            // backtrack: the parent's remaining set by Lemma L1 (the last
            // removed events of the pid are the highest removed ones), its
            // state from the stack
            --depth;
            if constexpr (EXPLAIN) xp.fell_to(depth);
            if constexpr (MEMO) memo_leave(mm);
            const uint32_t st = stk.get(depth, lane);
            const uint32_t j = st & 0xFFu;
            state = md.undone(state, st >> 8, ev, j, lane);
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
        const auto k = md.look(state, ev[col16(j, lane)], ev[col16(r, lane)]);
        ++nodes;
        found = 1u;
        if (k.err) return QSMD_STATUS_MODEL_ERROR;
        if (k.ok) {
            stk.put(depth, lane, j | (k.save << 8));
            ++depth;
            state = md.moved(state, k, md.next(k));
            // the pid's first remaining invocation (quirk Q1: not always j) and response
            rem = rem & ~(MO::lowest(rem & pmj & INV) | MO::bit((int)r));
            cand = t_cands(rem, INV, RESP);
            found = 0u;
            if constexpr (EXPLAIN)
                xp.descended(path, depth, state, [&](uint32_t d) { return stk.get(d, lane) & 0xFFu; });
            if constexpr (MEMO) return memo_enter(mm, limit);
        }
        return -1;
    }

    // One iteration of the pending rule: where findResponse
    // gives [] the candidate has one child per response symbol the model
    // allows, ascending -- an *assumed* response: a counted node whose
    // postcondition is not evaluated again, whose remaining set loses the
    // pid's first remaining invocation and no response.  A stack level is one
    // 32-bit word: chosen event 8 | what MD saves 8 | assumed symbol 5 (bits
    // 16..20) | assumed flag (bit 21).  The backtrack out of an assumed level
    // restores only the pid's highest removed invocation (the highest removed
    // response of the pid belongs to an earlier, completed operation) and goes
    // on with the next allowed symbol above the one popped, the mask read
    // again at the restored state.  Below a node the search is a function of
    // (rem, state) alone, so MEMO is check_step's rule, for a descent of
    // either kind.
    static constexpr uint32_t kAssumed = 1u << 21;
    template <class MD, bool MEMO, class Memo>
    __device__ __forceinline__ int pending_step(const MD& md, const uint16_t* ev, const Stack32& stk, int lane,
                                                uint64_t limit, Memo& mm) {
        const bool empty = !MO::any(cand);
        if (empty && (found == 0u || depth == 0u)) return kTerm;
        uint32_t am = 0u, j = 0u;       // the assumed symbols still to try for candidate j
        if (empty) {
            --depth;
            if constexpr (MEMO) memo_leave(mm);
            const uint32_t st = stk.get(depth, lane);
            j = st & 0xFFu;
            const uint32_t saved = (st >> 8) & 0xFFu;
            state = md.undone(state, saved, ev, j, lane);
            const M gone = ~rem & same_pid(j);
            rem = rem | t_topbit<M>(gone & INV);
            if (st & kAssumed) {
                // the symbols above the one popped (2u << 31 == 0: none)
                const uint32_t r = (st >> 16) & 31u;
                am = md.allowed(saved, MD::code(ev[col16(j, lane)])) & ~((2u << r) - 1u);
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
        // either kind of child are in flight together
        const uint32_t r = observed ? (uint32_t)MO::ctz(rr) : j;
        auto k = md.look(state, ev[col16(j, lane)], ev[col16(r, lane)]);
        uint32_t word;
        if (observed) {
            // an observed response: check_step's child
            if (nodes >= limit) return QSMD_STATUS_BUDGET;
            ++nodes;
            found = 1u;
            if ((k.ew >> k.rc) & 1u) return QSMD_STATUS_MODEL_ERROR;
            if (!((k.pw >> k.rc) & 1u)) return -1;
            word = j | (k.save << 8);
            rem = rem & ~MO::bit((int)r);
        } else {
            // findResponse => []: one child per allowed symbol, none tested
            if (am == 0u) am = k.pw & ~k.ew & md.symbols;
            if (am == 0u) return -1;                 // no symbol: no child, no node
            if (nodes >= limit) return QSMD_STATUS_BUDGET;
            const uint32_t rc = (uint32_t)__builtin_ctz(am);
            k = MD::with_response(k, rc);
            ++nodes;
            word = j | (k.save << 8) | (rc << 16) | kAssumed;
        }
        stk.put(depth, lane, word);
        ++depth;
        state = md.moved(state, k, md.next(k));
        rem = rem & ~MO::lowest(rem & pmj & INV);    // the pid's first remaining invocation (quirk Q1)
        cand = t_cands(rem, INV, RESP);
        found = 0u;
        if constexpr (MEMO) return memo_enter(mm, limit);
        return -1;
    }
};

// The lane stages its own history: 8 loads in flight (the index clamped into
// the history), the 16-bit events (MD::Staged: the element, and whether the
// tables cannot index it) into its LDS column, the kind and the seven pid bits
// into mask planes one 32-bit word at a time.  Returns false for an event the
// model cannot index (ENCODE_ERROR).
template <class M, class MD, class Lane>
__device__ __forceinline__ bool stage_events(const typename MD::Args& a, const qsmd_hdr& H, uint16_t* ev, int lane,
                                             Lane& dfs) {
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
                const typename MD::Staged sv(a, lo);
                if (in) ev[col16(e, lane)] = sv.element();
                const uint32_t bit = in ? 1u << (c0 + k) : 0u;
#pragma unroll
                for (int b = 0; b < 8; ++b) pl[b][q] |= ((lo >> b) & 1u) ? bit : 0u;
                bad |= in ? sv.invalid(a) : 0u;
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

// ------------------------------------------------------------------- rules
struct CheckRule {
    static constexpr bool kPending = false;
    static constexpr uint32_t kHits = TC_HITS;
    template <class MD> using Stack = typename MD::CheckStack;
};
struct PendingRule {
    static constexpr bool kPending = true;
    static constexpr uint32_t kHits = TC_PHITS;      // the pending call's own ("pending_memo")
    template <class MD> using Stack = Stack32;
};

// stack levels of a class, and the LDS words of one workgroup before the tables
template <class R, int EV> constexpr int kLevels = R::kPending ? EV : EV / 2;
template <class MD, class R, class M, bool MEMO>
constexpr size_t search_lds_words() {
    constexpr int EV = TW<M>::EV, LV = kLevels<R, EV>;
    return (size_t)(EV / 2 + LV * R::template Stack<MD>::kBytes / 4 + (MEMO ? 2 * LV : 0)) * C_LANES;
}

// ----------------------------------------------------------------- kernels
// Sort the headers into the three class lists; the histories decided from
// the header alone get their result here.
template <class Args>
__device__ __forceinline__ void bin_body(const Args& a, uint32_t model_id) {
    const int lane = threadIdx.x;
    WaveCounters cnt;
    for (uint64_t base = (uint64_t)blockIdx.x * C_LANES; base < a.s.n_hist; base += (uint64_t)gridDim.x * C_LANES) {
        const uint64_t h = base + lane;
        const bool active = h < a.s.n_hist;
        qsmd_hdr H{0, 0, 0, 0, 0, 0};
        if (active) H = a.s.hdr[h];
        const bool enc_ok = H.model_id == model_id && H.n_ev <= QSMD_MAX_EVENTS &&
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

// One class and pass of a call.  pass2 false: the class list with the pass-1
// budget; true: the class's heavy list, every search to its end.  MEMO: pass 2
// with the state memo (a.memo: one table of a.memo_entries entries per lane
// slot of the grid).  assumed (pending rule): the call's assumed bytes (the
// witness layout) or null.
template <class MD, class R, class M, bool MEMO, bool EXPLAIN>
__device__ __forceinline__ void search_body(typename MD::Args a, uint32_t pass2, uint8_t* assumed) {
    using S = typename MD::State;
    using Lane = TableLane<M, S>;
    using Stk = typename R::template Stack<MD>;
    using Memo = TableMemo<M, S, typename MD::MemoEntry>;
    constexpr int EV = TW<M>::EV, K = TW<M>::CLASS, LV = kLevels<R, EV>;
    constexpr uint32_t kStackWords = LV * Stk::kBytes / 4;
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const uint32_t* list = pass2 ? a.heavy_list[K] : a.class_list[K];
    const uint32_t total = a.cnt[(pass2 ? TC_HEAVY : TC_CLASS) + K];
    if ((uint64_t)blockIdx.x * C_LANES >= total) return;

    uint16_t* ev = reinterpret_cast<uint16_t*>(lds);
    const Stk stk(lds + (EV / 2) * C_LANES, lane);
    Memo mm;
    if constexpr (MEMO) {
        mm.entry = reinterpret_cast<uint64_t*>(lds + (EV / 2 + kStackWords) * C_LANES) + lane;
        mm.tab = a.memo + ((uint64_t)blockIdx.x * C_LANES + (uint64_t)lane) * (uint64_t)a.memo_entries *
                              (uint64_t)MD::MemoEntry::kQuads;
        mm.mask = a.memo_entries - 1u;
        mm.tag = MD::MemoEntry::tag_of(a.memo_epoch);
        mm.hits = 0u;
    }
    MD md;
    if constexpr (MD::kLdsBlob) {
        uint32_t* tab = lds + search_lds_words<MD, R, M, MEMO>();
        const uint4* src = reinterpret_cast<const uint4*>(a.t.blob);
        uint4* dst = reinterpret_cast<uint4*>(tab);
        for (uint32_t k = lane; k < a.t.blob_words / 4u; k += C_LANES) dst[k] = src[k];
        __syncthreads();
        md.bind(a.t, tab);
    } else {
        md.bind(a.t, nullptr);
    }

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
        Lane dfs;
        dfs.depth = 0;
        dfs.nodes = 0;
        dfs.found = 0;
        // -2: no history in this lane
        int status = -2;
        if (active) {
            status = stage_events<M, MD>(a, H, ev, lane, dfs) ? -1 : QSMD_STATUS_ENCODE_ERROR;
            if (status == -1) dfs.init(a.state0);
        }
        if constexpr (MEMO) mm.begin(h);
        DeepPath<S> xp;
        if constexpr (EXPLAIN) xp.begin(H.ev_off, a.state0);
        // the search, the time limit checked every 1024 iterations (a
        // wavefront-uniform counter: the loop runs while any lane searches)
        while (__ballot(status == -1) != 0ull) {
            for (uint32_t k = 0; k < 1024u; ++k) {
                if (status == -1) {
                    if constexpr (R::kPending)
                        status = dfs.template pending_step<MD, MEMO>(md, ev, stk, lane, limit, mm);
                    else
                        status = dfs.template check_step<MD, MEMO, EXPLAIN>(md, ev, stk, lane, limit, mm, xp, a.path);
                }
                if (__ballot(status == -1) == 0ull) break;
            }
            if (status == -1 && a.s.time_limit && __builtin_amdgcn_s_memrealtime() - t0 > a.s.time_limit) {
                atomicOr(a.s.timed_out, 1u);
                status = QSMD_STATUS_BUDGET;
            }
        }
        if (status >= 0) status = dfs.template finish<R::kPending>(status);
        // over pass 1's budget (not the caller's): pass 2 searches it again
        const bool heavy = tiered && status == QSMD_STATUS_BUDGET && dfs.nodes >= limit;
        wave_append(heavy, h, a.heavy_list[K], a.cnt + TC_HEAVY + K, lane);
        const bool out = active && !heavy;
        if (out) {
            a.s.status[h] = (uint8_t)status;
            if (a.s.nodes) a.s.nodes[h] = dfs.nodes;
            if (a.s.witness && status == QSMD_STATUS_LINEARISABLE) {
                // the witness (and the pending rule's assumed bytes) from the
                // stack (depth <= n_ev: inside the slot)
                uint8_t* w = a.s.witness + H.ev_off;
                uint8_t* as = R::kPending && assumed ? assumed + H.ev_off : nullptr;
                for (uint32_t d = 0; d < dfs.depth; ++d) {
                    const uint32_t st = stk.get(d, lane);
                    w[d] = (uint8_t)(st & 0xFFu);
                    if (as) as[d] = (st & Lane::kAssumed) ? (uint8_t)((st >> 16) & 31u) : (uint8_t)QSMD_ASSUMED_NONE;
                }
                if (dfs.depth < H.n_ev) {
                    w[dfs.depth] = QSMD_WITNESS_END;
                    if (as) as[dfs.depth] = QSMD_ASSUMED_NONE;
                }
            }
        }
        if constexpr (EXPLAIN) {
            const auto at = [&](uint32_t d) { return stk.get(d, lane) & 0xFFu; };
            if (out) xp.finish(a.path, status, H.n_ev, dfs.depth, dfs.state, at, a.explain + h);
        }
        cnt.add(out, status, dfs.nodes);
        if constexpr (MEMO) {
            // the group's hits: one atomic per wavefront
            const uint64_t hits = wave_sum64(mm.hits);
            mm.hits = 0u;
            if (lane == 0 && hits)
                __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a.cnt + R::kHits), (unsigned long long)hits,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    cnt.flush(a.s.buckets, lane);
}

// The call's totals from the buckets, the probe for the host.
template <class Args>
__device__ __forceinline__ void finish_body(const Args& a) {
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

// ------------------------------------------------------------------- host
// the grid of a kernel with one lane per header
inline uint32_t bin_grid(uint64_t n_hist) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_hist + 63) / 64, 1), 4096);
}
template <class Args>
hipError_t launch_bin(void (*bin)(Args), const Args& p, hipStream_t s) {
    hipLaunchKernelGGL(bin, dim3(bin_grid(p.s.n_hist)), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}
template <class Args>
hipError_t launch_finish(void (*finish)(Args), const Args& p, hipStream_t s) {
    hipLaunchKernelGGL(finish, dim3(1), dim3(C_LANES), 0, s, p);
    return hipGetLastError();
}

// One search kernel with `lds` bytes of dynamic LDS, the kernel's limit raised
// when it must be (ensure_dyn_lds: one cache per KERNEL, that is per instantiation).
template <auto KERNEL, class... A>
hipError_t launch_search(size_t lds, uint32_t grid, hipStream_t s, A... args) {
    if (lds > 64u * 1024u) {
        static std::atomic<int> set[kAttrDevices];
        const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(KERNEL), set, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(C_LANES), lds, s, args...);
    return hipGetLastError();
}

// The launches of a call: bin, per pass (two when p.budget) the classes in
// `classes` (bit k set = launch class k) on grid1 / grid2 workgroups, then
// after_pass, then finish.  per_class(TW<M>{}, grid, pass2) launches class M.
template <class Args, class PerClass, class AfterPass>
hipError_t launch_passes(hipError_t (*bin)(const Args&, hipStream_t), hipError_t (*finish)(const Args&, hipStream_t),
                         const Args& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                         hipStream_t s, PerClass per_class, AfterPass after_pass) {
    hipError_t e = bin(p, s);
    for (uint32_t pass2 = 0; pass2 < (p.budget ? 2u : 1u) && e == hipSuccess; ++pass2) {
        const uint32_t* g = pass2 ? grid2 : grid1;
        if (e == hipSuccess && (classes & 1u)) e = per_class(TW<uint32_t>{}, g[0], pass2);
        if (e == hipSuccess && (classes & 2u)) e = per_class(TW<uint64_t>{}, g[1], pass2);
        if (e == hipSuccess && (classes & 4u)) e = per_class(TW<M128>{}, g[2], pass2);
        if (e == hipSuccess) e = after_pass(pass2);
    }
    if (e != hipSuccess) return e;
    return finish(p, s);
}
template <class Args, class PerClass>
hipError_t launch_passes(hipError_t (*bin)(const Args&, hipStream_t), hipError_t (*finish)(const Args&, hipStream_t),
                         const Args& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                         hipStream_t s, PerClass per_class) {
    return launch_passes(bin, finish, p, grid1, grid2, classes, s, per_class, [](uint32_t) { return hipSuccess; });
}

// A check call's launches.  KN: a file's kernels -- bin, finish and
// launch_class<M, MEMO, EXPLAIN>.  EXPLAIN: the explain call, always the plain
// search; else pass 2 runs the MEMO kernels when p.memo.
template <class KN, bool EXPLAIN, class Args>
hipError_t launch_check(const Args& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                        hipStream_t s) {
    return launch_passes(KN::bin, KN::finish, p, grid1, grid2, classes, s, [&](auto w, uint32_t grid, uint32_t pass2) {
        using M = typename decltype(w)::Mask;
        if constexpr (EXPLAIN) return KN::template launch_class<M, false, true>(p, grid, pass2, s);
        else if (pass2 && p.memo) return KN::template launch_class<M, true, false>(p, grid, pass2, s);
        else return KN::template launch_class<M, false, false>(p, grid, pass2, s);
    });
}

}  // namespace tsearch
}  // namespace qsmd
