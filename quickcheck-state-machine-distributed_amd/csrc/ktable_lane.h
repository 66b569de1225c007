// ktable_lane.h -- what the two keyed searches share (csrc/ktable.hip,
// QSMD_MODEL_KTABLE's check call; csrc/kpending.hip, its pending call): the
// staged 16-bit event and the staging of a history's events.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.h"
#include "lane.h"
#include "mask.h"
#include "table_lane.h"

namespace qsmd {
namespace klane {

using namespace tlane;

// the staged event: its symbol, its key (invocations)
__device__ __forceinline__ uint32_t kev_code(uint32_t e) { return (e >> 8) & 31u; }
__device__ __forceinline__ uint32_t kev_key(uint32_t e) { return e >> 13; }

// tlane::stage_table for keyed events: the 16-bit LDS element is pid 7 |
// kind 1 | code 5 | key 3, and an invocation's key must be < n_keys.  DFS: the
// lane's search state (INV, RESP, P[7]).
template <class M, class DFS>
__device__ __forceinline__ bool stage_ktable(const KTableArgs& a, const qsmd_hdr& H, uint16_t* ev, int lane,
                                             DFS& dfs) {
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
                const bool resp = (lo & QSMD_EV_RESP) != 0u;
                const uint32_t code = (lo >> 8) & 0xFFu, key = resp ? 0u : (lo >> 16) & 0xFFu;
                if (in) ev[col16(e, lane)] = (uint16_t)((lo & 0xFFu) | ((code & 31u) << 8) | ((key & 7u) << 13));
                const uint32_t bit = in ? 1u << (c0 + k) : 0u;
#pragma unroll
                for (int b = 0; b < 8; ++b) pl[b][q] |= ((lo >> b) & 1u) ? bit : 0u;
                bad |= (in && (code >= (resp ? a.t.n_resp : a.t.n_inv) || key >= a.n_keys)) ? 1u : 0u;
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

}  // namespace klane
}  // namespace qsmd
