// ktable_host.h -- the host half of qsmd_ktable_set (api.hip): everything the
// keyed kernel will index is checked here, and the component's blob is built
// in the narrow table's format (internal.h TableDev); and the sizing of the
// keyed path's state memo ("ktable_memo").  No HIP runtime call, so it is
// also built and run on its own (tools/ktable_host_check.cpp,
// tools/ktable_memo_host_check.cpp).
#pragma once

#include <cstring>
#include <vector>

#include "internal.h"

namespace qsmd {

// null: `t` (but its device pointer) and `blob` describe the component; else
// the reason the arguments are refused (nothing is written then).
inline const char* ktable_build(const qsmd_table_model* m, uint32_t n_keys, TableDev& t,
                                std::vector<uint32_t>& blob) {
    if (n_keys == 0 || n_keys > QSMD_KTABLE_MAX_KEYS) return "qsmd_ktable_set: n_keys outside 1..8";
    if (!m || !m->on_inv || !m->on_resp || !m->post) return "qsmd_ktable_set: null table";
    if (m->n_states == 0 || m->n_states > QSMD_TABLE_MAX_STATES || m->n_inv == 0 || m->n_inv > QSMD_TABLE_MAX_INV ||
        m->n_resp == 0 || m->n_resp > QSMD_TABLE_MAX_RESP)
        return "qsmd_ktable_set: component dimensions outside 1..256 states, 1..32 symbols";
    if (m->init_state >= m->n_states) return "qsmd_ktable_set: init_state >= n_states";
    const uint32_t si = m->n_states * m->n_inv, sr = m->n_states * m->n_resp;
    for (uint32_t k = 0; k < si; ++k)
        if (m->on_inv[k] >= m->n_states) return "qsmd_ktable_set: on_inv entry >= n_states";
    for (uint32_t k = 0; k < sr; ++k)
        if (m->on_resp[k] >= m->n_states) return "qsmd_ktable_set: on_resp entry >= n_states";
    TableDev d{};
    d.n_states = m->n_states;
    d.n_inv = m->n_inv;
    d.n_resp = m->n_resp;
    d.has_err = m->post_err ? 1u : 0u;
    d.blob_words = table_words(d);
    // (bits at or above n_resp are never read: the kernel checks every code)
    blob.assign(d.blob_words, 0u);
    std::memcpy(blob.data(), m->post, (size_t)si * 4);
    if (m->post_err) std::memcpy(blob.data() + table_off_err(d), m->post_err, (size_t)si * 4);
    std::memcpy(blob.data() + table_off_inv(d), m->on_inv, si);
    std::memcpy(blob.data() + table_off_resp(d), m->on_resp, sr);
    t = d;
    return nullptr;
}

// the keyed model value from model0 (n_keys states, null: every key at
// `init`), key k's state in bits 8k .. 8k + 7; false: a state >= n_states
inline bool ktable_pack_state(const uint32_t* model0, uint32_t init, uint32_t n_keys, uint32_t n_states,
                              uint64_t& out) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < n_keys; ++k) {
        const uint32_t s = model0 ? model0[k] : init;
        if (s >= n_states) return false;
        v |= (uint64_t)s << (8u * k);
    }
    out = v;
    return true;
}

// Pass 2's state memo on the keyed path (knob "ktable_memo", table_search.h
// TableMemo with MemoEntry48): one direct-mapped table of `entries` entries per lane slot of
// pass 2's grid.  One entry size for every width class: 3 x uint4 (count 64 |
// epoch 32 | history 32, state 64 | rem words 0-1, rem words 2-3 | zero); the
// 32- and 64-event classes never touch the third.
constexpr uint32_t kKMemoEntryBytes = 48;
constexpr uint64_t kKMemoCapBytes = 1ull << 30;
constexpr uint64_t kKMemoMaxEntries = 1ull << 20;

// the knob's values: 0 (off) or a power of two in 2..2^20
inline bool ktable_memo_ok(uint64_t v) { return v == 0 || (v >= 2 && v <= kKMemoMaxEntries && (v & (v - 1)) == 0); }

struct KMemoPlan {
    uint32_t entry_bytes;
    uint64_t per_wg;              // bytes of one workgroup's 64 tables
    uint32_t grid;                // pass 2's workgroups with the memo
    uint64_t bytes;               // grid * per_wg: the allocation
};
// entries: an accepted non-zero knob value; grid2 >= 1: pass 2's grid without
// the memo; grid_cap: "table_memo_grid" (0 = none).  The tables are held to
// 1 GiB by a smaller grid, but one workgroup's are always allowed (3 GiB at
// 2^20 entries).  64 * 2^20 * 48 * 65536 < 2^64: no overflow.
inline KMemoPlan ktable_memo_plan(uint64_t entries, uint64_t grid2, uint64_t grid_cap) {
    KMemoPlan p{};
    p.entry_bytes = kKMemoEntryBytes;
    p.per_wg = 64ull * entries * kKMemoEntryBytes;
    uint64_t g = kKMemoCapBytes / p.per_wg;
    if (g < 1) g = 1;
    if (grid_cap && g > grid_cap) g = grid_cap;
    if (g > grid2) g = grid2;
    p.grid = (uint32_t)g;
    p.bytes = g * p.per_wg;
    return p;
}

}  // namespace qsmd
