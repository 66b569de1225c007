// ktgen.h -- the keyed-table-model generator kernel's launch interface
// (csrc/ktgen.hip; qsmd_gen_ktable_batch_device, include/qsmd_gen.h).
#pragma once

#include "internal.h"

namespace qsmd {

// Everything one launch needs, by value (the weights travel with the launch,
// as tgen.h's: no buffer of the context is written while an earlier launch
// may still read it).
struct KTGenArgs {
    TableDev t;                   // the context's keyed component (copied to LDS)
    uint32_t state0;              // the component's init_state
    uint32_t n_keys;              // 1..QSMD_KTABLE_MAX_KEYS
    uint32_t n_clients, n_ops;
    uint32_t prefix;              // min(prefix_ops, n_ops)
    uint32_t in_window;           // QSMD_GEN_LIN_IN_WINDOW
    uint32_t shared;              // QSMD_GEN_PID_SHARED
    uint32_t overlap;             // > 0
    uint32_t w_all;               // the sum of all pairs' weights
    uint32_t w_mask;              // bit i set <=> inv_weight[i] > 0
    uint32_t k_mask;              // bit k set <=> key_weight[k] > 0
    uint32_t w_unit;              // every inv and key weight is 0 or 1
    uint32_t bug_draw;            // p_bug > 0: unit() is drawn
    uint64_t bug_below;           // unit() < p_bug  <=>  (next() >> 11) < bug_below
    uint64_t seed, first, n_hist;
    uint32_t ev_base;
    qsmd_hdr* hdr;
    qsmd_event* events;
    uint8_t* bug;                 // may be null
    uint32_t inv_weight[QSMD_TABLE_MAX_INV];
    uint32_t key_weight[QSMD_KTABLE_MAX_KEYS];
};

// One workgroup per 64 histories (grid-stride past 65,536, or past 8 per CU
// when the component's blob is more than 4 KB).
hipError_t launch_ktgen(const KTGenArgs& a, uint32_t n_cu, hipStream_t s);

}  // namespace qsmd
