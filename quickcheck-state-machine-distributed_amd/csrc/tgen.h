// tgen.h -- the table-model generator kernel's launch interface
// (csrc/tgen.hip; qsmd_gen_table_batch_device, include/qsmd_gen.h).
#pragma once

#include "internal.h"

namespace qsmd {

// Everything one launch needs, by value (1.2 KB of the 4 KB a kernel's
// arguments may take: the weights travel with the launch, so no buffer of
// the context is written while an earlier launch may still read it).
struct TGenArgs {
    TableDev t;                   // model 3: the context's narrow table (copied to LDS)
    WTableDev wt;                 // model 4: its wide table (read by record)
    uint32_t state0;              // the table's init_state
    uint32_t model_id;
    uint32_t n_clients, n_ops;
    uint32_t prefix;              // min(prefix_ops, n_ops)
    uint32_t in_window;           // QSMD_GEN_LIN_IN_WINDOW
    uint32_t shared;              // QSMD_GEN_PID_SHARED
    uint32_t overlap;             // > 0
    uint32_t w_all;               // the sum of all weights
    uint32_t w_mask;              // narrow table: bit i set <=> weight[i] > 0
    uint32_t w_unit;              // every weight is 0 or 1
    uint32_t bug_draw;            // p_bug > 0: unit() is drawn
    uint64_t bug_below;           // unit() < p_bug  <=>  (next() >> 11) < bug_below
    uint64_t seed, first, n_hist;
    uint32_t ev_base;
    qsmd_hdr* hdr;
    qsmd_event* events;
    uint8_t* bug;                 // may be null
    uint32_t weight[QSMD_WTABLE_MAX_INV];
};

// One workgroup per 64 histories (grid-stride past 65,536, or past 8 per CU
// when every workgroup copies a table of more than 4 KB to LDS).
hipError_t launch_tgen(const TGenArgs& a, uint32_t n_cu, hipStream_t s);

}  // namespace qsmd
