// wtable.hip -- QSMD_MODEL_WTABLE: the reference search for a model too large
// for LDS (include/qsmd.h qsmd_wtable_model): up to 65,536 states, 256
// invocation and 256 response symbols.  The semantics are model 3's,
//     post  = bit r of post[s][i]            (word r >> 5, bit r & 31)
//     raise = bit r of post_err[s][i]
//     next  = on_resp[on_inv[s][i]][r]
// and the search is table_search.h's with the wide model below and the
// reference's rule (no pending call).  The model's policy:
//   * the tables are read from device memory (internal.h WTableDev: one
//     record per (state, invocation) holding on_inv and the postcondition
//     words).  Given (state, i, rc) the record's on_inv word, its post word
//     rc >> 5 and (only when the model has one) its post_err word are
//     independent loads issued together; on_resp is the one dependent load;
//   * a state has 16 bits, so the DFS stack is one 32-bit word per level
//     (event 8 | state before the step 16).  The events are the narrow
//     model's 16-bit elements;
//   * the memo's tag word is epoch 16 | state 16.
// LDS per workgroup: 4 / 8 / 16 KB of events and as much of stack (with the
// memo, 8 / 16 / 32 KB of node counts more); no table.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "table_search.h"

namespace qsmd {

namespace {

using namespace tsearch;

struct WideModel {
    using Args = WTableArgs;
    using State = uint32_t;
    using CheckStack = Stack32;
    using MemoEntry = MemoEntry32<16>;
    static constexpr uint32_t kModelId = QSMD_MODEL_WTABLE;
    static constexpr bool kLdsBlob = false;

    WTableDev t;
    const uint16_t* on_resp;

    __device__ __forceinline__ void bind(const WTableDev& dev, const uint32_t*) {
        t = dev;
        on_resp = reinterpret_cast<const uint16_t*>(dev.blob + dev.on_resp_off);
    }
    using Staged = NarrowModel::Staged;
    struct Look {
        uint32_t mid, rc, ok, err, save;
    };
    // the record of (state, i): three independent loads, post_err's only when
    // the model has one (a uniform condition)
    __device__ __forceinline__ Look look(State state, uint32_t ej, uint32_t er) const {
        const uint32_t i = ej >> 8, rc = er >> 8;
        const uint32_t* rec = t.blob + (state * t.n_inv + i) * t.rec_words;
        const uint32_t w = rc >> 5, b = rc & 31u;
        const uint32_t mid = rec[0];
        const uint32_t pw = rec[1u + w];
        const uint32_t ew = t.has_err ? rec[1u + t.post_words + w] : 0u;
        return {mid, rc, (pw >> b) & 1u, (ew >> b) & 1u, state};
    }
    __device__ __forceinline__ uint32_t next(const Look& k) const { return on_resp[k.mid * t.n_resp + k.rc]; }
    static __device__ __forceinline__ State moved(State, const Look&, uint32_t next) { return next; }
    static __device__ __forceinline__ State undone(State, uint32_t saved, const uint16_t*, uint32_t, int) {
        return saved;
    }
};

__global__ __launch_bounds__(C_LANES) void wtable_bin(WTableArgs a) { bin_body(a, WideModel::kModelId); }

template <class M, bool MEMO, bool EXPLAIN>
__global__ __launch_bounds__(C_LANES) void wtable_search(WTableArgs a, uint32_t pass2) {
    search_body<WideModel, CheckRule, M, MEMO, EXPLAIN>(a, pass2, nullptr);
}

__global__ __launch_bounds__(C_LANES) void wtable_finish(WTableArgs a) { finish_body(a); }

hipError_t launch_wtable_bin(const WTableArgs& p, hipStream_t s) { return launch_bin(wtable_bin, p, s); }
hipError_t launch_wtable_finish(const WTableArgs& p, hipStream_t s) { return launch_finish(wtable_finish, p, s); }

struct Kernels {
    static constexpr auto bin = launch_wtable_bin, finish = launch_wtable_finish;
    // (at most 64 KB, the 128-event class with the memo: no attribute to raise)
    template <class M, bool MEMO, bool EXPLAIN>
    static hipError_t launch_class(const WTableArgs& p, uint32_t grid, uint32_t pass2, hipStream_t s) {
        constexpr size_t lds = search_lds_words<WideModel, CheckRule, M, MEMO>() * 4;
        static_assert(lds <= 64u * 1024u, "dynamic LDS within the default limit");
        return launch_search<wtable_search<M, MEMO, EXPLAIN>>(lds, grid, s, p, pass2);
    }
};

}  // namespace

hipError_t launch_table(const WTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                        hipStream_t s) {
    return launch_check<Kernels, false>(p, grid1, grid2, classes, s);
}

// The explain call's launches (include/qsmd.h qsmd_explain_batch): launch_table
// with the EXPLAIN instantiations, always the plain search (p.memo null); the
// caller has run launch_explain_prepare on the stream.
hipError_t launch_table_explain(const WTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                                hipStream_t s) {
    return launch_check<Kernels, true>(p, grid1, grid2, classes, s);
}

}  // namespace qsmd
