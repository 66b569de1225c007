// ktable.hip -- QSMD_MODEL_KTABLE: the reference search on the product of
// n_keys (1..8) copies of one narrow table model (include/qsmd.h
// qsmd_ktable_set).  The model value is a vector s[0..n_keys) of component
// states; an invocation carries its component symbol in `code` and its key in
// `a`, and a step from s with invocation (k, i) and response r is
//     post  = bit r of post[s[k]][i]
//     raise = bit r of post_err[s[k]][i]      (wins over post)
//     s[k] := on_resp[on_inv[s[k]][i]][r]     (every other key unchanged)
// -- src/Linearisability.hs:63-65 on the product model, whose flat table
// would have n_states^n_keys states.
//
// The search is table_search.h's with the keyed model (KeyedModel there:
// kpending.hip uses it too) and the reference's rule.  Pass 2's exact-count
// state memo (knob "ktable_memo") is the shared rule on
// (rem, the full 64-bit state) with 48-byte entries (MemoEntry48);
// "table_memo" has no effect here: with "ktable_memo" 0 pass 2 is the plain
// one.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "table_search.h"

namespace qsmd {

namespace {

using namespace tsearch;

__global__ __launch_bounds__(C_LANES) void ktable_bin(KTableArgs a) { bin_body(a, KeyedModel::kModelId); }

template <class M, bool MEMO, bool EXPLAIN>
__global__ __launch_bounds__(C_LANES) void ktable_search(KTableArgs a, uint32_t pass2) {
    search_body<KeyedModel, CheckRule, M, MEMO, EXPLAIN>(a, pass2, nullptr);
}

__global__ __launch_bounds__(C_LANES) void ktable_finish(KTableArgs a) { finish_body(a); }

struct Kernels {
    static constexpr auto bin = launch_ktable_bin, finish = launch_ktable_finish;
    template <class M, bool MEMO, bool EXPLAIN>
    static hipError_t launch_class(const KTableArgs& p, uint32_t grid, uint32_t pass2, hipStream_t s) {
        return launch_search<ktable_search<M, MEMO, EXPLAIN>>(table_lds_bytes(p.t, TW<M>::CLASS, MEMO), grid, s, p,
                                                              pass2);
    }
};

}  // namespace

// The first and the last launch of a keyed call on their own (csrc/kpending.hip).
hipError_t launch_ktable_bin(const KTableArgs& p, hipStream_t s) { return launch_bin(ktable_bin, p, s); }
hipError_t launch_ktable_finish(const KTableArgs& p, hipStream_t s) { return launch_finish(ktable_finish, p, s); }

hipError_t launch_table(const KTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                        hipStream_t s) {
    return launch_check<Kernels, false>(p, grid1, grid2, classes, s);
}

// The explain call's launches (include/qsmd.h qsmd_explain_batch): launch_table
// with the EXPLAIN instantiations, always the plain search (p.memo null); the
// caller has run launch_explain_prepare on the stream.
hipError_t launch_table_explain(const KTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                                hipStream_t s) {
    return launch_check<Kernels, true>(p, grid1, grid2, classes, s);
}

}  // namespace qsmd
