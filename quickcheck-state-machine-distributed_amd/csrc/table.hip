// table.hip -- QSMD_MODEL_TABLE: the reference search for a finite-state
// model given as tables at run time (include/qsmd.h qsmd_table_model).
//
// The reference's `linearisable` takes any transition / postcondition
// closures (src/Linearisability.hs:52-58); a C ABI cannot.  A model with at
// most 256 states and 32 invocation / response symbols is four tables, which
// every workgroup copies to LDS (dynamic size: the table actually set; 80 KB
// at 256 x 32 x 32 with post_err), so nothing of the hot loop is in global
// memory.  The search is table_search.h's with the narrow model (NarrowModel
// there: tpending.hip uses it too) and the reference's rule; with the knob
// "table_memo" pass 2 runs the MEMO instantiations (the counts, the verdict
// and the witness are unchanged).  This file also holds what the three table
// models share outside the search: table_lds_bytes and the explain call's
// first kernel.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "table_search.h"

namespace qsmd {

namespace {

using namespace tsearch;

__global__ __launch_bounds__(C_LANES) void table_bin(TableArgs a) { bin_body(a, NarrowModel::kModelId); }

template <class M, bool MEMO, bool EXPLAIN>
__global__ __launch_bounds__(C_LANES) void table_search(TableArgs a, uint32_t pass2) {
    search_body<NarrowModel, CheckRule, M, MEMO, EXPLAIN>(a, pass2, nullptr);
}

__global__ __launch_bounds__(C_LANES) void table_finish(TableArgs a) { finish_body(a); }

// The explain call's first launch, for the three table models (a.model_id):
// every history's qsmd_explain record as the binning kernel's verdicts need it
// -- zero, with the initial state for an empty history (depth 0); the search
// kernels overwrite the records of the histories they decide -- and, for an
// ENCODE_ERROR found in the header, the terminator in the first byte of a slot
// that has one inside the events array.
__global__ __launch_bounds__(C_LANES) void explain_prepare(SearchArgs a, uint64_t state0, uint8_t* path,
                                                           uint4* explain) {
    for (uint64_t h = (uint64_t)blockIdx.x * C_LANES + threadIdx.x; h < a.n_hist; h += (uint64_t)gridDim.x * C_LANES) {
        const qsmd_hdr H = a.hdr[h];
        const bool enc_ok = H.model_id == a.model_id && H.n_ev <= QSMD_MAX_EVENTS &&
                            (uint64_t)H.ev_off + H.n_ev <= a.n_events;
        const uint64_t st = enc_ok ? state0 : 0ull;     // (enc_ok and searched: overwritten)
        explain[h] = make_uint4(0u, 0u, (uint32_t)st, (uint32_t)(st >> 32));
        if (!enc_ok && H.n_ev > 0u && (uint64_t)H.ev_off < a.n_events) path[H.ev_off] = QSMD_WITNESS_END;
    }
}

struct Kernels {
    static constexpr auto bin = launch_table_bin, finish = launch_table_finish;
    template <class M, bool MEMO, bool EXPLAIN>
    static hipError_t launch_class(const TableArgs& p, uint32_t grid, uint32_t pass2, hipStream_t s) {
        static_assert(sizeof(qsmd_totals) == T_N * 8, "qsmd_totals is T_N x u64 in T_* order");
        return launch_search<table_search<M, MEMO, EXPLAIN>>(table_lds_bytes(p.t, TW<M>::CLASS, MEMO), grid, s, p,
                                                             pass2);
    }
};

}  // namespace

size_t table_lds_bytes(const TableDev& t, int k, bool memo, bool pending) {
    const size_t ev = k == 0 ? 32 : (k == 1 ? 64 : 128);
    // (pending: the pending rule's stack, one 32-bit level per event)
    // (and with the memo its column of counts, one u64 per event)
    const size_t stack = pending ? ev : ev / 4;
    const size_t entry = memo ? (pending ? 2 * ev : ev) : 0;
    return ((ev / 2 + stack + entry) * C_LANES + (size_t)t.blob_words) * 4;
}

// The first and the last launch of a table call on their own (csrc/tpending.hip).
hipError_t launch_table_bin(const TableArgs& p, hipStream_t s) { return launch_bin(table_bin, p, s); }
hipError_t launch_table_finish(const TableArgs& p, hipStream_t s) { return launch_finish(table_finish, p, s); }

hipError_t launch_explain_prepare(const SearchArgs& a, uint64_t state0, uint8_t* path, uint4* explain,
                                  hipStream_t s) {
    hipLaunchKernelGGL(explain_prepare, dim3(bin_grid(a.n_hist)), dim3(C_LANES), 0, s, a, state0, path, explain);
    return hipGetLastError();
}

hipError_t launch_table(const TableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                        hipStream_t s) {
    return launch_check<Kernels, false>(p, grid1, grid2, classes, s);
}

// The explain call's launches (include/qsmd.h qsmd_explain_batch): launch_table
// with the EXPLAIN instantiations, always the plain search (p.memo null); the
// caller has run launch_explain_prepare on the stream.
hipError_t launch_table_explain(const TableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3], uint32_t classes,
                                hipStream_t s) {
    return launch_check<Kernels, true>(p, grid1, grid2, classes, s);
}

}  // namespace qsmd
