// tpending.hip -- qsmd_check_pending_batch: the search for QSMD_MODEL_TABLE
// with one change to the reference's rule: an invocation whose pid has no
// remaining response (a crashed client, a timeout) may take effect with any
// response the model allows.  A history with no response
// event at all whose root has no child is LINEARISABLE with 0 nodes (every
// operation dropped).
//
// The search is table_search.h's with the narrow model and the pending rule
// (TableLane::pending_step); the binning and the totals kernels are table.hip's
// (launch_table_bin, launch_table_finish); the explain record has no
// instantiation here.  One workgroup holds events [EV / 2][64] words | stack
// [EV][64] words | the tables: 48 KB + 80 KB at the 128-event class and the
// largest table.
//
// With the knob "pending_memo" pass 2 runs pending_search_memo: the exact-count
// state memo of the check call's pass 2 under the pending
// step.  The root rule of finish() concerns the root only, which is never
// recorded.  The column of node counts at entry has one 64-bit count per stack
// level, [EV][64] u64; a class whose columns and tables pass the device's LDS
// limit runs the plain kernel in pass 2 (the memo is exact: the same results).
#include <hip/hip_runtime.h>

#include "internal.h"
#include "table_search.h"

namespace qsmd {

namespace {

using namespace tsearch;

template <class M>
__global__ __launch_bounds__(C_LANES) void pending_search(TableArgs a, uint32_t pass2, uint8_t* assumed) {
    search_body<NarrowModel, PendingRule, M, false, false>(a, pass2, assumed);
}

// pass 2 with the state memo ("pending_memo")
template <class M>
__global__ __launch_bounds__(C_LANES) void pending_search_memo(TableArgs a, uint8_t* assumed) {
    search_body<NarrowModel, PendingRule, M, true, false>(a, 1u, assumed);
}

// The memo call's hits for the host (table_finish's probe holds the check
// call's, 0 here: the two knobs' counters are apart).
__global__ void pending_hits_probe(TableArgs a) {
    if (threadIdx.x == 0 && a.probe_host) {
        a.probe_host[kProbePendHits] = a.cnt[TC_PHITS];
        a.probe_host[kProbePendHits + 1] = a.cnt[TC_PHITS + 1];
        __threadfence_system();
    }
}

}  // namespace

hipError_t launch_table_pending(const TableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3],
                                uint32_t classes, uint8_t* assumed, size_t lds_limit, hipStream_t s) {
    return launch_passes(
        launch_table_bin, launch_table_finish, p, grid1, grid2, classes, s,
        [&](auto w, uint32_t grid, uint32_t pass2) {
            using M = typename decltype(w)::Mask;
            // pass 2 with the memo, unless the class's memo kernel does not fit lds_limit
            const size_t lds = table_lds_bytes(p.t, w.CLASS, true, true);
            if (pass2 && p.memo && lds <= lds_limit)
                return launch_search<pending_search_memo<M>>(lds, grid, s, p, assumed);
            return launch_search<pending_search<M>>(table_lds_bytes(p.t, w.CLASS, false, true), grid, s, p, pass2,
                                                    assumed);
        },
        [&](uint32_t pass2) {
            if (!(pass2 && p.memo)) return hipSuccess;
            hipLaunchKernelGGL(pending_hits_probe, dim3(1), dim3(C_LANES), 0, s, p);
            return hipGetLastError();
        });
}

}  // namespace qsmd
