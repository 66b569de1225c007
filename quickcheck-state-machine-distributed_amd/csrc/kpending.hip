// kpending.hip -- qsmd_check_kpending_batch: the search for QSMD_MODEL_KTABLE
// with the pending call's change to the reference's rule, on the product
// model: an invocation whose pid has no remaining response (a crashed client,
// a timeout) may take effect with any response the component allows at its
// key's state; its state has
// s[k] := on_resp[on_inv[s[k]][i]][r], every other key unchanged.
//
// The search is table_search.h's with the keyed model and the pending rule
// (TableLane::pending_step): the backtrack out of an assumed level restores the
// one byte of key k, k read from the chosen event (the highest removed
// response of the pid belongs to an earlier, completed operation, maybe on
// another key), and the allowed mask is cut to the bits below n_resp, so every
// on_resp index is in range.  One workgroup holds events [EV / 2][64] words |
// stack [EV][64] words | the component's tables: 48 KB + 80 KB at the
// 128-event class and the largest component.  The binning and the totals
// kernels are ktable.hip's (launch_ktable_bin, launch_ktable_finish).  No
// memo, no explain record and no local mode have an instantiation here.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "table_search.h"

namespace qsmd {

namespace {

using namespace tsearch;

template <class M>
__global__ __launch_bounds__(C_LANES) void kpending_search(KTableArgs a, uint32_t pass2, uint8_t* assumed) {
    search_body<KeyedModel, PendingRule, M, false, false>(a, pass2, assumed);
}

}  // namespace

hipError_t launch_ktable_pending(const KTableArgs& p, const uint32_t grid1[3], const uint32_t grid2[3],
                                 uint32_t classes, uint8_t* assumed, hipStream_t s) {
    return launch_passes(launch_ktable_bin, launch_ktable_finish, p, grid1, grid2, classes, s,
                         [&](auto w, uint32_t grid, uint32_t pass2) {
                             using M = typename decltype(w)::Mask;
                             return launch_search<kpending_search<M>>(table_lds_bytes(p.t, w.CLASS, false, true), grid,
                                                                      s, p, pass2, assumed);
                         });
}

}  // namespace qsmd
