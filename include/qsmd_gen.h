/*
 * qsmd_gen.h -- seeded synthetic history generator (C ABI).
 *
 * Produces batches in the include/qsmd.h layout.  It restates the delivery
 * policy of the reference's deterministic scheduler (src/Scheduler.hs:105-186:
 * one mailbox per (client, server) pair, requests and responses of a pair
 * strictly alternate, every tick delivers one event of a uniformly chosen
 * ready pair), the sequential prefix of prop_bank / prop_ticketDispenserParallel
 * (SchedulerSequential, test/Bank.hs:267-269, test/TicketDispenser.hs:294-297)
 * and the request distributions of test/Bank.hs:133-146 (Open:Deposit:
 * Withdraw:Transfer:CheckBalance = 1:5:5:8:5, money getPositive ~ U{1..100})
 * and test/TicketDispenser.hs:108-112 (Reset:TakeTicket = 1:8).
 *
 * Responses come from a sequentially executed implementation of the model
 * (the spec), applied at each operation's linearisation point; so histories
 * are linearisable unless a bug is injected (p_bug).  Each history's RNG is
 * derived from (seed, global history index) only, so any shard of a batch can
 * be generated independently and reproducibly on any rank.
 */
#ifndef QSMD_GEN_H
#define QSMD_GEN_H

#include "qsmd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Linearisation point of the implementation. */
#define QSMD_GEN_LIN_AT_INVOKE 0u  /* actor executes on delivery of the request
                                      (bankSM / clientSM, test/Bank.hs:217-242) */
#define QSMD_GEN_LIN_IN_WINDOW 1u  /* uniformly inside [invoke, response)       */

#define QSMD_GEN_PID_PER_CLIENT 0u /* Bank: pid = account (fromPid, Bank.hs:54)  */
#define QSMD_GEN_PID_SHARED     1u /* TicketDispenser: every event carries the
                                      test process's pid (Q1, TicketDispenser.hs:302-309) */

typedef struct qsmd_gen_params {
    uint32_t model_id;     /* QSMD_MODEL_BANK / QSMD_MODEL_TICKET                 */
    uint32_t n_clients;    /* C: Bank accounts / Ticket clients (<= 8)            */
    uint32_t n_ops;        /* K: total operations per history (<= 64)             */
    uint32_t prefix_ops;   /* sequential prefix (Bank: >= C, opens the accounts)  */
    uint32_t lin_policy;   /* QSMD_GEN_LIN_*                                       */
    uint32_t pid_mode;     /* QSMD_GEN_PID_*                                       */
    uint32_t overlap;      /* max operations outstanding at once (0 = C)          */
    uint32_t money_max;    /* Bank money ~ U{1..money_max} (0 = 100)              */
    double   p_bug;        /* probability of one injected response bug           */
    uint64_t seed;
} qsmd_gen_params;

/* Generate histories [first, first + n_hist) of the stream defined by p.
 * Every history has exactly 2*n_ops events; hdr[i].ev_off = (i * 2 * n_ops)
 * + ev_base.  events must hold n_hist * 2 * n_ops entries.  bug_out
 * (nullable) receives 1 for histories that carry an injected bug.
 * Returns 0, or QSMD_ERR_ARG. */
int qsmd_gen_batch(const qsmd_gen_params* p, uint64_t first, uint64_t n_hist,
                   uint32_t ev_base, qsmd_hdr* hdr, qsmd_event* events,
                   uint8_t* bug_out, int n_threads);

/* On-device generation (libqsmd.so, csrc/gen.hip): the same stream as
 * qsmd_gen_batch, byte-identical, written to device buffers (hdr_dev[n_hist],
 * events_dev[n_hist * 2 * n_ops], bug_dev nullable) and enqueued on `stream`
 * (NULL = the context's stream) of ctx's device.  Returns 0 or QSMD_ERR_*. */
int qsmd_gen_batch_device(qsmd_ctx* ctx, const qsmd_gen_params* p, uint64_t first, uint64_t n_hist,
                          uint32_t ev_base, qsmd_hdr* hdr_dev, qsmd_event* events_dev,
                          uint8_t* bug_dev, void* stream);

/* ---------------------------------------------------- table-model generator
 *
 * The same seeded, index-sharded generator for ANY table model
 * (QSMD_MODEL_TABLE / QSMD_MODEL_WTABLE, include/qsmd.h).  The implementation
 * answering requests is the table itself.  The definition below is complete:
 * the host function, the device kernel (csrc/tgen.hip) and the tests' Python
 * restatement (tests/tablegen_ref.py) emit identical bytes from it.
 *
 * RNG.  One generator per history: xoshiro256** whose four words are four
 * successive splitmix64 outputs from x = seed ^ (g * 0xD1B54A32D192ED03),
 * g = first + i the GLOBAL history index (all arithmetic mod 2^64).
 *   next()   one xoshiro256** output
 *   below(n) ((next() >> 32) * n) >> 32; n = 0 gives 0 WITHOUT a draw
 *   unit()   (next() >> 11) * 2^-53, a double
 * These are qsmd_gen_batch's.  "One draw" below is one next().
 *
 * Model.  s is a state index, starting at the table's init_state.
 *   acc(s, i) = post[s][i] & ~post_err[s][i], bits at or above n_resp cleared
 *               (no post_err: post[s][i]); over post_words words for model 4,
 *               response r being bit r & 31 of word r >> 5.
 *   weight(i) = inv_weight[i], or 1 for every i when inv_weight is NULL.
 *   request(s), one draw: i is enabled when weight(i) > 0 and acc(s, i) != 0.
 *     W = the sum of the enabled weights; if W == 0, every i with
 *     weight(i) > 0 is enabled instead and W is their sum.  w = below(W); the
 *     invocation is the first i, ascending, whose running sum of enabled
 *     weights exceeds w.
 *   execute(s, i), one draw: A = acc(s, i).  If A != 0, r is the
 *     below(popcount(A))-th set bit of A, ascending from bit 0 (so below(1) is
 *     still drawn).  Otherwise r = below(n_resp) and the history's flag byte
 *     gets bit 1, "stuck": the state moved between the request and its
 *     execution, and the model accepts no response there.  Then
 *     s = on_resp[on_inv[s][i]][r].
 *
 * Schedule.  K = n_ops, C = n_clients, P = min(prefix_ops, K), S = K - P,
 * overlap' = overlap ? overlap : C.  An invocation event of client c is
 * {kp = pid, code = i, 0, 0, 0}, its response {kp = 0x80 | pid, code = r, 0, 0,
 * 0}, pid = 0 with QSMD_GEN_PID_SHARED, else c.
 *   1. Prefix, P times: c = below(C); i = request(s); r = execute(s, i); emit
 *      the invocation, emit the response.
 *   2. S draws of below(C): queued[c] counts how often c was drawn.
 *   3. Suffix: every client is idle, invoked or executed (idle at first).
 *      Until S responses were emitted, a tick lists the ready actions, client
 *      0 first: "send" when c is idle, queued[c] > 0 and outstanding <
 *      overlap'; "execute" when c is invoked; "respond" when c is executed (a
 *      client has at most one).  n = below(number of ready actions) picks the
 *      n-th.
 *        send:    i = request(s); emit the invocation; queued[c]--,
 *                 outstanding++; with QSMD_GEN_LIN_AT_INVOKE r = execute(s, i)
 *                 at once and c is executed, else c is invoked.
 *        execute: r = execute(s, i) for c's pending i; c is executed.
 *        respond: emit c's response; c is idle, outstanding--.
 *   4. Bug.  If p_bug > 0: u = unit().  If u < p_bug and S >= 1 (the suffix
 *      responses are the S response events at positions >= 2 * P, numbered in
 *      event order from 0):
 *        coin = below(2), drawn only when n_resp >= 2 and S >= 2.
 *        If n_resp >= 2 and (S < 2 or coin == 0): k = below(S); d =
 *          below(n_resp - 1); response k's code becomes (code + 1 + d) %
 *          n_resp.  Flag bit 0.
 *        Else if S >= 2: k1 = below(S); k2 = below(S); if k2 == k1 then k2 =
 *          (k1 + 1) % S; responses k1 and k2 exchange codes (equal codes: the
 *          history is unchanged, the flag is still set).  Flag bit 0.
 *        Else (n_resp == 1 and S == 1) nothing changes and bit 0 stays clear.
 * Every history has 2 * K events, written to events[i * 2 * K ..) as
 * qsmd_gen_batch writes them (ev_base only moves ev_off: `events` may be a
 * slice that starts at entry ev_base of the checker's array); hdr[i] =
 * {ev_off = ev_base + i * 2 * K, n_ev = 2 * K, n_pid = 1 (shared pid) or C,
 * model_id, tag = (uint32_t)(first + i), reserved = 0}.  bug_out[i] (nullable)
 * is the flag byte: bit 0 an injected bug, bit 1 stuck; values 0..3.
 *
 * Promise.  With QSMD_GEN_PID_PER_CLIENT a history whose flag byte is 0 is
 * linearisable from init_state, its execute points being a witness.  (For a
 * model with post_err and QSMD_GEN_LIN_IN_WINDOW the reference's search, and
 * so the checker, may still report MODEL_ERROR for such a history: it raises
 * on a branch it tries before it reaches the witness.  With
 * QSMD_GEN_LIN_AT_INVOKE the invocation order is the witness and the search's
 * first path, so this cannot happen.)  With
 * QSMD_GEN_PID_SHARED there is NO such promise: the checker pairs an
 * invocation with the first remaining response of its pid (Q1), which on a
 * shared pid may be another client's, so a history generated without a bug
 * may be non-linearisable (this holds for qsmd_gen_batch's shared-pid
 * histories as well). */
typedef struct qsmd_gen_table_params {
    uint32_t model_id;     /* QSMD_MODEL_TABLE / QSMD_MODEL_WTABLE                */
    uint32_t n_clients;    /* C, 1..32                                            */
    uint32_t n_ops;        /* K, 1..64                                            */
    uint32_t prefix_ops;   /* sequential prefix, clamped to K                     */
    uint32_t lin_policy;   /* QSMD_GEN_LIN_*                                       */
    uint32_t pid_mode;     /* QSMD_GEN_PID_*                                       */
    uint32_t overlap;      /* max operations outstanding at once (0 = C)          */
    double   p_bug;       /* probability of one injected response bug, in [0, 1] */
    uint64_t seed;
    const uint32_t* inv_weight;  /* n_inv weights (host pointer); NULL = all 1    */
} qsmd_gen_table_params;

/* Generate histories [first, first + n_hist) of the stream above from `model`
 * (host pointers): a qsmd_table_model* when p->model_id is QSMD_MODEL_TABLE, a
 * qsmd_wtable_model* when QSMD_MODEL_WTABLE.  events holds n_hist * 2 * n_ops
 * entries.  QSMD_ERR_ARG, with no output written: everything qsmd_table_set /
 * qsmd_wtable_set reject in the model (QSMD_WTABLE_MAX_BYTES excepted: there
 * is no device copy), model_id not 3 or 4, C outside 1..32, K outside 1..64,
 * lin_policy or pid_mode above 1, p_bug NaN or outside [0, 1],
 * weights all zero or summing past 2^32 - 1, ev_base + n_hist * 2 * K past
 * 2^32 - 1. */
int qsmd_gen_table_batch(const qsmd_gen_table_params* p, const void* model,
                         uint64_t first, uint64_t n_hist, uint32_t ev_base,
                         qsmd_hdr* hdr, qsmd_event* events, uint8_t* bug_out,
                         int n_threads);

/* On-device generation (libqsmd.so, csrc/tgen.hip) of the same stream,
 * byte-identical, from the table the context holds (qsmd_table_set for model
 * 3, qsmd_wtable_set for 4; none set: QSMD_ERR_ARG).  Buffers and stream as
 * for qsmd_gen_batch_device; inv_weight is a host pointer, read before the
 * call returns.  The call is one of the context's ordered calls (include/
 * qsmd.h "Threading and streams"): it waits for the previous one, and a later
 * qsmd_table_set / qsmd_wtable_set waits for it before it frees the table. */
int qsmd_gen_table_batch_device(qsmd_ctx* ctx, const qsmd_gen_table_params* p,
                                uint64_t first, uint64_t n_hist,
                                uint32_t ev_base, qsmd_hdr* hdr_dev,
                                qsmd_event* events_dev, uint8_t* bug_dev,
                                void* stream);

/* ---------------------------------------------- keyed-table-model generator
 *
 * The same generator for QSMD_MODEL_KTABLE (include/qsmd.h): n_keys copies of
 * one narrow component table.  The stream is the table-model stream above on
 * the PRODUCT model, kept factored; the host function (csrc/gen/ktgen.cpp),
 * the device kernel (csrc/ktgen.hip) and the tests' restatement
 * (tests/ktablegen_ref.py) emit identical bytes from this definition.
 *
 * Unchanged from the table-model generator: the RNG with next(), below(n)
 * and unit(); the schedule, steps 1-4 (the prefix, the S client draws, the
 * ticks, the bug step with n_resp the component's); execute's "stuck" flag;
 * the header fields and ev_base; the flag byte.  What differs:
 *
 *   State.  s[0 .. n_keys) are component state indices, every key starting
 *     at the component's init_state.
 *   Invocation symbol.  A pair (k, i): key k < n_keys, i one of the
 *     component's n_inv invocation symbols.
 *   acc(s, (k, i)) = the component's acc(s[k], i) (post & ~post_err, bits at
 *     or above n_resp cleared).
 *   weight(k, i) = key_weight[k] * inv_weight[i], the product formed in 64
 *     bits; a NULL array counts as all 1.
 *   request(s), ONE draw over the pairs in ascending (k, i), key-major (k
 *     outer, i inner): a pair is enabled when weight(k, i) > 0 and
 *     acc(s, (k, i)) != 0.  W = the sum of the enabled weights; if W == 0,
 *     every pair with weight(k, i) > 0 is enabled instead and W is their sum.
 *     w = below(W); the invocation is the first pair, in that order, whose
 *     running sum of enabled weights exceeds w.
 *   execute(s, (k, i)), one draw, as for the component at s[k]: A =
 *     acc(s[k], i).  If A != 0, r is the below(popcount(A))-th set bit of A;
 *     otherwise r = below(n_resp) and the flag byte gets bit 1.  Then
 *     s[k] = on_resp[on_inv[s[k]][i]][r]; no other key changes.
 *   Events.  An invocation event is {kp = pid, code = i, a = k, b = 0, val =
 *     0}; a response event {kp = 0x80 | pid, code = r, 0, 0, 0}.
 *     hdr.model_id = QSMD_MODEL_KTABLE (5).
 *
 * So the keyed stream equals the QSMD_MODEL_WTABLE stream on the flat product
 * with invocation symbol k * n_inv + i and weight key_weight[k] *
 * inv_weight[i], code c re-encoded as (a = c / n_inv, code = c % n_inv).
 *
 * Promise.  As above, on the product: with QSMD_GEN_PID_PER_CLIENT a history
 * whose flag byte is 0 is linearisable from the initial vector (every key at
 * init_state), its execute points being a witness.  The same caveats hold:
 * for a component with post_err and QSMD_GEN_LIN_IN_WINDOW the reference's
 * search, and so the checker, may still report MODEL_ERROR for such a
 * history (it raises on a branch it tries before the witness; with
 * QSMD_GEN_LIN_AT_INVOKE it cannot); and with QSMD_GEN_PID_SHARED there is NO
 * promise, since the checker pairs an invocation with the first remaining
 * response of its pid (Q1), which may be another client's. */
typedef struct qsmd_gen_ktable_params {
    uint32_t n_keys;       /* 1..QSMD_KTABLE_MAX_KEYS                             */
    uint32_t n_clients;    /* C, 1..32                                            */
    uint32_t n_ops;        /* K, 1..64                                            */
    uint32_t prefix_ops;   /* sequential prefix, clamped to K                     */
    uint32_t lin_policy;   /* QSMD_GEN_LIN_*                                       */
    uint32_t pid_mode;     /* QSMD_GEN_PID_*                                       */
    uint32_t overlap;      /* max operations outstanding at once (0 = C)          */
    double   p_bug;        /* probability of one injected response bug, in [0, 1] */
    uint64_t seed;
    const uint32_t* inv_weight;  /* n_inv weights (host pointer); NULL = all 1    */
    const uint32_t* key_weight;  /* n_keys weights (host pointer); NULL = all 1   */
} qsmd_gen_ktable_params;

/* Generate histories [first, first + n_hist) of the keyed stream from
 * `component` (host pointers) on p->n_keys keys.  events holds n_hist * 2 *
 * n_ops entries.  QSMD_ERR_ARG, with no output written: everything
 * qsmd_ktable_set rejects in the component or in n_keys, C outside 1..32, K
 * outside 1..64, lin_policy or pid_mode above 1, p_bug NaN or outside [0, 1],
 * weights whose pairwise products are all zero or sum past 2^32 - 1,
 * ev_base + n_hist * 2 * K past 2^32 - 1. */
int qsmd_gen_ktable_batch(const qsmd_gen_ktable_params* p, const qsmd_table_model* component,
                          uint64_t first, uint64_t n_hist, uint32_t ev_base,
                          qsmd_hdr* hdr, qsmd_event* events, uint8_t* bug_out,
                          int n_threads);

/* On-device generation (libqsmd.so, csrc/ktgen.hip) of the same stream,
 * byte-identical, from the keyed table the context holds (qsmd_ktable_set;
 * none set, or p->n_keys different from the context's: QSMD_ERR_ARG).
 * Buffers and stream as for qsmd_gen_batch_device; the weights are host
 * pointers, read before the call returns.  The call is one of the context's
 * ordered calls: it waits for the previous one, and a later qsmd_ktable_set
 * waits for it before it frees the component. */
int qsmd_gen_ktable_batch_device(qsmd_ctx* ctx, const qsmd_gen_ktable_params* p,
                                 uint64_t first, uint64_t n_hist, uint32_t ev_base,
                                 qsmd_hdr* hdr_dev, qsmd_event* events_dev,
                                 uint8_t* bug_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QSMD_GEN_H */
