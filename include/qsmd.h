/*
 * qsmd.h -- C ABI of the MI355X-native linearisability checker.
 *
 * Drop-in boundary for ONE function of advancedtelematic/
 * quickcheck-state-machine-distributed:
 *
 *   linearisable :: Eq pid
 *                => (model -> Either inv resp -> model)      -- transition
 *                -> (model -> inv -> resp -> Bool)           -- postcondition
 *                -> model -> History pid inv resp -> Bool
 *   (src/Linearisability.hs:52-69, exported at :1-7; History at :18)
 *
 * The reference has no FFI; its callers are test/Bank.hs:285,
 * test/TicketDispenser.hs:253 and :320, one call per history.  The binding a
 * Haskell maintainer adds (`foreign import ccall safe "qsmd_check_batch"`) is
 * shown in INTEGRATION.md.  Every entry point below is plain C: caller-owned
 * buffers, plain pointers and sizes, no C++ or torch types.
 *
 * Semantics are bit-exact with the reference search:
 *   - same verdict for every history;
 *   - `nodes` = number of `step` evaluations (src/Linearisability.hs:63) of the
 *     reference's lazy left-to-right short-circuit DFS (exhaustive mode);
 *   - model exceptions (Bank `Map.!`, test/Bank.hs:128) surface as
 *     QSMD_STATUS_MODEL_ERROR exactly when the reference would raise them.
 */
#ifndef QSMD_H
#define QSMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSMD_ABI_VERSION 3u

/* ---------------------------------------------------------------- layout */

/* One history = one header (16 B) + n_ev events (8 B each) stored
 * contiguously at events[ev_off .. ev_off + n_ev).  Replaces the boxed list
 * `[(pid, Either inv resp)]` of src/Linearisability.hs:18. */
typedef struct qsmd_hdr {
    uint32_t ev_off;    /* index of the first event in the events array      */
    uint16_t n_ev;      /* number of events (<= QSMD_MAX_EVENTS)             */
    uint8_t  n_pid;     /* number of distinct dense pids used (<= 128)       */
    uint8_t  model_id;  /* QSMD_MODEL_* (must equal the call's model_id)     */
    uint32_t tag;       /* caller's tag, ignored by the checker              */
    uint32_t reserved;  /* must be 0                                         */
} qsmd_hdr;

/* One event.  kp = (kind << 7) | pid with kind 0 = Left inv, 1 = Right resp
 * (src/Linearisability.hs:18); pid is the dense per-history pid (the
 * marshaller maps `Eq pid` values to 0..n_pid-1 in order of first use). */
typedef struct qsmd_event {
    uint8_t kp;
    uint8_t code;       /* constructor code, model specific (below)          */
    uint8_t a;          /* Bank: account (dense, < QSMD_BANK_MAX_ACCOUNTS)   */
    uint8_t b;          /* Bank Transfer: destination account                */
    int32_t val;        /* Bank money / Balance; Ticket Number               */
} qsmd_event;

#define QSMD_EV_RESP      0x80u
#define QSMD_EV_PID_MASK  0x7Fu

#define QSMD_MAX_EVENTS   128   /* 64 operations (SURVEY.md §8b encode limit) */
#define QSMD_MAX_PIDS     128

/* ---------------------------------------------------------------- models */

#define QSMD_MODEL_TICKET 1u    /* test/TicketDispenser.hs:51-102          */
#define QSMD_MODEL_BANK   2u    /* test/Bank.hs:41-131                     */

/* TicketDispenser Request / Response (test/TicketDispenser.hs:51-63) */
#define QSMD_TICKET_TAKE_TICKET 0u
#define QSMD_TICKET_RESET       1u
#define QSMD_TICKET_NUMBER      0u   /* Number Int  (val)                  */
#define QSMD_TICKET_OK          1u

/* BankRequestF / BankResponse (test/Bank.hs:44-73) */
#define QSMD_BANK_OPEN_ACCOUNT   0u  /* a                                  */
#define QSMD_BANK_DEPOSIT        1u  /* a, val = money                     */
#define QSMD_BANK_WITHDRAW       2u  /* a, val = money                     */
#define QSMD_BANK_CHECK_BALANCE  3u  /* a                                  */
#define QSMD_BANK_TRANSFER       4u  /* a = from, val = money, b = to      */

#define QSMD_BANK_ACCOUNT_CREATED        0u
#define QSMD_BANK_DEPOSIT_MADE           1u
#define QSMD_BANK_WITHDRAWAL_MADE        2u
#define QSMD_BANK_TRANSFER_MADE          3u
#define QSMD_BANK_ACCOUNT_ALREADY_EXISTS 4u
#define QSMD_BANK_ACCOUNT_DOESNT_EXIST   5u
#define QSMD_BANK_INSUFFICIENT_FUNDS     6u
#define QSMD_BANK_BALANCE                7u  /* Balance Money (val)         */

#define QSMD_BANK_MAX_ACCOUNTS 8

/* Initial models (the `model0` argument).  NULL = the reference's initModel:
 * Nothing (test/TicketDispenser.hs:73-74) / M.empty (test/Bank.hs:86-87). */
typedef struct qsmd_ticket_model {
    uint32_t is_just;   /* 0 = Nothing, 1 = Just n                          */
    uint32_t reserved;
    int64_t  n;         /* must lie in int32 range                          */
} qsmd_ticket_model;

typedef struct qsmd_bank_model {
    uint32_t exists;    /* bit a set <=> account a is a key of the Map      */
    uint32_t reserved;
    int64_t  balance[QSMD_BANK_MAX_ACCOUNTS];  /* int32 range; 0 if absent  */
} qsmd_bank_model;

/* Table-driven model: ANY finite-state model, given as tables at run time
 * (no recompile).  The reference's `linearisable` takes arbitrary
 * transition / postcondition closures (src/Linearisability.hs:52-58); a C ABI
 * cannot, but a model with at most QSMD_TABLE_MAX_STATES states whose
 * invocations and responses are at most 32 symbols each is four tables.  A
 * step from state s with invocation symbol i and response symbol r is, as
 * src/Linearisability.hs:63-65:
 *     postcondition = bit r of post[s][i]
 *     next state    = on_resp[on_inv[s][i]][r]
 * An event's symbol is its `code` byte; a, b and val are ignored.  Limits:
 * 256 states, 32 invocation symbols, 32 response symbols, and as for every
 * model 128 events and 128 pids per history (pids may share events freely).
 *
 * qsmd_check_batch / qsmd_check_batch_device with QSMD_MODEL_TABLE:
 *   - model0: NULL = init_state, else a pointer to a uint32_t state, which
 *     must be < n_states (QSMD_ERR_ARG otherwise); no table set: QSMD_ERR_ARG;
 *   - QSMD_FLAG_EXHAUSTIVE, QSMD_FLAG_WITNESS and max_nodes as for the other
 *     models; QSMD_FLAG_MEMO is accepted and changes nothing (counts stay
 *     exact); QSMD_FLAG_EARLY_EXIT_BATCH, qsmd_split_frontier and
 *     qsmd_check_tasks return QSMD_ERR_UNSUPPORTED;
 *   - per history QSMD_STATUS_ENCODE_ERROR, with no search: hdr.model_id !=
 *     3, an invocation code >= n_inv, a response code >= n_resp, n_ev > 128,
 *     ev_off + n_ev > n_events;
 *   - totals and the time limit (qsmd_set_time_limit_ms, qsmd_timed_out) as
 *     for the other models.
 * Knob "table_budget" (default 256; qsmd_get_param reads it): histories are
 * searched in two passes per width class (<= 32, <= 64, <= 128 events), the
 * first with this node budget; a search over it runs again from the root in
 * the second, 64 to a wavefront, so a few long searches do not each hold 63
 * idle lanes.  0 = a single pass.  Results are unchanged.  qsmd_get_param
 * "table_pass2_last": histories the second pass took in the most recent
 * table call (waits for it).
 * Knob "table_memo" (default 0 = off: exactly the launches above; else a
 * power of two in 2..2^20, anything else QSMD_ERR_ARG): the second pass keeps
 * an exact-count state memo of that many entries per lane slot.  The subtree
 * below a node depends only on (remaining events, state); a subtree the
 * search backtracks out of is recorded under that full key with the nodes it
 * counted, and a later descent into the same key counts them at once and
 * backtracks.  Status, node count and witness stay the reference's; when
 * max_nodes (or 2^64 - 1 with max_nodes 0) falls inside a recorded subtree
 * the result is QSMD_STATUS_BUDGET with nodes == that limit.  A tree of 1e18
 * nodes with a few hundred distinct states is decided in a few thousand
 * iterations.  Limits: the memo serves the second pass only, so with
 * "table_budget" 0 there is none; it is opt-in; the tables (pass 2's
 * workgroups x 64 x entries x 32 bytes, device memory, allocated on first
 * use, kept until qsmd_close; QSMD_ERR_NOMEM when that fails) are held to
 * 1 GiB by launching fewer workgroups -- one workgroup's tables are always
 * allowed, 2 GiB at 2^20 entries.  Diagnostic knob "table_memo_grid": 0 =
 * automatic, else pass 2's workgroups at most while the memo is on.
 * qsmd_get_param "table_memo_hits_last": the memo's hits in the most recent
 * table call (waits for it).  The cascade's knobs, qsmd_probe_read and the
 * timing ring (qsmd_last_kernel_ms, qsmd_timing_read) do not apply to table
 * calls. */
/* Bits of post / post_err at or above n_resp are ignored by every entry, the
 * pending ones (qsmd_check_pending_batch, qsmd_check_kpending_batch) included. */
#define QSMD_MODEL_TABLE 3u
#define QSMD_TABLE_MAX_STATES 256
#define QSMD_TABLE_MAX_INV     32
#define QSMD_TABLE_MAX_RESP    32
typedef struct qsmd_table_model {
    uint32_t n_states, n_inv, n_resp, init_state;
    const uint8_t*  on_inv;    /* [n_states][n_inv]  transition m (Left inv)   */
    const uint8_t*  on_resp;   /* [n_states][n_resp] transition m (Right resp) */
    const uint32_t* post;      /* [n_states][n_inv]  bit r: postcondition m inv r */
    const uint32_t* post_err;  /* same shape, may be NULL; bit r: the postcondition
                                  raises -> QSMD_STATUS_MODEL_ERROR (wins over post) */
} qsmd_table_model;

/* Wide table-driven model: QSMD_MODEL_TABLE's semantics and call surface for
 * a model beyond its limits -- up to 65,536 states (16 bits) and 256
 * invocation / 256 response symbols (the event's `code` byte).  The tables
 * stay in device memory instead of LDS, so a step pays two dependent
 * device-memory reads where model 3 pays LDS reads: a model that fits model 3
 * should use model 3 (DESIGN.md §10c has the measured ratio).
 *   - on_inv [n_states][n_inv] and on_resp [n_states][n_resp] are uint16_t;
 *   - post and the optional post_err are [n_states][n_inv][post_words] with
 *     post_words = ceil(n_resp / 32); response r is bit r & 31 of word r >> 5;
 *   - a step is model 3's: post, post_err wins, next state
 *     on_resp[on_inv[s][i]][r].
 * QSMD_WTABLE_MAX_BYTES caps the context's device copy (n_states * n_inv *
 * (1 + post_words * (post_err ? 2 : 1)) * 4 bytes for on_inv and the
 * postcondition words, plus n_states * n_resp * 2 for on_resp, rounded up to
 * 16).  64 MiB is a design decision, not a measurement: a quarter of the
 * 256 MiB Infinity Cache, so the tables and the state memo stay cached
 * together.
 * qsmd_check_batch / qsmd_check_batch_device with QSMD_MODEL_WTABLE behave as
 * documented for QSMD_MODEL_TABLE above, with hdr.model_id 4, the wide
 * table's n_states / n_inv / n_resp, and qsmd_wtable_set in place of
 * qsmd_table_set.  The knobs "table_budget", "table_memo", "table_memo_grid"
 * and the read-outs "table_pass2_last", "table_memo_hits_last" apply
 * unchanged.  A context holds one narrow and one wide table, independently.
 * Bits of the last post / post_err word at or above n_resp are ignored. */
#define QSMD_MODEL_WTABLE 4u
#define QSMD_WTABLE_MAX_STATES 65536
#define QSMD_WTABLE_MAX_INV      256
#define QSMD_WTABLE_MAX_RESP     256
#define QSMD_WTABLE_MAX_BYTES (64u << 20)
typedef struct qsmd_wtable_model {
    uint32_t n_states, n_inv, n_resp, init_state;
    const uint16_t* on_inv;    /* [n_states][n_inv]  transition m (Left inv)   */
    const uint16_t* on_resp;   /* [n_states][n_resp] transition m (Right resp) */
    const uint32_t* post;      /* [n_states][n_inv][post_words]                */
    const uint32_t* post_err;  /* same shape, may be NULL (wins over post)     */
} qsmd_wtable_model;

/* Keyed table model: a map of small states (the shape of the reference's own
 * Bank model, key -> value) without tabulating the product.  The model is one
 * *component* table -- a qsmd_table_model within model 3's limits: 256
 * states, 32 invocation / response symbols -- and n_keys in
 * 1..QSMD_KTABLE_MAX_KEYS.  The model value is a vector s[0..n_keys) of
 * component states.  An invocation event carries its component symbol in
 * `code` and its key in `a`; a response carries its symbol in `code` and its
 * `a` is ignored; b and val are ignored everywhere.  A step from s with an
 * invocation (k, i) and a response r is src/Linearisability.hs:63-65 on the
 * product model:
 *     postcondition = bit r of post[s[k]][i]
 *     post_err bit r of [s[k]][i] raises QSMD_STATUS_MODEL_ERROR (wins)
 *     next state    = s with s[k] := on_resp[on_inv[s[k]][i]][r]
 * Flat, the same model has n_states^n_keys states (a 4-value register on 8
 * keys: 65,536 states x 168 invocation symbols, the whole of model 4); keyed,
 * it is the 4-state table in LDS and 8 bytes of state, searched at model 3's
 * speed with model 3's search: same verdicts, node counts and witnesses as
 * the reference on the product model.
 *
 * qsmd_check_batch / qsmd_check_batch_device with QSMD_MODEL_KTABLE behave as
 * documented for QSMD_MODEL_TABLE above, with these differences:
 *   - model0: NULL = every key at init_state, else a pointer to n_keys
 *     uint32_t states, each < n_states (QSMD_ERR_ARG otherwise); no keyed
 *     table set (qsmd_ktable_set): QSMD_ERR_ARG;
 *   - per history QSMD_STATUS_ENCODE_ERROR also for hdr.model_id != 5 and for
 *     an invocation whose key (`a`) is >= n_keys;
 *   - the second pass's exact-count state memo has its own knob here,
 *     "ktable_memo" (default 0 = off: the plain second pass; else a power of
 *     two in 2..2^20 entries per lane slot, anything else QSMD_ERR_ARG and
 *     the old value stays).  The rule is "table_memo"'s on (remaining events,
 *     the full 64-bit state): status, node count and witness are unchanged,
 *     a max_nodes inside a folded subtree gives BUDGET with nodes ==
 *     max_nodes.  An entry is 48 bytes; the tables share "table_memo"'s
 *     allocation (first use, QSMD_ERR_NOMEM, the 1 GiB cap -- one workgroup's
 *     tables always allowed, 3 GiB at 2^20 entries -- and "table_memo_grid").
 *     "table_memo_hits_last" reads its hits after a model-5 call.
 *     "table_memo" has no effect on model 5, "ktable_memo" none on models 3
 *     and 4.
 * "table_budget" and "table_pass2_last" apply unchanged.  A context holds one
 * narrow, one wide and one keyed table, independently.
 *
 * Local mode -- knob "ktable_local" (qsmd_set_param / qsmd_get_param; default
 * 0 = off: exactly the launches and results above; 1 = on; any other value
 * QSMD_ERR_ARG and the old value stays).  Linearisability is local (Herlihy &
 * Wing, Theorem 1): a complete, well-formed history over independent objects
 * is linearisable exactly when each object's sub-history is.  With the knob at
 * 1 a QSMD_MODEL_KTABLE call of qsmd_check_batch / qsmd_check_batch_device
 * checks every *splittable* history key by key instead of on the product.  A
 * call that carries QSMD_FLAG_WITNESS takes the product route whole, as if the
 * knob were 0 (so does a call with more than (2^32-1) / n_keys histories);
 * the knob has no effect on any other model.
 *   - A history is splittable when (1) it is encode-valid by the rules above
 *     (hdr.model_id == 5, n_ev <= 128, ev_off + n_ev <= n_events, every
 *     invocation code < n_inv and a < n_keys, every response code < n_resp)
 *     and (2) for every pid that occurs, the pid's events in history order
 *     alternate invocation, response, invocation, response, ..., from an
 *     invocation to a response: no pending invocation, no lone response, no
 *     two invocations of one pid in flight.  An operation is then an
 *     invocation and the next event of its pid, and a response belongs to its
 *     invocation's key.
 *   - Every other history is searched on the product, unchanged: its status
 *     and nodes (an ENCODE_ERROR included) are those of the knob at 0.
 *   - Sub-history k of a splittable history, for each key k in ascending
 *     order: the events of the operations whose invocation has a == k, in
 *     history order, bytes unchanged, the same header but for ev_off and n_ev,
 *     the same model0 vector.  A key with no operation has none.  Each is
 *     searched by the model-5 search above with the call's flags, max_nodes
 *     (applied to each sub-search on its own), time limit, "table_budget" and
 *     "ktable_memo".  Every sub-history is searched: no short cut across keys.
 *   - The history's status is that of the lowest key whose sub-search is not
 *     LINEARISABLE, or LINEARISABLE when there is none; its nodes is the sum
 *     over its sub-searches; n_ev == 0 gives LINEARISABLE with 0 nodes.
 *     qsmd_totals counts histories (nodes: the sum of the per-history values);
 *     qsmd_timed_out, "table_pass2_last" and "table_memo_hits_last" describe
 *     the launch over the sub-histories.
 *   - "ktable_local_last" (qsmd_get_param; waits for the call): the histories
 *     that were split in the most recent QSMD_MODEL_KTABLE call, 0 when it
 *     took the product route.
 *   - The call stays asynchronous on the caller's stream.  The sub-histories
 *     are laid out in a copy of the events array, each history's inside its
 *     own slot [ev_off, ev_off + n_ev): with the knob at 1 the slots of
 *     different headers must not overlap.
 * Promised: for a component without post_err, a splittable history's verdict
 * (LINEARISABLE / NONLINEARISABLE) is the reference's on the product model
 * whenever neither side ends in BUDGET.  With post_err, LINEARISABLE still
 * means that every key's sub-history is linearisable, and the rule above
 * holds.  Not promised: the node counts are not the reference's on the
 * product -- they are the reference's on each key, summed; BUDGET is per key
 * (a history the product search leaves BUDGET is usually decided); and with
 * post_err a failing history may read NONLINEARISABLE where the product search
 * reads MODEL_ERROR, or the reverse (when the reference raises depends on the
 * order of its branches). */
#define QSMD_MODEL_KTABLE 5u
#define QSMD_KTABLE_MAX_KEYS 8

/* -------------------------------------------------------------- results */

#define QSMD_STATUS_NONLINEARISABLE 0u  /* linearisable ... == False        */
#define QSMD_STATUS_LINEARISABLE    1u  /* == True                          */
#define QSMD_STATUS_MODEL_ERROR     2u  /* reference raises (Map.!)         */
#define QSMD_STATUS_ENCODE_ERROR    3u  /* unknown code, pid/account range, */
                                        /* > QSMD_MAX_EVENTS, bad model_id  */
#define QSMD_STATUS_BUDGET          4u  /* max_nodes reached, undecided     */
#define QSMD_STATUS_SKIPPED         5u  /* QSMD_FLAG_EARLY_EXIT_BATCH       */

#define QSMD_FLAG_EXHAUSTIVE       1u  /* reference search, exact counts    */
#define QSMD_FLAG_MEMO             2u  /* prune known-failing states        */
#define QSMD_FLAG_WITNESS          4u  /* fill witness_out                  */
#define QSMD_FLAG_EARLY_EXIT_BATCH 8u  /* stop at first non-linearisable    */

/* Witness: for a LINEARISABLE history i, witness_out[hdr[i].ev_off + d] is
 * the (history-local) index of the invocation event chosen at depth d of the
 * successful path; the list ends at the first 0xFF (or at n_ev).  Replay:
 * at each step the operation is (pid p of that event, its inv, the first
 * remaining response of p) -- SURVEY.md §8a Lemma L1.  witness_out has as
 * many bytes as the events array. */
#define QSMD_WITNESS_END 0xFFu

typedef struct qsmd_totals {
    uint64_t checked;           /* histories with a decided status         */
    uint64_t linearisable;
    uint64_t nonlinearisable;
    uint64_t model_errors;
    uint64_t encode_errors;
    uint64_t budget;
    uint64_t skipped;
    uint64_t nodes;             /* sum of per-history node counts          */
} qsmd_totals;

/* -------------------------------------------------------------- context */

typedef struct qsmd_ctx qsmd_ctx;

/* Return codes: 0 = ok, < 0 = API / device error (qsmd_last_error). */
#define QSMD_OK              0
#define QSMD_ERR_ARG        -1
#define QSMD_ERR_DEVICE     -2
#define QSMD_ERR_NOMEM      -3
#define QSMD_ERR_UNSUPPORTED -4

/* Bind a context to one HIP device (one process per GPU).  SURVEY.md §8b
 * proposed a device mask; a context serves exactly one device instead, and a
 * process drives several GPUs with one context per device. */
int  qsmd_open(qsmd_ctx** out, int device);
void qsmd_close(qsmd_ctx* ctx);
const char* qsmd_last_error(const qsmd_ctx* ctx);
uint32_t qsmd_abi_version(void);

/* Set the context's table model (one per context; a second call replaces
 * it).  Host pointers; the tables are copied, the context owns the device
 * copy and frees it in qsmd_close.  Everything the kernel will index is
 * checked: dimensions non-zero and within the maxima, every on_inv / on_resp
 * entry and init_state < n_states, on_inv / on_resp / post non-NULL --
 * otherwise QSMD_ERR_ARG, and the context keeps its previous table.  Waits
 * for the context's last call. */
int qsmd_table_set(qsmd_ctx* ctx, const qsmd_table_model* model);

/* Set the context's wide table model (QSMD_MODEL_WTABLE; one per context,
 * beside the narrow one).  The rules of qsmd_table_set: dimensions, every
 * on_inv / on_resp entry, init_state, the non-NULL tables and
 * QSMD_WTABLE_MAX_BYTES are checked -- otherwise QSMD_ERR_ARG, and the
 * context keeps its previous wide table.  Waits for the context's last call;
 * the device copy is freed in qsmd_close. */
int qsmd_wtable_set(qsmd_ctx* ctx, const qsmd_wtable_model* model);

/* Set the context's keyed table model (QSMD_MODEL_KTABLE; one per context,
 * beside the narrow and the wide one): `component` on n_keys keys.  The rules
 * of qsmd_table_set for the component (dimensions, every on_inv / on_resp
 * entry, init_state, the non-NULL tables), and n_keys in
 * 1..QSMD_KTABLE_MAX_KEYS -- otherwise QSMD_ERR_ARG, and the context keeps
 * its previous keyed table.  Waits for the context's last call; the device
 * copy is freed in qsmd_close. */
int qsmd_ktable_set(qsmd_ctx* ctx, const qsmd_table_model* component, uint32_t n_keys);

/* Threading and streams.  Every entry point of one context serialises on the
 * context's mutex, and the check calls of one context are ordered: a call on
 * a stream other than the previous call's first waits (on the device) for
 * that call, because they share the context's device workspace.  Calls that
 * should overlap use one context each (bench.py keeps calls in flight that
 * way).  Contexts share no device state.  A device call on a caller's stream
 * records a completion event on it, and the context's later waits (its next
 * call on another stream, qsmd_close, qsmd_probe_read, qsmd_timed_out, a knob
 * that reallocates) wait for that event, never for the caller's stream or the
 * whole device: the caller may destroy its stream once its own work on it is
 * done. */

/* Check a batch held in HOST memory (the drop-in for one call per history;
 * n_hist = 1 is valid).  Buffers are copied in and out; the library keeps no
 * pointer after return.  max_nodes = 0 means unbounded.  nodes_out,
 * witness_out, totals_out and model0 may be NULL.  Synchronous. */
int qsmd_check_batch(qsmd_ctx* ctx, uint32_t model_id,
                     const qsmd_hdr* hdr, uint64_t n_hist,
                     const qsmd_event* events, uint64_t n_events,
                     const void* model0, uint32_t flags, uint64_t max_nodes,
                     uint8_t* status_out, uint64_t* nodes_out,
                     uint8_t* witness_out, qsmd_totals* totals_out);

/* Same, with every buffer already resident in device memory (HBM) and work
 * enqueued on `stream` (a hipStream_t, NULL = the context's stream, a
 * blocking stream: ordered after the caller's work on the legacy default
 * stream, as HIP orders blocking streams): two to five kernel launches, no
 * host round trip.  totals_dev (device, may be NULL)
 * receives the qsmd_totals of the batch.  Asynchronous: synchronise the
 * stream before reading outputs. */
int qsmd_check_batch_device(qsmd_ctx* ctx, uint32_t model_id,
                            const qsmd_hdr* hdr_dev, uint64_t n_hist,
                            const qsmd_event* events_dev, uint64_t n_events,
                            const void* model0_host, uint32_t flags,
                            uint64_t max_nodes,
                            uint8_t* status_dev, uint64_t* nodes_dev,
                            uint8_t* witness_dev, qsmd_totals* totals_dev,
                            void* stream);

/* ----------------------------------------------------------------- explain
 * Where a history went wrong: the deepest linearised path of its search, for
 * the table models (QSMD_MODEL_TABLE, QSMD_MODEL_WTABLE, QSMD_MODEL_KTABLE).
 *
 * qsmd_explain_batch runs the search of qsmd_check_batch -- the same flags
 * (QSMD_FLAG_EXHAUSTIVE), max_nodes, time limit and "table_budget" passes --
 * and reports status and nodes exactly as qsmd_check_batch without a memo
 * does.  A *node at depth d* is a step whose postcondition held, so that the
 * search recurses; d counts the operations on the stack, that node included.
 * Per history one path is reported in the witness layout: path_out[ev_off + k]
 * is the history-local index of the invocation event chosen at depth k, and
 * the list ends at QSMD_WITNESS_END when it is shorter than n_ev.
 *
 *   LINEARISABLE     the witness; the state at its end
 *   NONLINEARISABLE, the path to the first node of maximal depth in DFS order
 *   BUDGET           among the nodes counted before the search ended (by
 *                    exhaustion, max_nodes or the time limit); the state after
 *                    that node's operation.  Depth 0: no first operation
 *                    passed (the state is the initial one)
 *   MODEL_ERROR      the search's current path when the postcondition raised,
 *                    i.e. the path to the parent of the raising step; the
 *                    state at its end
 *   ENCODE_ERROR     the path bytes as the caller gave them, except that a
 *                    slot with n_ev >= 1 and ev_off < n_events has its first
 *                    byte set to QSMD_WITNESS_END; the record all zero
 *
 * n_ev == 0 is LINEARISABLE with depth 0 at the initial state (no byte
 * written).
 *
 * Limits.  The explanation is always the plain search, for model 5 on the
 * product: the knobs "table_memo", "ktable_memo" and "ktable_local" are
 * ignored by these two calls (a folded subtree has no path to report), so a
 * history whose plain search passes max_nodes reads BUDGET, with the deepest
 * path seen so far, even where the memo would have let a check call decide it.
 * "table_budget" applies; pass 2 starts again from the root, and so does the
 * record.  qsmd_timed_out and "table_pass2_last" describe the call as they do
 * for a check.  The cascade models (1, 2) return QSMD_ERR_UNSUPPORTED, and so
 * does QSMD_FLAG_EARLY_EXIT_BATCH; QSMD_FLAG_WITNESS and QSMD_FLAG_MEMO are
 * accepted and change nothing.  The model0 rules, "no table set" and the
 * n_hist limits are those of the check call.  nodes_out and totals_out may be
 * NULL; path_out (n_events bytes) and explain_out (n_hist records) may not. */
typedef struct qsmd_explain {
    uint16_t depth;      /* operations on the reported path                          */
    uint16_t reserved;   /* 0                                                        */
    uint32_t reserved2;  /* 0                                                        */
    uint64_t state;      /* model state at its end: models 3 / 4 the state index;    */
                         /* model 5 key k's component state in bits 8k .. 8k + 7     */
} qsmd_explain;          /* 16 bytes */

/* Host memory, synchronous (as qsmd_check_batch). */
int qsmd_explain_batch(qsmd_ctx* ctx, uint32_t model_id,
                       const qsmd_hdr* hdr, uint64_t n_hist,
                       const qsmd_event* events, uint64_t n_events,
                       const void* model0, uint32_t flags, uint64_t max_nodes,
                       uint8_t* status_out, uint64_t* nodes_out,
                       uint8_t* path_out, qsmd_explain* explain_out,
                       qsmd_totals* totals_out);

/* Device memory, asynchronous on `stream` (as qsmd_check_batch_device). */
int qsmd_explain_batch_device(qsmd_ctx* ctx, uint32_t model_id,
                              const qsmd_hdr* hdr_dev, uint64_t n_hist,
                              const qsmd_event* events_dev, uint64_t n_events,
                              const void* model0_host, uint32_t flags,
                              uint64_t max_nodes,
                              uint8_t* status_dev, uint64_t* nodes_dev,
                              uint8_t* path_dev, qsmd_explain* explain_dev,
                              qsmd_totals* totals_dev, void* stream);

/* ----------------------------------------------------------------- pending
 * Let pending invocations take effect (QSMD_MODEL_TABLE only; opt-in).
 *
 * The check calls follow the reference: an invocation whose pid has no
 * remaining response (a crashed client, a timeout) is an operation that never
 * happened.  qsmd_check_pending_batch also lets it take effect, at any point
 * after its invocation, with a response nobody saw.  The search is the check
 * call's with two changes:
 *
 *   1. A candidate (state s, invocation i) whose pid has no remaining
 *      response has one child per response symbol r, in ascending order, with
 *      bit r of post[s][i] set and bit r of post_err[s][i] clear: an *assumed*
 *      response.  Each is one counted node (max_nodes is tested before it);
 *      its postcondition is not evaluated again; its state is
 *      on_resp[on_inv[s][i]][r]; its remaining set loses the pid's first
 *      remaining invocation and no response.  No allowed symbol: no child, no
 *      node, as today.
 *   2. A non-empty history that holds no response event at all and whose root
 *      has no child is LINEARISABLE with 0 nodes and an empty witness.
 *
 * A pending invocation that is never chosen stays in the remaining set; a
 * node without children succeeds, which reads "it never took effect".  On a
 * history with nothing pending the call equals qsmd_check_batch in status,
 * nodes and witness.  With raise tables the call can read MODEL_ERROR where
 * the check call reads LINEARISABLE: an assumed operation can lead the search
 * to a raising postcondition (the reference's first-raise rule on more paths).
 *
 * With QSMD_FLAG_WITNESS, assumed_out[ev_off + d] is the response symbol
 * assumed at witness level d, or QSMD_ASSUMED_NONE for an observed response
 * (written for the levels of the witness and its terminator; the witness
 * layout, n_events bytes; may be NULL).  A witness can be as long as the
 * history has invocations.  Replay: an assumed level removes only the pid's
 * first remaining invocation.
 *
 * "table_budget", max_nodes, the time limit, the totals, the probe and the
 * ENCODE_ERROR rules are the check call's; the knob "table_memo" is ignored.
 * Knob "pending_memo" (default 0 = off: exactly the launches above; else a
 * power of two in 2..2^20, anything else QSMD_ERR_ARG and the old value
 * stays): the second pass of these two calls, and of no other, keeps
 * "table_memo"'s exact-count state memo of that many entries per lane slot.
 * Status, node count, witness, assumed bytes and totals are unchanged; a
 * max_nodes inside a folded subtree gives BUDGET with nodes == max_nodes, a
 * count beyond 2^64 - 1 BUDGET with nodes == 2^64 - 1.  The tables are
 * "table_memo"'s allocation and sizing ("table_memo_grid" included).  A width
 * class whose memo kernel would pass the device's LDS limit (the 128-event
 * class with tables over 48 KB) runs the plain second pass.  With
 * "table_budget" 0 the knob is inert.  qsmd_get_param "pending_memo_hits_last":
 * the memo's hits in the most recent pending call (waits for it; 0 when that
 * call ran without the memo); "table_memo_hits_last" is not moved by it.
 * Models 1, 2, 4, 5 and QSMD_FLAG_EARLY_EXIT_BATCH return
 * QSMD_ERR_UNSUPPORTED (model 5 has entries of its own:
 * qsmd_check_kpending_batch below). */
#define QSMD_ASSUMED_NONE 0xFFu

/* Host memory, synchronous (as qsmd_check_batch). */
int qsmd_check_pending_batch(qsmd_ctx* ctx, uint32_t model_id,
                             const qsmd_hdr* hdr, uint64_t n_hist,
                             const qsmd_event* events, uint64_t n_events,
                             const void* model0, uint32_t flags, uint64_t max_nodes,
                             uint8_t* status_out, uint64_t* nodes_out,
                             uint8_t* witness_out, qsmd_totals* totals_out,
                             uint8_t* assumed_out);

/* Device memory, asynchronous on `stream` (as qsmd_check_batch_device). */
int qsmd_check_pending_batch_device(qsmd_ctx* ctx, uint32_t model_id,
                                    const qsmd_hdr* hdr_dev, uint64_t n_hist,
                                    const qsmd_event* events_dev, uint64_t n_events,
                                    const void* model0_host, uint32_t flags,
                                    uint64_t max_nodes,
                                    uint8_t* status_dev, uint64_t* nodes_dev,
                                    uint8_t* witness_dev, qsmd_totals* totals_dev,
                                    void* stream, uint8_t* assumed_dev);

/* ----------------------------------------------------------- keyed pending
 * The same rule on the keyed table model (QSMD_MODEL_KTABLE; opt-in): the
 * pending call for the context's keyed table (qsmd_ktable_set), new entries
 * because qsmd_check_pending_batch keeps refusing model 5.
 *
 * A candidate (state vector s, invocation (k, i)) whose pid has no remaining
 * response has one child per response symbol r, ascending, with bit r of
 * post[s[k]][i] set and bit r of post_err[s[k]][i] clear; each is one counted
 * node (max_nodes is tested before it) whose postcondition is not evaluated
 * again, with s[k] := on_resp[on_inv[s[k]][i]][r] and every other key
 * unchanged; its remaining set loses the pid's first remaining invocation and
 * no response.  A non-empty history with no response event at all whose root
 * has no child is LINEARISABLE with 0 nodes and an empty witness.  On a
 * history with nothing pending, status, nodes and witness are
 * qsmd_check_batch(QSMD_MODEL_KTABLE)'s, bit for bit.
 *
 * model0: n_keys uint32 states or NULL, as for the keyed check call (a state
 * >= n_states: QSMD_ERR_ARG).  The witness and assumed layouts,
 * QSMD_ASSUMED_NONE, the totals, the probe ("table_pass2_last") and the time
 * limit are qsmd_check_pending_batch's; "table_budget" and max_nodes apply as
 * for every table call; a history's ENCODE_ERROR follows the keyed check
 * call's rules (hdr.model_id, a symbol the component does not have, a key >=
 * n_keys).  No keyed table set: QSMD_ERR_ARG.  QSMD_FLAG_EARLY_EXIT_BATCH:
 * QSMD_ERR_UNSUPPORTED.
 *
 * By default it is the plain search on the product, and always the plain
 * search: the knobs "ktable_memo", "ktable_local", "table_memo" and
 * "pending_memo" do not reach it, and "ktable_local_last" and
 * "pending_memo_hits_last" are not moved by it ("table_memo_hits_last" reads
 * 0 after it, as after qsmd_check_pending_batch without its memo).  One
 * workgroup needs the component's tables and 12 / 24 / 48 KB of LDS (32 / 64 /
 * 128-event class): 128 KB at the largest component in the widest class.
 *
 * Local mode -- knob "kpending_local" (qsmd_set_param / qsmd_get_param;
 * default 0 = off: every launch and result as above; 1 = on; any other value
 * QSMD_ERR_ARG and the old value stays).  The rule above is local as well: a
 * pending invocation on one key helps no other.  With the knob at 1,
 * qsmd_check_kpending_batch and qsmd_check_kpending_batch_device check every
 * history that is *splittable here* key by key.  The knob reaches no other
 * call ("ktable_local" is the check call's and does not reach this one);
 * "ktable_memo", "table_memo" and "pending_memo" still do not reach this call.
 *   - Splittable here is QSMD_MODEL_KTABLE's definition (above) with one
 *     change to (2): a pid's events in history order alternate invocation,
 *     response, ..., from an invocation, and may end on an invocation.  That
 *     last invocation is pending and belongs to the key in its own a byte.
 *     Still on the product route, status and nodes those of the knob at 0 bit
 *     for bit: a lone response (a pid whose first event, or whose event after
 *     a response, is a response); a pid with two operations in flight, which
 *     covers an invocation after a pending one of the same pid; every encode
 *     error (a code >= n_inv / n_resp, a key >= n_keys); a header that fails
 *     the header test (model_id != 5, n_ev > 128, ev_off + n_ev > n_events).
 *   - Sub-history k, for each key k in ascending order: the events of the
 *     operations invoked on key k (an operation is an invocation and, if the
 *     pid has a later event, the pid's next event), in history order, bytes
 *     unchanged, the same header but for ev_off and n_ev.  Each is searched
 *     by the rule above with the call's flags, max_nodes (applied to each
 *     part on its own), time limit, "table_budget" and model0's state for
 *     that key (the whole model0 vector is passed on; a part moves one key's
 *     state only).  Every part is searched: no short cut across keys.
 *   - The rule's last sentence applies per part: a part with no response
 *     event whose root has no child is LINEARISABLE with 0 nodes.  A key with
 *     no operation is an empty part: LINEARISABLE, 0 nodes.
 *   - The history's status is that of the lowest key whose part is not
 *     LINEARISABLE, or LINEARISABLE when there is none; its nodes is the sum
 *     over its parts.  qsmd_totals counts histories (nodes: the sum of the
 *     per-history values); qsmd_timed_out and "table_pass2_last" describe the
 *     launch over the parts.
 *   - A call that carries QSMD_FLAG_WITNESS takes the product route whole,
 *     witness and assumed included, as if the knob were 0, and
 *     "kpending_local_last" reads 0 after it.  So does a call with more than
 *     (2^32-1) / n_keys histories.
 *   - "kpending_local_last" (qsmd_get_param; waits for the call): the
 *     histories that were split in the most recent keyed pending call, 0 when
 *     it took the product route.  The two counters are separate:
 *     "ktable_local_last" is not moved by a keyed pending call,
 *     "kpending_local_last" is not moved by a check call.
 *   - The call stays asynchronous on the caller's stream.  As for
 *     "ktable_local", with the knob at 1 the event slots [ev_off, ev_off +
 *     n_ev) of different headers must not overlap.
 * Promised: for a component without post_err, a splittable history's verdict
 * is the product route's whenever neither side ends in BUDGET.  Not promised:
 * node counts are per key, summed, not the product's; BUDGET is per key (a
 * history the product search leaves BUDGET is usually decided); and with
 * post_err a failing history may read NONLINEARISABLE where the product reads
 * MODEL_ERROR, or the reverse.  The ABI version is unchanged. */

/* Host memory, synchronous (as qsmd_check_batch). */
int qsmd_check_kpending_batch(qsmd_ctx* ctx,
                              const qsmd_hdr* hdr, uint64_t n_hist,
                              const qsmd_event* events, uint64_t n_events,
                              const void* model0, uint32_t flags, uint64_t max_nodes,
                              uint8_t* status_out, uint64_t* nodes_out,
                              uint8_t* witness_out, qsmd_totals* totals_out,
                              uint8_t* assumed_out);

/* Device memory, asynchronous on `stream` (as qsmd_check_batch_device). */
int qsmd_check_kpending_batch_device(qsmd_ctx* ctx,
                                     const qsmd_hdr* hdr_dev, uint64_t n_hist,
                                     const qsmd_event* events_dev, uint64_t n_events,
                                     const void* model0_host, uint32_t flags,
                                     uint64_t max_nodes,
                                     uint8_t* status_dev, uint64_t* nodes_dev,
                                     uint8_t* witness_dev, qsmd_totals* totals_dev,
                                     void* stream, uint8_t* assumed_dev);

/* Safety net: a search launch whose lanes run longer than this wall time
 * stops and reports QSMD_STATUS_BUDGET for the unfinished histories (default
 * 120000 ms; 0 disables).  Not part of the reference semantics. */
int qsmd_set_time_limit_ms(qsmd_ctx* ctx, uint64_t ms);

/* Tuning knob: cap on the number of workgroups of the first search stage
 * (beyond it each workgroup loops over several groups of 64 histories).
 * Default 65536.  Does not change any result. */
int qsmd_set_stage0_grid(qsmd_ctx* ctx, uint64_t max_blocks);

/* Tuning knob: node budget of the first search stage (0 = none).  A history
 * whose search needs more nodes goes on in the heavy stage (one lane per
 * history with an exact-count state memo, from the saved search state; or
 * one wavefront per history), so one long search does not hold 63 idle
 * lanes.  Default (until set; knob "stage0_budget_auto" 1 restores it):
 * automatic -- 24, or 16 while the context's last finished call sent fewer
 * than 1 in 50 histories to the heavy stage, back to 24 above 1 in 5.
 * Results are unchanged. */
int qsmd_set_stage0_budget(qsmd_ctx* ctx, uint64_t nodes);

/* Tuning knobs by name (none changes a result):
 *   "stage0_budget"     as qsmd_set_stage0_budget
 *   "stage0_budget_auto" 1: the automatic stage-0 budget (the default)
 *   "stage0w_budget"    the same for 33..64-event histories (default: automatic,
 *                       24 when the heavy stage runs in lane mode, 48 in
 *                       wave mode; "stage0w_budget_auto" 1 restores it)
 *   "stage0_grid"       as qsmd_set_stage0_grid
 *   "split_budget"      as qsmd_set_split_budget
 *   "split_xmemo"       1 (default): the giant stage's exact-count memo
 *   "heavy_mode"        2 (default): the heavy stage in lane mode (one lane
 *                       per history, a private memo table per lane) when the
 *                       last finished call sent more than "wave_max"
 *                       (default 16384) histories there, or sent under a
 *                       fifth of its batch and had no wide (65..128-event)
 *                       history; else wave mode (one wavefront per history,
 *                       the state DAG or the DFS in wave-uniform registers,
 *                       an LDS memo per wavefront); 0: always wave mode; 1:
 *                       always lane mode
 *   "memo_lds"          lane mode's memo tables: 1 (default) in LDS when the
 *                       last finished call's heavy histories fit one
 *                       workgroup per CU, else in HBM; 0: always HBM (an
 *                       LDS-table workgroup holds a CU); 2: always LDS
 *   "memo_lds_entries"  the LDS tables' entries per lane, a power of two in
 *                       4..64 (default 64: 128 KB per workgroup; 16: 32 KB)
 *   "memo_grid", "memo_lane_entries"  lane mode: workgroups at most (0 = 12
 *                       per CU), entries per lane (HBM tables: grid x 64 x
 *                       entries x 96 B, grown on demand; the LDS tables hold
 *                       min(memo_lds_entries, entries))
 *   "wave_grid"         wave mode workgroups (0 = the last call's heavy count
 *                       + 25 %, at most 16 per CU; grid-stride beyond)
 *   "wave_min_rem"      wave mode: no memo probe at nodes with at most this
 *                       many remaining events (default 4)
 *   "dag_states"        wave mode: capacity in states of the per-wavefront
 *                       state DAG (default 128, items 4x that; 0 = the DFS
 *                       for every history); a history whose DAG does not fit
 *                       runs the DFS.  A TicketDispenser history whose DAG is
 *                       a chain (every history on one pid) runs as one
 *                       (scalar mask work, no DAG arrays) unless it is 0
 *   "memo_after"        lane mode: the memo probes a search's nodes after
 *                       it counted this many (default 32; its failed
 *                       subtrees are recorded from the start)
 *   "tail_cap", "tail_min"  lane mode: a search still running after tail_cap
 *                       wavefront iterations (default 256; 0 = never) goes to
 *                       a wave-mode launch after the heavy stage and is
 *                       searched there from the root (the state DAG), when
 *                       the last finished call sent at least tail_min
 *                       (default 65536) histories, and a fifth of its batch,
 *                       to the heavy stage (tail_min 0: whatever it sent)
 *   "heavy_buckets"     1 (default): for the same long lists, the heavy
 *                       stage forms its groups of 64 in order of predicted
 *                       work (stage 0 records each heavy history's untried
 *                       candidates on its stack; a counting sort orders the
 *                       list); 0: in list order
 *   "resume_cap"        lane mode: stage 0's saved search states, slots per
 *                       heavy-list shard (0 = automatic: twice the last
 *                       call's heavy count per shard, at least 1024); a heavy
 *                       history past them starts again at the root
 *   "fold"              lane mode: 1 (default) no stage-0w launch after a
 *                       call that deferred nothing to it (the heavy stage
 *                       takes what stage 0 defers on to the giant stage);
 *                       0: every call launches it
 *   "timing_events"     1: record the per-call timing events (qsmd_timing_read,
 *                       qsmd_last_kernel_ms); 0 (default until
 *                       qsmd_timing_reset): none
 *   "giant_grid"        giant stage workgroups (0 = automatic: 1 when the last
 *                       finished call had no giant, deferred nothing and had
 *                       no wide history and this is no early-exit call -- a
 *                       call that has giants after all runs them on that
 *                       grid, once; 2 per CU before any call has finished,
 *                       after a call with giants and on lane mode's folded
 *                       route; an early-exit call without them: one per
 *                       fixup chunk, 8 to 2 per CU; else 64)
 *   "wave_stats_ptr", "memo_stats_ptr", "memo_stats_groups"  diagnostics:
 *                       device buffers: wave mode 16 x u64 (DFS iterations
 *                       max / sum, s_memtime cycles max / sum, nodes sum per
 *                       DFS-searched history; DAG-searched histories, their
 *                       cycles max / sum, per-phase cycles, levels;
 *                       tools/wave_stats.py), lane mode per-group
 *                       records (tools/memo_stats.py)
 *   "giant_stall_us"    diagnostic: the workgroup of the giant stage's first
 *                       frontier chunk starts this late (tests of the time
 *                       limit's phase-wait safety net: a giant combined by a
 *                       workgroup that gave up waiting is BUDGET) */
int qsmd_set_param(qsmd_ctx* ctx, const char* name, uint64_t value);

/* Read a knob ("table_budget", "stage0_budget": 0 while automatic, "stage0w_budget_auto", "fold",
 * "heavy_mode", "memo_after", "resume_cap", "tail_cap", "tail_min", "heavy_buckets", "giant_grid"),
 * "giant_grid_last": the giant stage's workgroups in the most recent Bank /
 * Ticket check call, or "stage0_budget_last": the stage-0 budget the most recent
 * finished check call ran with (the automatic one included; waits for the
 * context's last call). */
int qsmd_get_param(qsmd_ctx* ctx, const char* name, uint64_t* out);

/* Tuning knob (default 1024): histories the compact stages cannot hold go to
 * the giant stage, which first searches each one in a lane for 16 x this
 * many iterations and otherwise splits it over many lanes (see "Split
 * search" below); the heavy stage hands it a history after 64 x this many
 * iterations.  0 disables the split (every search runs to its end in one
 * lane or wavefront).  Results are unchanged. */
int qsmd_set_split_budget(qsmd_ctx* ctx, uint64_t nodes);

/* QSMD_FLAG_MEMO: the giant stage keeps a table in HBM of search states
 * (remaining events, model) known to fail, shared by every lane searching the
 * same history, and prunes a subtree whose root state is in it.  Verdicts
 * and witnesses are unchanged; node counts of the giant stage's histories
 * become "nodes explored" (fewer than the reference's, and not reproducible
 * from run to run).  Capacity in entries of 64 B, a power of two (default
 * 1 << 22 = 256 MiB, allocated on first use). */
int qsmd_set_memo_capacity(qsmd_ctx* ctx, uint64_t entries);

/* ----------------------------------------------------------- split search
 *
 * One very large history searched by many GPUs.  The
 * reference DFS (src/Linearisability.hs:52-69) is cut at depth `depth`:
 * every node it reaches at that depth (a passed postcondition, i.e. a `step`
 * that recurses) roots a task, its subtree.  Tasks come in the reference's
 * DFS order, each with the number of nodes the reference counts up to and
 * including its root.  Searching the tasks anywhere, in any order, and
 * folding the results in task order (qsmd_combine_tasks) gives the verdict,
 * exhaustive node count and witness of the single search. */
#define QSMD_SPLIT_MAX_DEPTH 16

typedef struct qsmd_task {
    uint32_t hist;          /* history index in the batch (0 for this API)   */
    uint16_t depth;         /* prefix length d (<= QSMD_SPLIT_MAX_DEPTH)     */
    uint16_t reserved;
    uint64_t top_before;    /* reference nodes up to and including the root  */
    uint8_t  path[QSMD_SPLIT_MAX_DEPTH];  /* invocation event chosen at each */
                                          /* prefix level (witness indices)  */
} qsmd_task;

typedef struct qsmd_frontier {
    uint32_t status;        /* the search above the cut: NONLINEARISABLE =   */
                            /* exhausted (the tasks decide); LINEARISABLE /  */
                            /* MODEL_ERROR = decided after top_nodes unless  */
                            /* a task decides first; BUDGET; ENCODE_ERROR    */
    uint32_t depth;         /* cut depth chosen                              */
    uint64_t top_nodes;     /* nodes counted above the cut                   */
    uint64_t n_tasks;
} qsmd_frontier;

/* Cut the search of ONE history (hdr[0]) at the smallest depth that yields
 * at least min_tasks tasks (at most max_tasks, depth <= 16).  witness_out
 * (n_ev bytes, may be NULL) receives the path when the search above the cut
 * ends LINEARISABLE. */
int qsmd_split_frontier(qsmd_ctx* ctx, uint32_t model_id, const qsmd_hdr* hdr,
                        const qsmd_event* events, uint64_t n_events,
                        const void* model0, uint32_t flags, uint64_t max_nodes,
                        uint32_t min_tasks, qsmd_task* tasks_out, uint64_t max_tasks,
                        qsmd_frontier* frontier_out, uint8_t* witness_out);

/* Search the subtrees of tasks[0..n_tasks) of history hdr[0] (tasks in DFS
 * order; any subset of a frontier, kept in order).  Per task: status
 * LINEARISABLE = the subtree holds a linearisation, NONLINEARISABLE = it
 * does not, MODEL_ERROR, BUDGET, SKIPPED = not searched because an earlier
 * task of this call decided; nodes = nodes of the subtree below its root
 * up to its decision; witness_out (n_tasks x 64 B, may be NULL) = the full
 * path of a LINEARISABLE task.  QSMD_FLAG_MEMO applies. */
int qsmd_check_tasks(qsmd_ctx* ctx, uint32_t model_id, const qsmd_hdr* hdr,
                     const qsmd_event* events, uint64_t n_events,
                     const void* model0, uint32_t flags, uint64_t max_nodes,
                     const qsmd_task* tasks, uint64_t n_tasks,
                     uint8_t* status_out, uint64_t* nodes_out, uint8_t* witness_out);

/* Fold task results in DFS order (host only, no device).  winner_out = index
 * of the deciding task, -1 when the decision came from above the cut. */
int qsmd_combine_tasks(const qsmd_frontier* frontier, const qsmd_task* tasks,
                       const uint8_t* status, const uint64_t* nodes, uint64_t n_tasks,
                       uint64_t max_nodes, uint8_t* status_out, uint64_t* nodes_out,
                       int64_t* winner_out);

/* ------------------------------------------------------------ wellformed
 *
 * Batched `wellformed pids history` (src/Linearisability.hs:97-135; call
 * site test/Bank.hs:281-283): every listed pid's subhistory must be
 * sequential; the result is the first NotSequential error in `pids` order,
 * as the constructor code, the pid and the history-local indices of the
 * events it names (ev0 = the first, ev1 = the second; equal when it names
 * one).  InvocationFollowedByNonMatchingResponse compares the pids of one
 * subhistory, which are equal, so wellformed never returns it. */
typedef struct qsmd_wf {
    uint8_t  code;      /* QSMD_WF_*                                         */
    uint8_t  pid;       /* dense pid of the failing subhistory               */
    uint16_t ev0;
    uint16_t ev1;
    uint16_t reserved;
} qsmd_wf;

#define QSMD_WF_OK                                         0u
#define QSMD_WF_FIRST_EVENT_ISNT_INVOCATION                1u
#define QSMD_WF_INVOCATION_FOLLOWED_BY_INVOCATION          2u
#define QSMD_WF_INVOCATION_FOLLOWED_BY_NON_MATCHING_RESPONSE 3u
#define QSMD_WF_RESPONSE_FOLLOWED_BY_RESPONSE              4u
#define QSMD_WF_RESPONSE_FOLLOWED_BY_INVOCATION            5u
#define QSMD_WF_LONE_RESPONSE                              6u
#define QSMD_WF_ENCODE_ERROR                               0xFEu

/* pids: the `pids` list as dense pid indices (< 128, each at most once),
 * applied to every history; NULL = all pids in order 0, 1, 2, ...
 * Host buffers, synchronous. */
int qsmd_wellformed_batch(qsmd_ctx* ctx, const qsmd_hdr* hdr, uint64_t n_hist,
                          const qsmd_event* events, uint64_t n_events,
                          const uint8_t* pids, uint32_t n_pids, qsmd_wf* out);
/* Same on device-resident hdr / events / out, enqueued on `stream`. */
int qsmd_wellformed_batch_device(qsmd_ctx* ctx, const qsmd_hdr* hdr_dev, uint64_t n_hist,
                                 const qsmd_event* events_dev, uint64_t n_events,
                                 const uint8_t* pids, uint32_t n_pids, qsmd_wf* out_dev,
                                 void* stream);

/* Device time (ms, HIP events on the launch stream) of the search kernels of
 * the most recent timed check call, measured once that stream has completed.
 * Timing is off until qsmd_timing_reset (or knob "timing_events" 1): the
 * events are three packets per call on the caller's stream. */
int qsmd_last_kernel_ms(qsmd_ctx* ctx, float* ms_out);

/* Per-call device timings since the last reset, which also turns timing on
 * (at most the last 1024 calls):
 * stage0_ms[i] = the first (dominant) search kernel (0 when the host entry
 * skipped stage 0: no history of the call fitted it), call_ms[i] = every
 * kernel of call i.  Synchronises on the recorded events. */
int qsmd_timing_reset(qsmd_ctx* ctx);
int qsmd_timing_read(qsmd_ctx* ctx, float* stage0_ms, float* call_ms, uint64_t max,
                     uint64_t* n_out);
/* The same with heavy_ms[i] = the heavy-stage kernel of call i in lane mode
 * (events the launch records at its start and end; -1 in wave mode).  Any of
 * the three arrays may be NULL. */
int qsmd_timing_read_stages(qsmd_ctx* ctx, float* stage0_ms, float* heavy_ms, float* call_ms,
                            uint64_t max, uint64_t* n_out);

/* Diagnostic: out4 = [histories stage 0 passed to stage 0w, heavy histories
 * of stage 0, heavy histories of stage 0w, giants] of the most recent check
 * call (waits for it). */
int qsmd_probe_read(qsmd_ctx* ctx, uint32_t* out4);

/* Whether the time limit (qsmd_set_time_limit_ms) fired in the most recent
 * check call (waits for it): *out = 1 when some of its QSMD_STATUS_BUDGET
 * results come from the time limit rather than max_nodes, else 0. */
int qsmd_timed_out(qsmd_ctx* ctx, int* out);

#ifdef __cplusplus
}
#endif

#endif /* QSMD_H */
