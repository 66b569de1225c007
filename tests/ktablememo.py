"""CPU references for the keyed path's exact-count state memo
(csrc/ktable.hip, knob "ktable_memo").

TEST INFRASTRUCTURE ONLY.

* the deep keyed histories of the GPU tests (:func:`kreads`,
  :func:`klin_deep`, :func:`klock_deep`) and the table of their known answers
  (:data:`KDEEP`).  The answers are ``tablememo.exact_count`` on
  ``ktablegen.product(component, K)``: never the code under test.
* :func:`kmemo_dfs` -- a literal mirror of ``TableLane::check_step<KeyedModel, MEMO>``, which is
  ``tablememo.memo_dfs`` with the 64-bit packed state (key k in bits 8k ..
  8k + 7), the kernel's slot hash over both state words, and a lossy
  direct-mapped table.  ``state_mask`` weakens the memo's key (hash and hit
  test see only ``state & state_mask``): the tests use it to show that the
  deep rows tell a memo that keys on part of the state from a right one.
"""

from __future__ import annotations

import functools

import ktablegen as kg
import tablegen as tg
import tablememo as tm

U64 = tm.U64
L, R = tg.L, tg.R
COMPONENTS = {"register": tg.REGISTER, "lock": tg.LOCK}


@functools.lru_cache(maxsize=None)
def product(name, K):
    return kg.product(COMPONENTS[name], K)


# ---------------------------------------------------------------------------
# deep histories (pids 0 .. w - 1)
# ---------------------------------------------------------------------------

def _write_prologue(K):
    h = []
    for k in range(K):
        h += [(0, L((k, ("Write", 0)))), (1, L((k, ("Write", 1)))), (0, R("Ok")), (1, R("Ok"))]
    return h


def kreads(K, widths, keys=None):
    """Register^K: both writes overlapped on every key, then per round r of
    width w, w overlapping reads of key keys[r] (default r % K) answered
    Val 0; the very last answer is Val 1 (no order explains it)."""
    h = _write_prologue(K)
    for r, w in enumerate(widths):
        k = keys[r] if keys is not None else r % K
        h += [(p, L((k, "Read"))) for p in range(w)] + [(p, R(("Val", 0))) for p in range(w)]
    h[-1] = (h[-1][0], R(("Val", 1)))
    return h


def klin_deep(K, w, rounds):
    """Register^K: the write prologue, rounds of w overlapping failing Cas on
    key (K - 1 - r) % K, then every key read as 0 -- linearisable only with
    Write 1 before Write 0 on every key."""
    h = _write_prologue(K)
    for r in range(rounds):
        k = (K - 1 - r) % K
        h += [(p, L((k, ("Cas", 3, 3)))) for p in range(w)] + [(p, R("CasFail")) for p in range(w)]
    for k in range(K):
        h += [(0, L((k, "Read"))), (0, R(("Val", 0)))]
    return h


def klock_deep(K, w, rounds):
    """Lock^K: Lock and Unlock overlapped on every key, then rounds of w
    IsLocked on key (K - 1 - r) % K answered No, the very last Yes: an order
    with Unlock first raises."""
    h = []
    for k in range(K):
        h += [(0, L((k, "Lock"))), (1, L((k, "Unlock"))), (0, R("Ok")), (1, R("Ok"))]
    for r in range(rounds):
        k = (K - 1 - r) % K
        h += [(p, L((k, "IsLocked"))) for p in range(w)] + [(p, R("No")) for p in range(w)]
    h[-1] = (h[-1][0], R("Yes"))
    return h


# name -> (component, K, history, events, status, nodes, distinct (rem, state))
KDEEP = {
    "kreads_2_3x2": ("register", 2, kreads(2, [3] * 2), 20, "nonlin", 132, 31),
    "kreads_8_4x4_k7373": ("register", 8, kreads(8, [4] * 4, keys=[7, 3, 7, 3]), 64, "nonlin", 29900284, 5309),
    "kreads_8_4x8_k76543210": ("register", 8, kreads(8, [4] * 8, keys=[7, 6, 5, 4, 3, 2, 1, 0]), 96, "nonlin",
                               202638646780, 4839),
    "kreads_8_4x12": ("register", 8, kreads(8, [4] * 12), 128, "nonlin", 51406392555494908, 4898),
    "kreads_4_8x4": ("register", 4, kreads(4, [8] * 4), 80, "nonlin", 1797298063189725564, 3759),
    "klin_deep_2_3_2": ("register", 2, klin_deep(2, 3, 2), 24, "lin", 479, 64),
    "klin_deep_5_4_4": ("register", 5, klin_deep(5, 4, 4), 62, "lin", 47530577, 2032),
    "klin_deep_8_4_2": ("register", 8, klin_deep(8, 4, 2), 64, "lin", 698188, 8934),
    "klin_deep_8_4_8": ("register", 8, klin_deep(8, 4, 8), 112, "lin", 133363421949412, 31908),
    "klock_deep_3_3_2": ("lock", 3, klock_deep(3, 3, 2), 24, "error", 76, 17),
    "klock_deep_8_4_4": ("lock", 8, klock_deep(8, 4, 4), 64, "error", 467025, 69),
    "klock_deep_8_4_10": ("lock", 8, klock_deep(8, 4, 10), 112, "error", 89247150380625, 159),
}
# the rows of the lossy-table tests, per entry count (the others are beyond
# the iteration cap there)
LOSSY_ROWS = ["kreads_2_3x2", "klin_deep_2_3_2", "klock_deep_3_3_2", "klin_deep_8_4_2", "klock_deep_8_4_4"]
LOSSY = {2: LOSSY_ROWS, 16: LOSSY_ROWS + ["kreads_8_4x4_k7373", "klin_deep_5_4_4"]}
# max_nodes at, one below and one above the exact count
BUDGET_CASES = [("kreads_8_4x4_k7373", 29900283, ("budget", 29900283)),
                ("kreads_8_4x4_k7373", 29900284, ("nonlin", 29900284)),
                ("kreads_8_4x4_k7373", 29900285, ("nonlin", 29900284)),
                ("klin_deep_8_4_2", 698187, ("budget", 698187)), ("klin_deep_8_4_2", 698188, ("lin", 698188))]
ITERATION_CAP = 1_000_000


def exact(name, max_nodes=0, stats=None):
    comp, K, hist = KDEEP[name][:3]
    return tm.exact_count(product(comp, K), hist, max_nodes, stats)


# ---------------------------------------------------------------------------
# kmemo_dfs: TableLane::check_step<KeyedModel, MEMO>, literally
# ---------------------------------------------------------------------------

HASH_S = (0x165667B1, 0xD6E8FEB9)       # the state's low and high word


def kmemo_slot(rem, n_words, state, entries):
    """The kernel's slot hash (table_search.h TableMemo::slot_of, 64-bit state)."""
    x = ((state & 0xFFFFFFFF) * HASH_S[0]) & 0xFFFFFFFF
    x ^= ((state >> 32) * HASH_S[1]) & 0xFFFFFFFF
    for k in range(n_words):
        x ^= (((rem >> (32 * k)) & 0xFFFFFFFF) * tm.HASH_K[k]) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    return x & (entries - 1)


_ctz = tm._ctz


def kmemo_dfs(comp, K, hist, entries, max_nodes=0, info=None, model0=None, state_mask=U64):
    """(status, nodes, path) as the kernel's memo pass computes them on
    ``comp``^K (``comp``: "register" / "lock"); ``entries`` 0 is the plain
    search.  ``model0``: K component state values (default: the initial one
    everywhere).  ``info`` (a dict) receives "iterations" and "hits"."""
    t = tm._table(comp)
    n = len(hist)
    if n == 0:
        return "lin", 0, []
    n_words = 1 if n <= 32 else (2 if n <= 64 else 4)
    ALL = (1 << n) - 1
    RESP = sum(1 << k for k, (_, (kind, _)) in enumerate(hist) if kind == "R")
    INV = ALL & ~RESP
    pid_mask = {}
    for k, (pid, _) in enumerate(hist):
        pid_mask[pid] = pid_mask.get(pid, 0) | (1 << k)
    code = [t.inv_index[x[1]] if kind == "L" else t.resp_index[x] for _, (kind, x) in hist]
    key = [x[0] if kind == "L" else 0 for _, (kind, x) in hist]
    assert all(0 <= k < K for k in key)
    limit = max_nodes if max_nodes else U64
    post = [[int(v) for v in row] for row in t.post]
    post_err = [[int(v) for v in row] for row in t.post_err] if t.post_err is not None else None
    on_inv = [[int(v) for v in row] for row in t.on_inv]
    on_resp = [[int(v) for v in row] for row in t.on_resp]

    def cands(rem):
        rr, c = rem & RESP, rem & INV
        return c & ((1 << _ctz(rr)) - 1) if rr else c

    def topbit(x):
        return 1 << (x.bit_length() - 1) if x else 0

    rem = INV | RESP
    cand = cands(rem)
    start = [t.init_state] * K if model0 is None else [t.state_index[v] for v in model0]
    state = sum(s << (8 * k) for k, s in enumerate(start))
    depth, found, nodes = 0, 0, 0
    stk, entry = [None] * (n // 2 + 1), [0] * (n // 2 + 1)
    table = [None] * entries
    skip = False
    iters = hits = 0
    status = None
    while status is None:
        iters += 1
        empty = cand == 0
        if empty and (found == 0 or depth == 0):
            status = "lin" if (not found and depth > 0) else "nonlin"
            break
        if empty:
            depth -= 1
            if entries and not skip:                     # the subtree left has failed
                table[kmemo_slot(rem, n_words, state & state_mask, entries)] = (rem, state & state_mask,
                                                                                nodes - entry[depth])
            skip = False
            j, was = stk[depth]
            shift = 8 * key[j]
            state = (state & ~(0xFF << shift)) | (was << shift)
            gone = ~rem & pid_mask[hist[j][0]] & ALL
            rem |= topbit(gone & INV) | topbit(gone & RESP)
            cand = cands(rem) & ~((1 << (j + 1)) - 1)
            found = 1
            if cand == 0:
                continue
        j = _ctz(cand)
        cand &= cand - 1
        pmj = pid_mask[hist[j][0]]
        rr = rem & pmj & RESP
        if not rr:
            continue
        if nodes >= limit:
            status = "budget"
            break
        r = _ctz(rr)
        i, rc = code[j], code[r]
        shift = 8 * key[j]
        sk = (state >> shift) & 0xFF
        ok = (post[sk][i] >> rc) & 1
        err = (post_err[sk][i] >> rc) & 1 if post_err is not None else 0
        nodes += 1
        found = 1
        if err:
            status = "error"
            break
        if ok:
            stk[depth] = (j, sk)
            depth += 1
            state ^= (sk ^ on_resp[on_inv[sk][i]][rc]) << shift
            lowest_inv = (rem & pmj & INV) & -(rem & pmj & INV)
            rem &= ~(lowest_inv | (1 << r))
            cand = cands(rem)
            found = 0
            if entries:
                entry[depth - 1] = nodes
                e = table[kmemo_slot(rem, n_words, state & state_mask, entries)]
                if e is not None and e[0] == rem and e[1] == state & state_mask:
                    hits += 1
                    if nodes + e[2] > limit:             # (u64 overflow included: limit <= 2^64 - 1)
                        nodes = limit
                        status = "budget"
                        break
                    nodes += e[2]
                    cand, found, skip = 0, 1, True
    if info is not None:
        info["iterations"], info["hits"] = iters, hits
    path = []
    if status == "lin":
        removed = 0
        for d in range(depth):
            j = stk[d][0]
            pm = pid_mask[hist[j][0]]
            live = ALL & ~removed
            r = _ctz(live & pm & RESP)
            i0 = _ctz(live & pm & INV)
            path.append((hist[j][0], hist[j][1][1], hist[r][1][1]))
            removed |= (1 << i0) | (1 << r)
    return status, nodes, path


@functools.lru_cache(maxsize=None)
def mirror(name, entries, max_nodes=0):
    """kmemo_dfs on a KDEEP row, computed once and shared:
    (status, nodes, path, iterations, hits)."""
    comp, K, hist = KDEEP[name][:3]
    info = {}
    st, nd, path = kmemo_dfs(comp, K, hist, entries, max_nodes, info)
    return st, nd, path, info["iterations"], info["hits"]
