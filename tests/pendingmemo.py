"""CPU references for the pending search's exact-count state memo
(csrc/tpending.hip, knob "pending_memo").

TEST INFRASTRUCTURE ONLY.

* :func:`exact_count_pending` -- what ``pending_ref.linearisable_pending``
  returns (status and node count), computed without walking its tree: a
  memoised recursion over (remaining events, model state) that restates
  ``pending_ref.interleavings`` on a tuple of event indices (``filter1``,
  ``findResponse``, else one child per ``pending_ref.allowed`` symbol, counted
  but not tested), plain ``any`` at the root, ``any'`` below, and the rule of
  the root without a child in a history without a response.
* :func:`pending_memo_dfs` -- a literal mirror of ``TableLane::pending_step<MEMO>`` (csrc/table_search.h):
  Lemma L1 bitsets, one child per iteration, the resume of an assumed level at
  its next allowed symbol, a lossy direct-mapped table of ``entries`` entries
  with the kernel's slot hash (``tablememo.memo_slot``).
* the deep crashed histories of the GPU tests (:func:`crashed_reads`,
  :func:`crashed_lin_deep`, :func:`crashed_lock`, :func:`crashed_lock_error`)
  and the table of their known answers (:data:`DEEP`).

A model is a ``tablegen`` closure dict.
"""

from __future__ import annotations

import sys

import pending_ref as pr
import tablegen as tg
import tablememo as tm
from linearise_lists import ModelError

U64 = tm.U64
L, R = tg.L, tg.R


# ---------------------------------------------------------------------------
# exact_count_pending
# ---------------------------------------------------------------------------

def _children(model, hist, es, state):
    """``pending_ref.interleavings`` on a tuple of event indices:
    (j, response or symbol, es', assumed) per child."""
    out = []
    for j in es:
        pid, (kind, inv) = hist[j]
        if kind != "L":
            break                                        # takeInvocations
        first_inv = next(k for k in es if hist[k][0] == pid and hist[k][1][0] == "L")   # filter1
        es1 = tuple(k for k in es if k != first_inv)
        r = next((k for k in es1 if hist[k][0] == pid and hist[k][1][0] == "R"), None)  # findResponse
        if r is not None:
            out.append((j, hist[r][1][1], tuple(k for k in es1 if k != r), False))
        else:
            out += [(j, sym, es1, True) for sym in pr.allowed(model, state, inv)]
    return out


def exact_count_pending(model, hist, max_nodes=0, stats=None):
    """(status, nodes) of ``pending_ref.linearisable_pending``; with a limit
    smaller than the total, ("budget", max_nodes).  ``stats`` (a dict)
    receives "states": the distinct (remaining events, state) keys met."""
    tr, post = model["transition"], model["postcondition"]
    memo = {}

    def forest(es, state, root):
        key = (es, state)
        if key in memo:
            return memo[key]
        kids = _children(model, hist, es, state)
        if not kids:
            res = (not root, 0)                          # any' [] = True, any [] = False
        else:
            n, res = 0, None
            for j, resp, es2, assumed in kids:
                n += 1                                   # step evaluated
                inv = hist[j][1][1]
                if not assumed:
                    try:
                        ok = post(state, inv, resp)
                    except ModelError:
                        res = ("error", n)
                        break
                    if not ok:
                        continue
                out, sub = forest(es2, tr(tr(state, ("L", inv)), ("R", resp)), False)
                n += sub
                if out is not False:
                    res = (out, n)
                    break
            if res is None:
                res = (False, n)
        memo[key] = res
        return res

    if not hist:
        return "lin", 0
    es0 = tuple(range(len(hist)))
    if not _children(model, hist, es0, model["init"]) and not any(ev[0] == "R" for _, ev in hist):
        return "lin", 0                                  # nothing was observed: every operation dropped
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        out, n = forest(es0, model["init"], True)
    finally:
        sys.setrecursionlimit(old)
    if stats is not None:
        stats["states"] = len(memo)
    if max_nodes and n > max_nodes:
        return "budget", max_nodes
    return {True: "lin", False: "nonlin", "error": "error"}[out], n


# ---------------------------------------------------------------------------
# pending_memo_dfs: TableLane::pending_step<MEMO>, literally
# ---------------------------------------------------------------------------

def _ctz(x):
    return (x & -x).bit_length() - 1


def pending_memo_dfs(model, hist, entries, max_nodes, info=None):
    """(status, nodes, path) as the kernel's memo pass computes them, path the
    operations ``(pid, inv, resp, assumed)``; ``entries`` 0 is the plain
    search.  ``info`` (a dict) receives "iterations", "hits" and "trace": per
    hit (the nodes counted before it, the recorded count)."""
    t = tm._table(model["name"])
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
    code = [t.inv_index[x] if kind == "L" else t.resp_index[x] for _, (kind, x) in hist]
    symbols = (1 << len(t.resps)) - 1
    limit = max_nodes if max_nodes else U64

    def cands(rem):
        rr, c = rem & RESP, rem & INV
        return c & ((1 << _ctz(rr)) - 1) if rr else c

    def topbit(x):
        return 1 << (x.bit_length() - 1) if x else 0

    def words(state, i):
        pw = int(t.post[state, i])
        ew = int(t.post_err[state, i]) if t.post_err is not None else 0
        return pw, ew

    rem = INV | RESP
    cand = cands(rem)
    state, depth, found, nodes = t.init_state, 0, 0, 0
    stk, entry = [None] * n, [0] * n                     # one level per event
    table = [None] * entries
    skip = False
    iters = hits = 0
    trace = []
    status = None
    while status is None:
        iters += 1
        empty = cand == 0
        if empty and (found == 0 or depth == 0):
            status = "lin" if (not found and (depth > 0 or RESP == 0)) else "nonlin"
            break
        am, j = 0, 0
        if empty:
            depth -= 1
            if entries and not skip:                     # the subtree left has failed
                table[tm.memo_slot(rem, n_words, state, entries)] = (rem, state, nodes - entry[depth])
            skip = False
            j, state, sym = stk[depth]
            gone = ~rem & pid_mask[hist[j][0]] & ALL
            rem |= topbit(gone & INV)
            if sym is not None:                          # the symbols above the one popped
                pw, ew = words(state, code[j])
                am = pw & ~ew & symbols & ~((2 << sym) - 1)
            else:
                rem |= topbit(gone & RESP)
            cand = cands(rem) & ~((1 << (j + 1)) - 1)
            found = 1
            if am == 0 and cand == 0:
                continue
        if am == 0:
            j = _ctz(cand)
            cand &= cand - 1
        pmj = pid_mask[hist[j][0]]
        rr = rem & pmj & RESP
        observed = am == 0 and rr != 0
        i = code[j]
        pw, ew = words(state, i)
        if observed:
            if nodes >= limit:
                status = "budget"
                break
            r = _ctz(rr)
            rc = code[r]
            nodes += 1
            found = 1
            if (ew >> rc) & 1:
                status = "error"
                break
            if not (pw >> rc) & 1:
                continue
            level = (j, state, None)
            rem &= ~(1 << r)
        else:
            if am == 0:
                am = pw & ~ew & symbols
            if am == 0:
                continue                                 # no symbol: no child, no node
            if nodes >= limit:
                status = "budget"
                break
            rc = _ctz(am)
            nodes += 1
            level = (j, state, rc)
        stk[depth] = level
        depth += 1
        state = int(t.on_resp[int(t.on_inv[state, i]), rc])
        lowest_inv = (rem & pmj & INV) & -(rem & pmj & INV)
        rem &= ~lowest_inv
        cand = cands(rem)
        found = 0
        if entries:
            entry[depth - 1] = nodes
            e = table[tm.memo_slot(rem, n_words, state, entries)]
            if e is not None and e[0] == rem and e[1] == state:
                hits += 1
                trace.append((nodes, e[2]))
                if nodes + e[2] > limit:                 # (u64 overflow included: limit <= 2^64 - 1)
                    nodes = limit
                    status = "budget"
                    break
                nodes += e[2]
                cand, found, skip = 0, 1, True
    if info is not None:
        info["iterations"], info["hits"], info["trace"] = iters, hits, trace
    path = []
    if status == "lin":
        removed = 0
        for d in range(depth):
            j, _, sym = stk[d]
            pid, (_, inv) = hist[j]
            live = ALL & ~removed
            removed |= 1 << _ctz(live & pid_mask[pid] & INV)
            if sym is None:
                r = _ctz(live & pid_mask[pid] & RESP)
                removed |= 1 << r
                path.append((pid, inv, hist[r][1][1], False))
            else:
                path.append((pid, inv, t.resps[sym], True))
    return status, nodes, path


# ---------------------------------------------------------------------------
# deep crashed histories: the pending clients' pids are no one else's
# ---------------------------------------------------------------------------

CRASHED = 100           # the first pid of the pending clients

assert "Ok" in tg.REG_RESPS and ("Val", 2) in tg.REG_RESPS and "CasFail" in tg.REG_RESPS
assert {"Yes", "No"} <= set(tg.LOCK_RESPS)


def crashed_reads(widths, writers):
    """Register: ``writers`` pending ``Write 1`` first, then per round of width
    w, w overlapping reads answered Val 0; the very last answer is Val 2 (no
    order and no assumed write explains it)."""
    h = [(CRASHED + k, L(("Write", 1))) for k in range(writers)]
    for w in widths:
        h += [(p, L("Read")) for p in range(w)] + [(p, R(("Val", 0))) for p in range(w)]
    h[-1] = (h[-1][0], R(("Val", 2)))
    return h


def crashed_lin_deep(w, rounds):
    """Register: a pending Write 0 and a pending Write 1, rounds of w
    overlapping failing Cas, then a Read of 0."""
    h = [(CRASHED, L(("Write", 0))), (CRASHED + 1, L(("Write", 1)))]
    for _ in range(rounds):
        h += [(p, L(("Cas", 3, 3))) for p in range(w)] + [(p, R("CasFail")) for p in range(w)]
    return h + [(0, L("Read")), (0, R(("Val", 0)))]


def crashed_lock(w, rounds):
    """Lock: a pending Lock and a pending Unlock, rounds of w IsLocked
    answered No, the very last Yes."""
    h = [(CRASHED, L("Lock")), (CRASHED + 1, L("Unlock"))]
    for _ in range(rounds):
        h += [(p, L("IsLocked")) for p in range(w)] + [(p, R("No")) for p in range(w)]
    h[-1] = (h[-1][0], R("Yes"))
    return h


def crashed_lock_error(w, rounds):
    """``tablememo.lock_deep`` (Lock and Unlock overlapped and answered: the
    order Unlock-first raises, deep in the tree) behind one pending
    IsLocked."""
    return [(CRASHED, L("IsLocked"))] + tm.lock_deep(w, rounds)


def writes_only(n):
    """n pending Writes of n pids: n levels on the first path, ``lin`` with n nodes."""
    return [(i, L(("Write", 1 + i % 3))) for i in range(n)]


# name -> (model, history, events, status, nodes, states or None); the node
# count of the row over 2^64 is the u64 budget, its exact count in DEEP_EXACT
DEEP = {
    "crashed_reads_2x2_1": (tg.REGISTER, crashed_reads([2, 2], 1), 9, "nonlin", 27, None),
    "crashed_reads_3x2_2": (tg.REGISTER, crashed_reads([3, 3], 2), 14, "nonlin", 505, None),
    "crashed_reads_4x4_1": (tg.REGISTER, crashed_reads([4] * 4, 1), 33, "nonlin", 1179841, None),
    "crashed_reads_4x7_2": (tg.REGISTER, crashed_reads([4] * 7, 2), 58, "nonlin", 45873023044, None),
    "crashed_reads_8x3_2": (tg.REGISTER, crashed_reads([8] * 3, 2), 50, "nonlin", 311834861632804, 2552),
    "crashed_reads_1x24_4x9_2": (tg.REGISTER, crashed_reads([1] * 24 + [4] * 9, 2), 122, "nonlin",
                                 26422861285660, None),
    "crashed_reads_4x15_2": (tg.REGISTER, crashed_reads([4] * 15, 2), 122, "budget", U64, 872),
    "crashed_lin_deep_3_2": (tg.REGISTER, crashed_lin_deep(3, 2), 16, "lin", 255, None),
    "crashed_lin_deep_4_3": (tg.REGISTER, crashed_lin_deep(4, 3), 28, "lin", 75026, None),
    "crashed_lin_deep_4_7": (tg.REGISTER, crashed_lin_deep(4, 7), 60, "lin", 24891794818, None),
    "crashed_lock_3_2": (tg.LOCK, crashed_lock(3, 2), 14, "lin", 133, None),
    "crashed_lock_4_3": (tg.LOCK, crashed_lock(4, 3), 26, "lin", 27940, None),
    "crashed_lock_4_7": (tg.LOCK, crashed_lock(4, 7), 58, "lin", 9262894988, None),
    # derived with exact_count_pending (the two small error rows also with the literal rule)
    "crashed_lin_deep_4_8": (tg.REGISTER, crashed_lin_deep(4, 8), 68, "lin", 597403075614, 157),
    "crashed_lin_deep_4_12": (tg.REGISTER, crashed_lin_deep(4, 12), 100, "lin", 198204002814590606, 233),
    "crashed_lock_error_3_2": (tg.LOCK, crashed_lock_error(3, 2), 17, "error", 73, None),
    "crashed_lock_error_4_3": (tg.LOCK, crashed_lock_error(4, 3), 29, "error", 19460, None),
    "crashed_lock_error_4_7": (tg.LOCK, crashed_lock_error(4, 7), 61, "error", 6455957060, None),
}
DEEP_EXACT = {"crashed_reads_4x15_2": 5049487426087555352644}
# the rows the literal rule can walk
SMALL = ("crashed_reads_2x2_1", "crashed_reads_3x2_2", "crashed_lin_deep_3_2", "crashed_lin_deep_4_3",
         "crashed_lock_3_2", "crashed_lock_4_3", "crashed_lock_error_3_2", "crashed_lock_error_4_3")
