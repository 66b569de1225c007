"""CPU references for the table path's exact-count state memo
(csrc/table.hip, knob "table_memo").

TEST INFRASTRUCTURE ONLY.

* :func:`exact_count` -- what the reference search returns (status and node
  count), computed without walking its tree: a memoised recursion over
  (remaining events, model state), plain ``any`` at the root and ``any'``
  below (src/Linearisability.hs:61, :67-69).  Independent of the kernel's
  bitset formulation: it removes events from a tuple the way ``filter1`` and
  ``findResponse`` do.
* :func:`memo_dfs` -- a literal mirror of ``TableLane::check_step`` (csrc/table_search.h) with the memo
  rule: Lemma L1 bitsets, one candidate per iteration, a lossy direct-mapped
  table of ``entries`` entries with the kernel's slot hash.
* the deep histories of the GPU tests (:func:`reads`, :func:`lin_deep`,
  :func:`lock_deep`) and the table of their known answers (:data:`DEEP`).

A model is a ``tablegen`` closure dict.
"""

from __future__ import annotations

import functools
import sys

import tablegen as tg
from linearise_lists import ModelError

U64 = (1 << 64) - 1
L, R = tg.L, tg.R


# ---------------------------------------------------------------------------
# exact_count
# ---------------------------------------------------------------------------

def _children(hist, es):
    """``interleavings`` on a tuple of event indices: (j, r, es') per child."""
    out = []
    for j in es:
        pid, (kind, _) = hist[j]
        if kind != "L":
            break                                        # takeInvocations
        first_inv = next(k for k in es if hist[k][0] == pid and hist[k][1][0] == "L")   # filter1
        es1 = tuple(k for k in es if k != first_inv)
        r = next((k for k in es1 if hist[k][0] == pid and hist[k][1][0] == "R"), None)  # findResponse
        if r is not None:
            out.append((j, r, tuple(k for k in es1 if k != r)))
    return out


def exact_count(model, hist, max_nodes=0, stats=None):
    """(status, nodes) of the reference search of ``hist``; with a limit
    smaller than the total, ("budget", max_nodes).  ``stats`` (a dict)
    receives "states": the distinct (remaining events, state) keys met."""
    tr, post = model["transition"], model["postcondition"]
    memo = {}

    def forest(es, state, root):
        """(outcome, nodes counted) of any / any' over the children of a node:
        outcome True (a success), False (every child failed) or "error"."""
        key = (es, state)
        if key in memo:
            return memo[key]
        kids = _children(hist, es)
        if not kids:
            res = (not root, 0)                          # any' [] = True, any [] = False
        else:
            n, res = 0, None
            for j, r, es2 in kids:
                n += 1                                   # step evaluated
                inv, resp = hist[j][1][1], hist[r][1][1]
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
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        out, n = forest(tuple(range(len(hist))), model["init"], True)
    finally:
        sys.setrecursionlimit(old)
    if stats is not None:
        stats["states"] = len(memo)
    if max_nodes and n > max_nodes:
        return "budget", max_nodes
    return {True: "lin", False: "nonlin", "error": "error"}[out], n


# ---------------------------------------------------------------------------
# memo_dfs: TableLane::check_step, literally
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _table(name):
    from qsmd.models import TableModel
    m = {"register": tg.REGISTER, "lock": tg.LOCK}[name]
    return TableModel.from_closures(m["transition"], m["postcondition"], m["init"], m["invs"], m["resps"],
                                    raises=ModelError)


HASH_K = (0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F)


def memo_slot(rem, n_words, state, entries):
    """The kernel's slot hash (table_search.h TableMemo::slot_of)."""
    x = (state * 0x165667B1) & 0xFFFFFFFF
    for k in range(n_words):
        x ^= (((rem >> (32 * k)) & 0xFFFFFFFF) * HASH_K[k]) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    return x & (entries - 1)


def _ctz(x):
    return (x & -x).bit_length() - 1


def memo_dfs(model, hist, entries, max_nodes, info=None):
    """(status, nodes, path) as the kernel's memo pass computes them;
    ``entries`` 0 is the plain search.  ``info`` (a dict) receives
    "iterations" and "hits"."""
    t = _table(model["name"])
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
    limit = max_nodes if max_nodes else U64

    def cands(rem):
        rr, c = rem & RESP, rem & INV
        return c & ((1 << _ctz(rr)) - 1) if rr else c

    def topbit(x):
        return 1 << (x.bit_length() - 1) if x else 0

    rem = INV | RESP
    cand = cands(rem)
    state, depth, found, nodes = t.init_state, 0, 0, 0
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
                table[memo_slot(rem, n_words, state, entries)] = (rem, state, nodes - entry[depth])
            skip = False
            j, state = stk[depth]
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
        ok = (int(t.post[state, i]) >> rc) & 1
        err = (int(t.post_err[state, i]) >> rc) & 1 if t.post_err is not None else 0
        nodes += 1
        found = 1
        if err:
            status = "error"
            break
        if ok:
            stk[depth] = (j, state)
            depth += 1
            state = int(t.on_resp[int(t.on_inv[state, i]), rc])
            lowest_inv = (rem & pmj & INV) & -(rem & pmj & INV)
            rem &= ~(lowest_inv | (1 << r))
            cand = cands(rem)
            found = 0
            if entries:
                entry[depth - 1] = nodes
                e = table[memo_slot(rem, n_words, state, entries)]
                if e is not None and e[0] == rem and e[1] == state:
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


# ---------------------------------------------------------------------------
# deep histories
# ---------------------------------------------------------------------------

def reads(widths):
    """Register: per round of width w, w overlapping reads answered Val 0;
    the very last answer is Val 1 (no order explains it)."""
    h = []
    for w in widths:
        h += [(p, L("Read")) for p in range(w)] + [(p, R(("Val", 0))) for p in range(w)]
    h[-1] = (h[-1][0], R(("Val", 1)))
    return h


def lin_deep(w, rounds):
    """Register: two overlapping writes, then rounds of w overlapping failing
    Cas, then a Read of 0 -- linearisable only with Write 1 before Write 0."""
    h = [(0, L(("Write", 0))), (1, L(("Write", 1))), (0, R("Ok")), (1, R("Ok"))]
    for _ in range(rounds):
        h += [(p, L(("Cas", 3, 3))) for p in range(w)] + [(p, R("CasFail")) for p in range(w)]
    return h + [(0, L("Read")), (0, R(("Val", 0)))]


def lock_deep(w, rounds):
    """Lock: Lock and Unlock overlapped, then rounds of w IsLocked answered
    No, the very last Yes: the order Unlock-first raises."""
    h = [(0, L("Lock")), (1, L("Unlock")), (0, R("Ok")), (1, R("Ok"))]
    for _ in range(rounds):
        h += [(p, L("IsLocked")) for p in range(w)] + [(p, R("No")) for p in range(w)]
    h[-1] = (h[-1][0], R("Yes"))
    return h


# name -> (model, history, events, status, nodes, states or None); the node
# count of the row over 2^64 is the u64 budget, its exact count in DEEP_EXACT
DEEP = {
    "reads_4x4": (tg.REGISTER, reads([4] * 4), 32, "nonlin", 467008, 53),
    "reads_4x8": (tg.REGISTER, reads([4] * 8), 64, "nonlin", 154942969408, 113),
    "reads_8x4": (tg.REGISTER, reads([8] * 4), 64, "nonlin", 1796136622124653600, 893),
    "reads_1x24_4x10": (tg.REGISTER, reads([1] * 24 + [4] * 10), 128, "nonlin", 89247150380632, 167),
    "reads_4x16": (tg.REGISTER, reads([4] * 16), 128, "budget", U64, 233),
    "lin_deep_4_3": (tg.REGISTER, lin_deep(4, 3), 30, "lin", 52305, 63),
    "lin_deep_4_7": (tg.REGISTER, lin_deep(4, 7), 62, "lin", 17348826721, 139),
    "lin_deep_4_9": (tg.REGISTER, lin_deep(4, 9), 78, "lin", 9992924173929, 177),
    "lock_deep_3_2": (tg.LOCK, lock_deep(3, 2), 16, "error", 72, None),
    "lock_deep_4_3": (tg.LOCK, lock_deep(4, 3), 28, "error", 19459, None),
    "lock_deep_4_7": (tg.LOCK, lock_deep(4, 7), 60, "error", 6455957059, None),
    "lock_deep_4_9": (tg.LOCK, lock_deep(4, 9), 76, "error", 3718631265859, None),
}
DEEP_EXACT = {"reads_4x16": 17055396037254253254208}
