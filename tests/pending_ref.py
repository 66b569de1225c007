"""The search that lets pending invocations take effect
(qsmd_check_pending_batch), restated literally on lists.

TEST INFRASTRUCTURE ONLY.

It is ``oracle/linearise_lists.py``'s search -- the same ``take_invocations``,
``filter1`` and ``find_response``, the same node counter and ``max_nodes``
test as ``_step`` -- with two changes:

    interleavings(m, es) = for (pid, inv) in takeInvocations es:
        es1 = filter1 (not . matchInvocation pid) es
        case findResponse pid es1 of
          [(resp, es2)] -> child (pid, inv, resp, es2, observed)
          []            -> for r in resps, post m inv r holds and does not raise:
                             child (pid, inv, r, es1, assumed)
    step m child = count a node; observed: postcondition m inv resp && ...; assumed: no test

and a non-empty history without any response event whose root has no child is
linearisable with 0 nodes.  A model is a ``tablegen``-style closure dict
(``transition``, ``postcondition``, ``init``, ``resps``).
"""

from __future__ import annotations

import sys

from linearise_lists import (BudgetExceeded, ModelError, _Counter, filter1, find_response, take_invocations)


def allowed(model, m, inv):
    """The response symbols, in table order, whose postcondition holds at
    ``m`` for ``inv`` and does not raise."""
    out = []
    for r in model["resps"]:
        try:
            if model["postcondition"](m, inv, r):
                out.append(r)
        except ModelError:
            pass
    return out


def interleavings(model, m, es):
    """Yields ``(pid, inv, resp, es', assumed)``; the subforest of a child is
    ``interleavings(model, m', es')``."""
    if not es:
        return
    for pid, inv in take_invocations(es):
        def not_match_invocation(e, pid=pid):
            return not (e[0] == pid and e[1][0] == "L")
        es1 = filter1(not_match_invocation, es)
        found = find_response(pid, es1)
        if found:
            resp, es2 = found[0]
            yield (pid, inv, resp, es2, False)
        else:
            for r in allowed(model, m, inv):
                yield (pid, inv, r, es1, True)


def _step(model, m, node, ctr):
    if ctr.max_nodes and ctr.nodes >= ctr.max_nodes:
        raise BudgetExceeded()
    ctr.nodes += 1
    pid, inv, resp, es2, assumed = node
    if not assumed and not model["postcondition"](m, inv, resp):
        return False
    tr = model["transition"]
    m2 = tr(tr(m, ("L", inv)), ("R", resp))
    ctr.path.append((pid, inv, resp, assumed))
    roses = interleavings(model, m2, es2)
    first = next(roses, None)
    if first is None:                               # any' _ [] = True
        return True
    if _step(model, m2, first, ctr):
        return True
    for child in roses:
        if _step(model, m2, child, ctr):
            return True
    ctr.path.pop()
    return False


def linearisable_pending(model, es, max_nodes=0, model0=None):
    """``(status, nodes, path)``: status as ``linearise_lists.linearisable``,
    path the operations ``(pid, inv, resp, assumed)`` of the linearisation."""
    ctr = _Counter(max_nodes)
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    init = model["init"] if model0 is None else model0
    try:
        if not es:
            return "lin", 0, []
        children = 0
        for node in interleavings(model, init, es):
            children += 1
            if _step(model, init, node, ctr):
                return "lin", ctr.nodes, list(ctr.path)
        if children == 0 and not any(ev[0] == "R" for _, ev in es):
            return "lin", 0, []                     # nothing was observed: every operation dropped
        return "nonlin", ctr.nodes, []
    except ModelError:
        return "error", ctr.nodes, []
    except BudgetExceeded:
        return "budget", ctr.nodes, []
    finally:
        sys.setrecursionlimit(old)


def crash(history, rng, p):
    """Per client with probability ``p``, one of its responses (drawn
    uniformly) and everything that client does after it disappear."""
    out = list(history)
    for pid in sorted({q for q, _ in history}):
        if rng.random() >= p:
            continue
        resps = [k for k, (q, ev) in enumerate(out) if q == pid and ev[0] == "R"]
        if not resps:
            continue
        cut = rng.choice(resps)
        out = [e for k, e in enumerate(out) if not (e[0] == pid and k >= cut)]
    return out


def pending_invocations(history):
    """The indices of the invocations that never get a response: per pid, the
    invocations beyond its number of responses."""
    n_resp, seen, out = {}, {}, []
    for pid, ev in history:
        if ev[0] == "R":
            n_resp[pid] = n_resp.get(pid, 0) + 1
    # (a well-formed client history: the k-th response answers the k-th invocation)
    for k, (pid, ev) in enumerate(history):
        if ev[0] == "L":
            seen[pid] = seen.get(pid, 0) + 1
            if seen[pid] > n_resp.get(pid, 0):
                out.append(k)
    return out


def witness_ops(model_resps, hist, wit, assumed):
    """The operations ``(pid, inv, resp, assumed)`` a device witness names:
    ``assumed[d]`` None for an observed level (the pid's first remaining
    response, removed), else the index of the assumed symbol (only the pid's
    first remaining invocation is removed)."""
    removed, path = set(), []
    for j, a in zip(wit, assumed):
        pid, (_, inv) = hist[j]
        i0 = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "L" and p == pid)
        removed.add(i0)
        if a is None:
            r = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "R" and p == pid)
            removed.add(r)
            path.append((pid, inv, hist[r][1][1], False))
        else:
            path.append((pid, inv, model_resps[a], True))
    return path
