"""The explain calls' rule (include/qsmd.h qsmd_explain_batch), restated
literally over the reference's forest of interleavings.

TEST INFRASTRUCTURE ONLY.

``explain`` is oracle/linearise_lists.linearisable -- the same ``interleavings``
generators, the same ``step`` with its ``max_nodes`` rule (the budget is
checked before a node is counted), ``any'`` on the children -- which also
keeps, while it searches,

* the current path (the operations of the steps whose postcondition held and
  which have not been backtracked out of) and the model value at its end;
* the first path of maximal depth: a copy is taken whenever a descent makes
  the current path longer than every path before it, with the model value
  after that node's operation.

It returns ``(status, nodes, path, model)``:

  ``lin``              the witness (the current path at the leaf), the model there
  ``nonlin``, ``budget``   the first deepest path, the model after its last operation
                       (no operation passed: ``[]`` and ``model0``)
  ``error``            the current path when the postcondition raised (the path
                       to the parent of the raising step), the model there

``path`` is a list of operations ``(pid, inv, resp)``.  An empty history is
``("lin", 0, [], model0)``.
"""

from __future__ import annotations

import sys

from linearise_lists import BudgetExceeded, ModelError, interleavings


class _Rec:
    __slots__ = ("nodes", "max_nodes", "path", "models", "best", "best_model")

    def __init__(self, model0, max_nodes):
        self.nodes = 0
        self.max_nodes = max_nodes
        self.path = []
        self.models = [model0]          # models[d]: the model value at the end of path[:d]
        self.best = []
        self.best_model = model0


def _step(transition, postcondition, model, node, rec):
    """``step`` (src/Linearisability.hs:63-65) as linearise_lists._step, with the record."""
    if rec.max_nodes and rec.nodes >= rec.max_nodes:
        raise BudgetExceeded()
    rec.nodes += 1
    pid, inv, resp, es2 = node
    if not postcondition(model, inv, resp):
        return False
    model2 = transition(transition(model, ("L", inv)), ("R", resp))
    rec.path.append((pid, inv, resp))
    rec.models.append(model2)
    if len(rec.path) > len(rec.best):       # the first node of this depth
        rec.best = list(rec.path)
        rec.best_model = model2
    roses = interleavings(es2)
    first = next(roses, None)
    if first is None:
        return True
    if _step(transition, postcondition, model2, first, rec):
        return True
    for child in roses:
        if _step(transition, postcondition, model2, child, rec):
            return True
    rec.path.pop()
    rec.models.pop()
    return False


def explain(transition, postcondition, model0, es, max_nodes=0):
    rec = _Rec(model0, max_nodes)
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        if not es:
            return "lin", 0, [], model0
        for node in interleavings(es):
            if _step(transition, postcondition, model0, node, rec):
                return "lin", rec.nodes, list(rec.path), rec.models[-1]
        return "nonlin", rec.nodes, rec.best, rec.best_model
    except ModelError:
        return "error", rec.nodes, list(rec.path), rec.models[-1]
    except BudgetExceeded:
        return "budget", rec.nodes, rec.best, rec.best_model
    finally:
        sys.setrecursionlimit(old)


def explain_all(closures, hists, max_nodes=0, model0=None):
    """``explain`` for a tablegen model dict on every history."""
    init = closures["init"] if model0 is None else model0
    return [explain(closures["transition"], closures["postcondition"], init, list(h), max_nodes) for h in hists]


# The shapes of the parity tests (clients, operations, p_bug, histories):
# 3x10 and 4x16 fall in the 32-event class, 3 clients x 24 operations (48
# events) in the 64-event class, 2 x 40 and 3 x 40 (80 events) in the
# 128-event class.
SHAPES = {"3x10": (3, 10, 0.1, 256), "4x16": (4, 16, 0.03, 128), "3x24": (3, 24, 0.04, 64),
          "2x40": (2, 40, 0.05, 32), "3x40": (3, 40, 0.03, 16)}
ANYSHAPE = "anyshape"       # 64 bent histories of anyshape's "6x16" and 64 of its random family


def histories(closures, shape, seed="explain/1"):
    import random

    import anyshape as an
    import tablegen as tg
    if shape == ANYSHAPE:
        return an.batch(closures, "6x16", n=64, seed=seed) + an.batch(closures, an.RANDOM, n=64, seed=seed)
    c, k, p, n = SHAPES[shape]
    rng = random.Random(f"{seed}/{closures['name']}/{shape}")
    return [tg.gen_history(closures, rng, c, k, p) for _ in range(n)]
