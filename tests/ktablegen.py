"""The product of K copies of one of tablegen's models, as closures: the
inputs of the keyed-table tests (qsmd.models.KeyedTableModel,
QSMD_MODEL_KTABLE).

TEST INFRASTRUCTURE ONLY.

``product(component, K)`` is a tablegen model dict whose states are K-tuples
of component states and whose invocations are ``(key, inv)``; responses are
the component's.  tablegen.gen_history / gen_batch and
oracle/linearise_lists.linearisable take it unchanged.

A response names no key, and the reference applies ``transition`` twice per
step (``transition (transition m (Left inv)) (Right resp)``,
src/Linearisability.hs:64), so the value between the two calls remembers the
invocation's key (``Mid``: a tuple that compares and hashes as the plain one).
Tabulating the product flat (``WideTableModel.from_closures``) identifies
such a value with the plain tuple, which is exact for a component whose
response transition is the identity -- every model of tablegen is one.
"""

from __future__ import annotations


class Mid(tuple):
    key = None


def _set(s, k, v):
    return s[:k] + (v,) + s[k + 1:]


def product(component, K):
    tr, post, real = component["transition"], component["postcondition"], component["real"]

    def transition(s, ev):
        kind, x = ev
        if kind == "L":
            k, i = x
            out = Mid(_set(s, k, tr(s[k], ("L", i))))
            out.key = k
            return out
        k = getattr(s, "key", None)
        return tuple(s) if k is None else _set(s, k, tr(s[k], ("R", x)))

    def postcondition(s, inv, resp):
        k, i = inv
        return post(s[k], i, resp)

    def real_(s, inv):
        k, i = inv
        v, resp = real(s[k], i)
        return _set(s, k, v), resp

    w = component.get("weights")
    return dict(name=f"{component['name']}^{K}", transition=transition, postcondition=postcondition,
                init=(component["init"],) * K, invs=[(k, i) for k in range(K) for i in component["invs"]],
                resps=list(component["resps"]), real=real_ if real else None,
                weights=None if w is None else list(w) * K)
