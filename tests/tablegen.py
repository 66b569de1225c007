"""Finite-state models as closures (the shape the reference's `linearisable`
takes, src/Linearisability.hs:52-58) and a history generator for them: the
inputs of the table-model tests (qsmd.models.TableModel, QSMD_MODEL_TABLE).

TEST INFRASTRUCTURE ONLY.

Each model is a dict: ``transition``, ``postcondition``, ``init``, ``invs``,
``resps`` (the symbol lists, in table order) and ``real(state, inv) ->
(state', resp)``, the system the generator runs.
"""

from __future__ import annotations

import random

from linearise_lists import ModelError

L = lambda x: ("L", x)  # noqa: E731
R = lambda x: ("R", x)  # noqa: E731

# ---------------------------------------------------------------------------
# Register: values 0..3, Write v / Read / Cas a b (21 invocations),
# Ok / Val v / CasOk / CasFail (7 responses)
# ---------------------------------------------------------------------------

REG_VALUES = (0, 1, 2, 3)
REG_INVS = ([("Write", v) for v in REG_VALUES] + ["Read"] +
            [("Cas", a, b) for a in REG_VALUES for b in REG_VALUES])
REG_RESPS = ["Ok"] + [("Val", v) for v in REG_VALUES] + ["CasOk", "CasFail"]


def reg_transition(m, ev):
    kind, x = ev
    if kind == "R" or x == "Read":
        return m
    if x[0] == "Write":
        return x[1]
    return x[2] if m == x[1] else m           # Cas a b


def reg_postcondition(m, inv, resp):
    if inv == "Read":
        return resp == ("Val", m)
    if inv[0] == "Write":
        return resp == "Ok"
    return resp == ("CasOk" if m == inv[1] else "CasFail")


def reg_real(m, inv):
    if inv == "Read":
        return m, ("Val", m)
    if inv[0] == "Write":
        return inv[1], "Ok"
    return (inv[2], "CasOk") if m == inv[1] else (m, "CasFail")


REGISTER = dict(name="register", transition=reg_transition, postcondition=reg_postcondition, init=0,
                invs=REG_INVS, resps=REG_RESPS, real=reg_real)

# ---------------------------------------------------------------------------
# Lock: a try-lock.  Unlock on an unlocked lock has no meaning in the model:
# its postcondition raises (post_err).
# ---------------------------------------------------------------------------

LOCK_INVS = ["Lock", "Unlock", "IsLocked"]
LOCK_RESPS = ["Ok", "Busy", "Yes", "No"]


def lock_transition(m, ev):
    kind, x = ev
    if kind == "R" or x == "IsLocked":
        return m
    return x == "Lock"


def lock_postcondition(m, inv, resp):
    if inv == "Lock":
        return resp == ("Busy" if m else "Ok")
    if inv == "IsLocked":
        return resp == ("Yes" if m else "No")
    if not m:
        raise ModelError("Unlock of an unlocked lock")
    return resp == "Ok"


def lock_real(m, inv):
    if inv == "Lock":
        return True, ("Busy" if m else "Ok")
    if inv == "IsLocked":
        return m, ("Yes" if m else "No")
    return False, "Ok"


# (Unlock dealt rarely: most generated histories should get past it)
LOCK = dict(name="lock", transition=lock_transition, postcondition=lock_postcondition, init=False,
            invs=LOCK_INVS, resps=LOCK_RESPS, real=lock_real, weights=[6, 1, 6])

# ---------------------------------------------------------------------------
# TicketDispenser (test/TicketDispenser.hs:81-102) as a finite-state model:
# Nothing, Just 0..K and a sink (Just n beyond K, which a history of at most K
# operations from Nothing never reaches); `Number i` is symbol i for i in
# 1..K+1, every other value one junk symbol (it matches no state).
# ---------------------------------------------------------------------------

SINK = "sink"


def ticket_closures(K):
    invs = ["TakeTicket", "Reset"]
    resps = ["Ok"] + [("Number", i) for i in range(1, K + 2)] + ["Junk"]

    def transition(m, ev):
        kind, x = ev
        if kind == "R":
            return m
        if x == "Reset":
            return 0
        if m is None or m == SINK:
            return m
        return m + 1 if m < K else SINK

    def postcondition(m, inv, resp):
        if inv == "TakeTicket" and isinstance(resp, tuple):
            return m is not None and m != SINK and resp[1] == m + 1
        return inv == "Reset" and resp == "Ok"

    return dict(name=f"ticket{K}", transition=transition, postcondition=postcondition, init=None,
                invs=invs, resps=resps, real=None)


def ticket_symbols(history, K):
    """A TicketDispenser history (oracle / kats shapes) in the ticket table's
    symbols."""
    out = []
    for pid, (kind, x) in history:
        if kind == "R" and isinstance(x, tuple):
            x = x if 1 <= x[1] <= K + 1 else "Junk"
        out.append((pid, (kind, x)))
    return out


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------

def gen_history(model, rng, n_clients, n_ops, p_bug):
    """K operations dealt to C client programs; at each tick a client with a
    deliverable event, picked uniformly, delivers its next invocation (the
    operation is applied to the real state then, its response remembered) or,
    with one pending, the remembered response.  With probability p_bug per
    operation the response is replaced by a random symbol."""
    programs = [[] for _ in range(n_clients)]
    for _ in range(n_ops):
        programs[rng.randrange(n_clients)].append(rng.choices(model["invs"], model.get("weights"))[0])
    state = model["init"]
    pending = [None] * n_clients
    pos = [0] * n_clients
    hist = []
    while True:
        ready = [c for c in range(n_clients) if pending[c] is not None or pos[c] < len(programs[c])]
        if not ready:
            return hist
        c = rng.choice(ready)
        if pending[c] is None:
            inv = programs[c][pos[c]]
            pos[c] += 1
            state, resp = model["real"](state, inv)
            if rng.random() < p_bug:
                resp = rng.choice(model["resps"])
            pending[c] = (resp,)
            hist.append((c, L(inv)))
        else:
            hist.append((c, R(pending[c][0])))
            pending[c] = None


# (clients, operations, p_bug, histories): the settings of the parity tests
SETTINGS = {"4x16": (4, 16, 0.03, 2000), "6x24": (6, 24, 0.03, 500), "3x10": (3, 10, 0.1, 2000)}
SEED = 1234
MAX_NODES = 20000


def gen_batch(model, setting, n=None, seed=SEED):
    c, k, p, n0 = SETTINGS[setting]
    rng = random.Random(f"{seed}/{model['name']}/{setting}")
    return [gen_history(model, rng, c, k, p) for _ in range(n0 if n is None else n)]
