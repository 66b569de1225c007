"""The keyed-table-model generator's stream (include/qsmd_gen.h,
"keyed-table-model generator") restated on Python integers: what
qsmd_gen_ktable_batch and the device kernel must emit, byte for byte.

TEST INFRASTRUCTURE ONLY.  Written from the header's definition, not from
either implementation: a list of component states, a list of (key, inv)
pairs with their weights, plain lists for the schedule.  The RNG and the
component's acc(s, i) are tablegen_ref's.  ``COUNTERS`` records which parts
of the definition a run reached.
"""

from __future__ import annotations

import collections

import numpy as np

from qsmd import codec
from tablegen_ref import PID_SHARED, LIN_AT_INVOKE, Rng, Tables

COUNTERS = collections.Counter()


class KTables:
    """The component's tables and the pairs' weights, key-major."""

    def __init__(self, model, inv_weight=None, key_weight=None):
        self.c = Tables(model.component)
        self.n_keys, self.n_inv, self.n_resp = model.n_keys, self.c.n_inv, self.c.n_resp
        iw = [1] * self.n_inv if inv_weight is None else [int(x) for x in inv_weight]
        kw = [1] * self.n_keys if key_weight is None else [int(x) for x in key_weight]
        assert len(iw) == self.n_inv and len(kw) == self.n_keys
        self.pairs = [(k, i) for k in range(self.n_keys) for i in range(self.n_inv)]
        self.weight = [kw[k] * iw[i] for k, i in self.pairs]
        self.unit = all(x <= 1 for x in iw + kw)


def _request(t, r, s):
    COUNTERS["unit_pick" if t.unit else "general_scan"] += 1
    en = [w > 0 and t.c.acc(s[k], i) != 0 for (k, i), w in zip(t.pairs, t.weight)]
    W = sum(w for w, e in zip(t.weight, en) if e)
    if W == 0:
        COUNTERS["fallback"] += 1
        en = [w > 0 for w in t.weight]
        W = sum(t.weight)
    if W == 256 and t.unit:         # eight keys' 32 invocations, all enabled: the most a unit-weight draw spans
        COUNTERS["w256"] += 1
    x, run = r.below(W), 0
    for pair, w, e in zip(t.pairs, t.weight, en):
        if e:
            run += w
            if run > x:
                COUNTERS["key", pair[0]] += 1
                return pair
    raise AssertionError("request: no invocation")


def _execute(t, r, s, pair, flags):
    k, i = pair
    a = t.c.acc(s[k], i)
    if a:
        x = [b for b in range(t.n_resp) if (a >> b) & 1][r.below(bin(a).count("1"))]
    else:
        x = r.below(t.n_resp)
        flags[0] |= 2
        COUNTERS["stuck"] += 1
    s[k] = int(t.c.on_resp[int(t.c.on_inv[s[k], i]), x])
    return x


def gen_one(t, index, *, n_clients, n_ops, prefix_ops=0, lin_policy=0, pid_mode=0, overlap=0, p_bug=0.0, seed=0):
    """Events [(kp, code, a)] and the flag byte of history `index`."""
    r = Rng(seed, index)
    C, K = n_clients, n_ops
    P = min(prefix_ops, K)
    S = K - P
    ov = overlap if overlap else C
    pid = (lambda c: 0) if pid_mode == PID_SHARED else (lambda c: c)
    s, flags, ev = [t.c.init] * t.n_keys, [0], []
    for _ in range(P):
        c = r.below(C)
        k, i = pair = _request(t, r, s)
        x = _execute(t, r, s, pair, flags)
        ev.append((pid(c), i, k))
        ev.append((0x80 | pid(c), x, 0))
    queued = [0] * C
    for _ in range(S):
        queued[r.below(C)] += 1
    IDLE, INVOKED, EXECUTED = 0, 1, 2
    phase, inv, resp = [IDLE] * C, [None] * C, [0] * C
    outstanding = done = 0
    while done < S:
        may_send = outstanding < ov
        ready = [c for c in range(C) if phase[c] != IDLE or (may_send and queued[c] > 0)]
        c = ready[r.below(len(ready))]
        if phase[c] == IDLE:
            inv[c] = _request(t, r, s)
            ev.append((pid(c), inv[c][1], inv[c][0]))
            queued[c] -= 1
            outstanding += 1
            if lin_policy == LIN_AT_INVOKE:
                resp[c] = _execute(t, r, s, inv[c], flags)
                phase[c] = EXECUTED
            else:
                phase[c] = INVOKED
        elif phase[c] == INVOKED:
            resp[c] = _execute(t, r, s, inv[c], flags)
            phase[c] = EXECUTED
        else:
            ev.append((0x80 | pid(c), resp[c], 0))
            phase[c] = IDLE
            outstanding -= 1
            done += 1
    if p_bug > 0:
        u = r.unit()
        if u < p_bug and S >= 1:
            at = [e for e in range(2 * P, len(ev)) if ev[e][0] & 0x80]
            assert len(at) == S
            nr = t.n_resp
            coin = r.below(2) if nr >= 2 and S >= 2 else 0
            if nr >= 2 and (S < 2 or coin == 0):
                e = at[r.below(S)]
                d = r.below(nr - 1)
                ev[e] = (ev[e][0], (ev[e][1] + 1 + d) % nr, 0)
                flags[0] |= 1
                COUNTERS["bug_change"] += 1
            elif S >= 2:
                k1 = r.below(S)
                k2 = r.below(S)
                if k2 == k1:
                    k2 = (k1 + 1) % S
                e1, e2 = at[k1], at[k2]
                ev[e1], ev[e2] = (ev[e1][0], ev[e2][1], 0), (ev[e2][0], ev[e1][1], 0)
                flags[0] |= 1
                COUNTERS["bug_swap"] += 1
            else:
                COUNTERS["bug_noop"] += 1
    return ev, flags[0]


def generate(model, first, n_hist, ev_base=0, inv_weight=None, key_weight=None, **kw):
    """(hdr, events, flags) numpy arrays, as qsmd.gen.generate_ktable returns
    them, for histories [first, first + n_hist)."""
    t = KTables(model, inv_weight, key_weight)
    per = 2 * kw["n_ops"]
    hdr = np.zeros(n_hist, dtype=codec.HDR_DTYPE)
    events = np.zeros(n_hist * per, dtype=codec.EV_DTYPE)
    flags = np.zeros(n_hist, dtype=np.uint8)
    n_pid = 1 if kw.get("pid_mode", 0) == PID_SHARED else kw["n_clients"]
    for i in range(n_hist):
        ev, f = gen_one(t, first + i, **kw)
        assert len(ev) == per
        hdr[i] = (ev_base + i * per, per, n_pid, 5, (first + i) & 0xFFFFFFFF, 0)
        events["kp"][i * per:(i + 1) * per] = [e[0] for e in ev]
        events["code"][i * per:(i + 1) * per] = [e[1] for e in ev]
        events["a"][i * per:(i + 1) * per] = [e[2] for e in ev]
        flags[i] = f
    return hdr, events, flags
