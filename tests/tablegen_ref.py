"""The table-model generator's stream (include/qsmd_gen.h, "table-model
generator") restated on Python integers masked to 64 bits: what
qsmd_gen_table_batch and the device kernel must emit, byte for byte.

TEST INFRASTRUCTURE ONLY.  Written from the header's definition, not from
either implementation: no masks of ready clients, no staged events -- the
plain lists the definition speaks of.
"""

from __future__ import annotations

import numpy as np

from qsmd import codec

M64 = (1 << 64) - 1
LIN_AT_INVOKE, LIN_IN_WINDOW = 0, 1
PID_PER_CLIENT, PID_SHARED = 0, 1


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return x, z ^ (z >> 31)


def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & M64


class Rng:
    def __init__(self, seed, index):
        x = (seed ^ (index * 0xD1B54A32D192ED03)) & M64
        self.s = []
        for _ in range(4):
            x, z = _splitmix(x)
            self.s.append(z)

    def next(self):
        s = self.s
        r = (_rotl((s[1] * 5) & M64, 7) * 9) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 45)
        return r

    def below(self, n):
        return (((self.next() >> 32) * n) >> 32) if n else 0

    def unit(self):
        return (self.next() >> 11) * 2.0 ** -53


class Tables:
    """acc(s, i) as one Python int per entry, computed on first use."""

    def __init__(self, model):
        self.m = model
        self.n_states, self.n_inv, self.n_resp = len(model.states), len(model.invs), len(model.resps)
        self.init = model.init_state
        self.on_inv = model.on_inv
        self.on_resp = model.on_resp
        self._acc = {}
        self._req = {}
        self._mask = (1 << self.n_resp) - 1

    def acc(self, s, i):
        a = self._acc.get((s, i))
        if a is None:
            post, err = self.m.post[s, i], None if self.m.post_err is None else self.m.post_err[s, i]
            words = np.atleast_1d(post)
            a = sum(int(w) << (32 * k) for k, w in enumerate(words))
            if err is not None:
                a &= ~sum(int(w) << (32 * k) for k, w in enumerate(np.atleast_1d(err)))
            a &= self._mask
            self._acc[(s, i)] = a
        return a


def _request(t, w, r, s):
    # the enabled invocations of a state depend on (weights, state) only: kept
    key = (s, w)
    hit = t._req.get(key)
    if hit is None:
        en = [w[i] > 0 and t.acc(s, i) != 0 for i in range(t.n_inv)]
        W = sum(w[i] for i in range(t.n_inv) if en[i])
        if W == 0:
            en = [x > 0 for x in w]
            W = sum(w)
        hit = t._req[key] = (en, W)
    en, W = hit
    x, run = r.below(W), 0
    for i in range(t.n_inv):
        if en[i]:
            run += w[i]
            if run > x:
                return i
    raise AssertionError("request: no invocation")


def _execute(t, r, s, i, flags):
    a = t.acc(s, i)
    if a:
        k = r.below(bin(a).count("1"))
        x = [b for b in range(t.n_resp) if (a >> b) & 1][k]
    else:
        x = r.below(t.n_resp)
        flags[0] |= 2
    return int(t.on_resp[int(t.on_inv[s, i]), x]), x


def gen_one(t, w, index, *, n_clients, n_ops, prefix_ops=0, lin_policy=0, pid_mode=0, overlap=0, p_bug=0.0,
            seed=0):
    """Events [(kp, code)] and the flag byte of history `index`."""
    r = Rng(seed, index)
    C, K = n_clients, n_ops
    P = min(prefix_ops, K)
    S = K - P
    ov = overlap if overlap else C
    pid = (lambda c: 0) if pid_mode == PID_SHARED else (lambda c: c)
    s, flags, ev = t.init, [0], []
    for _ in range(P):
        c = r.below(C)
        i = _request(t, w, r, s)
        s, x = _execute(t, r, s, i, flags)
        ev.append((pid(c), i))
        ev.append((0x80 | pid(c), x))
    queued = [0] * C
    for _ in range(S):
        queued[r.below(C)] += 1
    IDLE, INVOKED, EXECUTED = 0, 1, 2
    phase, inv, resp = [IDLE] * C, [0] * C, [0] * C
    outstanding = done = 0
    while done < S:
        # the ready actions, client 0 first: a client has at most one (send when
        # idle, execute when invoked, respond when executed)
        may_send = outstanding < ov
        ready = [c for c in range(C) if phase[c] != IDLE or (may_send and queued[c] > 0)]
        c = ready[r.below(len(ready))]
        if phase[c] == IDLE:
            inv[c] = _request(t, w, r, s)
            ev.append((pid(c), inv[c]))
            queued[c] -= 1
            outstanding += 1
            if lin_policy == LIN_AT_INVOKE:
                s, resp[c] = _execute(t, r, s, inv[c], flags)
                phase[c] = EXECUTED
            else:
                phase[c] = INVOKED
        elif phase[c] == INVOKED:
            s, resp[c] = _execute(t, r, s, inv[c], flags)
            phase[c] = EXECUTED
        else:
            ev.append((0x80 | pid(c), resp[c]))
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
                ev[e] = (ev[e][0], (ev[e][1] + 1 + d) % nr)
                flags[0] |= 1
            elif S >= 2:
                k1 = r.below(S)
                k2 = r.below(S)
                if k2 == k1:
                    k2 = (k1 + 1) % S
                e1, e2 = at[k1], at[k2]
                ev[e1], ev[e2] = (ev[e1][0], ev[e2][1]), (ev[e2][0], ev[e1][1])
                flags[0] |= 1
    return ev, flags[0]


def generate(model, first, n_hist, ev_base=0, inv_weight=None, tables=None, **kw):
    """(hdr, events, flags) numpy arrays, as qsmd.gen.generate_table returns
    them, for histories [first, first + n_hist)."""
    t = tables or Tables(model)
    w = tuple([1] * t.n_inv if inv_weight is None else [int(x) for x in inv_weight])
    per = 2 * kw["n_ops"]
    hdr = np.zeros(n_hist, dtype=codec.HDR_DTYPE)
    events = np.zeros(n_hist * per, dtype=codec.EV_DTYPE)
    flags = np.zeros(n_hist, dtype=np.uint8)
    n_pid = 1 if kw.get("pid_mode", 0) == PID_SHARED else kw["n_clients"]
    for i in range(n_hist):
        ev, f = gen_one(t, w, first + i, **kw)
        assert len(ev) == per
        hdr[i] = (ev_base + i * per, per, n_pid, model.model_id, (first + i) & 0xFFFFFFFF, 0)
        events["kp"][i * per:(i + 1) * per] = [e[0] for e in ev]
        events["code"][i * per:(i + 1) * per] = [e[1] for e in ev]
        flags[i] = f
    return hdr, events, flags
