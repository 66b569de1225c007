"""Finite-state models beyond the narrow table's limits (256 states, 32
symbols): the inputs of the wide-table tests (qsmd.models.WideTableModel,
QSMD_MODEL_WTABLE).

TEST INFRASTRUCTURE ONLY.

Each model is a closure dict in the shape of ``tablegen.REGISTER`` (``name``,
``transition``, ``postcondition``, ``init``, ``invs``, ``resps``, ``real``), so
``tablegen.gen_history`` / ``gen_batch``, the literal oracle and
``tablememo.exact_count`` work on them unchanged; :func:`wide_table` is the
model's :class:`WideTableModel`.
"""

from __future__ import annotations

import functools
import random

import numpy as np

import tablegen as tg
from linearise_lists import ModelError

L, R = tg.L, tg.R

# ---------------------------------------------------------------------------
# KV: 5 keys over 4 values.  1,024 states, 105 invocations (Write k v: 20,
# Read k: 5, Cas k old new: 80), 6 responses.  No raising postcondition.
# ---------------------------------------------------------------------------

KV_KEYS = range(5)
KV_VALUES = range(4)
KV_INVS = ([("Write", k, v) for k in KV_KEYS for v in KV_VALUES] + [("Read", k) for k in KV_KEYS] +
           [("Cas", k, a, b) for k in KV_KEYS for a in KV_VALUES for b in KV_VALUES])
KV_RESPS = ["Ok"] + [("Val", v) for v in KV_VALUES] + ["Fail"]


def _kv_set(m, k, v):
    return m[:k] + (v,) + m[k + 1:]


def kv_real(m, inv):
    op, k = inv[0], inv[1]
    if op == "Read":
        return m, ("Val", m[k])
    if op == "Write":
        return _kv_set(m, k, inv[2]), "Ok"
    return (_kv_set(m, k, inv[3]), "Ok") if m[k] == inv[2] else (m, "Fail")


def kv_transition(m, ev):
    kind, x = ev
    return m if kind == "R" else kv_real(m, x)[0]


def kv_postcondition(m, inv, resp):
    return resp == kv_real(m, inv)[1]


KV = dict(name="kv", transition=kv_transition, postcondition=kv_postcondition, init=(0,) * 5,
          invs=KV_INVS, resps=KV_RESPS, real=kv_real)

# ---------------------------------------------------------------------------
# WCOUNTER: states 0..299, `add i` for i in 0..255, responses 0..255.
#   post: r == (s + i) % 256; raises when s % 64 == 63 and i == 0;
#   next state (s + i) % 300.
# Response codes above 31 land in post words 1..7.  (add 0, add 1 and add 63
# dealt often: the generated histories then meet the raising states and hold
# many commuting operations.)
# ---------------------------------------------------------------------------

WC_STATES, WC_SYMS = 300, 256


def wc_transition(s, ev):
    return (s + ev[1]) % WC_STATES if ev[0] == "L" else s


def wc_postcondition(s, i, r):
    if s % 64 == 63 and i == 0:
        raise ModelError("wcounter at 63 mod 64")
    return r == (s + i) % 256


def wc_real(s, i):
    return (s + i) % WC_STATES, (s + i) % 256


WCOUNTER = dict(name="wcounter", transition=wc_transition, postcondition=wc_postcondition, init=0,
                invs=list(range(WC_SYMS)), resps=list(range(WC_SYMS)), real=wc_real,
                weights=[600, 60] + [1] * 61 + [25] + [1] * (WC_SYMS - 64))

# ---------------------------------------------------------------------------
# BIG: a mod-65536 counter, `add 0` / `add 1`; the response is the top bit of
# the new state xor its low bit.  From 65535 a step wraps to 0.
# ---------------------------------------------------------------------------

BIG_STATES = 65536


def _big_resp(t):
    return ((t >> 15) ^ t) & 1


def big_real(s, i):
    t = (s + i) % BIG_STATES
    return t, _big_resp(t)


def big_transition(s, ev):
    return (s + ev[1]) % BIG_STATES if ev[0] == "L" else s


def big_postcondition(s, i, r):
    return r == _big_resp((s + i) % BIG_STATES)


BIG = dict(name="big", transition=big_transition, postcondition=big_postcondition, init=0,
           invs=[0, 1], resps=[0, 1], real=big_real)

# ---------------------------------------------------------------------------
# REG512: a register over the values 0..511 with a few symbols: Write v for v
# in REG512_VALUES (each value with its twin v + 256: equal in the low eight
# bits) and Read.
# ---------------------------------------------------------------------------

REG512_STATES = 512
REG512_VALUES = (1, 257, 5, 261, 200, 456)
REG512_INVS = [("Write", v) for v in REG512_VALUES] + ["Read"]
REG512_RESPS = ["Ok", ("Val", 0)] + [("Val", v) for v in REG512_VALUES]

REG512 = dict(name="reg512", transition=tg.reg_transition, postcondition=tg.reg_postcondition, init=0,
              invs=REG512_INVS, resps=REG512_RESPS, real=tg.reg_real)


# ---------------------------------------------------------------------------
# the WideTableModels
# ---------------------------------------------------------------------------

def _bits(ns, ni, nr, s, i, r):
    """post[s][i] with bit r[k] set for every k (index arrays)."""
    post = np.zeros((ns, ni, (nr + 31) // 32), dtype=np.uint32)
    np.bitwise_or.at(post, (s, i, r >> 5), np.uint32(1) << (r & 31).astype(np.uint32))
    return post


def _wcounter_table():
    from qsmd.models import WideTableModel
    n, k = WC_STATES, WC_SYMS
    s, i = np.meshgrid(np.arange(n), np.arange(k), indexing="ij")
    on_inv = (s + i) % n
    on_resp = np.repeat(np.arange(n)[:, None], k, axis=1)
    post = _bits(n, k, k, s.ravel(), i.ravel(), ((s + i) % 256).ravel())
    err = np.zeros_like(post)
    err[np.arange(n) % 64 == 63, 0, :] = 0xFFFFFFFF
    return WideTableModel(list(range(n)), WCOUNTER["invs"], WCOUNTER["resps"], on_inv, on_resp, post, err)


def _big_table():
    from qsmd.models import WideTableModel
    n = BIG_STATES
    s, i = np.meshgrid(np.arange(n), np.arange(2), indexing="ij")
    t = (s + i) % n
    on_resp = np.repeat(np.arange(n)[:, None], 2, axis=1)
    post = _bits(n, 2, 2, s.ravel(), i.ravel(), (((t >> 15) ^ t) & 1).ravel())
    return WideTableModel(list(range(n)), [0, 1], [0, 1], t, on_resp, post)


def _reg512_table():
    from qsmd.models import WideTableModel
    n, ni, nr = REG512_STATES, len(REG512_INVS), len(REG512_RESPS)
    read = ni - 1
    on_inv = np.repeat(np.arange(n)[:, None], ni, axis=1)
    for k, v in enumerate(REG512_VALUES):
        on_inv[:, k] = v
    on_resp = np.repeat(np.arange(n)[:, None], nr, axis=1)
    post = np.zeros((n, ni, 1), dtype=np.uint32)
    post[:, :read, 0] = 1                                   # Write v: Ok
    for r, x in enumerate(REG512_RESPS[1:], 1):             # Read in state v: Val v
        post[x[1], read, 0] = 1 << r
    return WideTableModel(list(range(n)), REG512_INVS, REG512_RESPS, on_inv, on_resp, post)


@functools.lru_cache(maxsize=None)
def wide_table(name):
    """The WideTableModel of a model of this module (KV from its closures,
    the others from numpy tables: WCOUNTER alone would take 2e7 closure
    calls), or of a ``tablegen`` model given as a closure dict's name."""
    from qsmd.models import WideTableModel
    built = {"wcounter": _wcounter_table, "big": _big_table, "reg512": _reg512_table}
    if name in built:
        return built[name]()
    c = BY_NAME[name]
    return WideTableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                        raises=ModelError)


BY_NAME = {"kv": KV, "wcounter": WCOUNTER, "big": BIG, "reg512": REG512,
           "register": tg.REGISTER, "lock": tg.LOCK, "ticket": tg.ticket_closures(16)}


def sampled_entries_equal_closures(name, n=1000, seed=0):
    """n sampled (state, invocation, response) entries of a numpy-built table
    against the model's closures; returns the number compared."""
    from qsmd.models import ModelError as PackageModelError
    c, m = BY_NAME[name], wide_table(name)
    rng = random.Random(f"{name}/{seed}")
    for _ in range(n):
        s, i, r = rng.choice(m.states), rng.choice(m.invs), rng.choice(m.resps)
        assert m.transition(s, L(i)) == c["transition"](s, L(i)), (s, i)
        assert m.transition(s, R(r)) == c["transition"](s, R(r)), (s, r)
        try:
            want = c["postcondition"](s, i, r)
        except ModelError:
            want = "raises"
        try:
            got = m.postcondition(s, i, r)
        except PackageModelError:
            got = "raises"
        assert got == want, (s, i, r)
    return n


def state_indices_visited(name, hist):
    """The table's state indices the real system passes through when the
    history's invocations are applied in history order (the generator's
    order)."""
    c, m = BY_NAME[name], wide_table(name)
    s, out = c["init"], []
    for _, (kind, x) in hist:
        if kind == "L":
            s = c["real"](s, x)[0]
            out.append(m.state_index[s])
    return out
