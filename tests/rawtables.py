"""Random raw tables whose responses move the state: the inputs of
test_rawtables_host.py and test_gpu_rawtables.py.

TEST INFRASTRUCTURE ONLY.

Every named model of tablegen / wtablegen has an identity ``on_resp``, exactly
one allowed response per (state, invocation) and no table bit at or above
``n_resp``, so the fourth table, words of ``post`` with several bits and the
``& symbols`` cut of the pending kernels are never what decides a verdict
there.  Here all four tables are drawn at random:

    postcondition = bit r of post[s][i]        (post_err bit r: raises, wins)
    next state    = on_resp[on_inv[s][i]][r]

:func:`tables` draws them, :func:`closures` restates the step on the boolean
cubes and the int arrays themselves (the reference side never imports
``qsmd.models``), :func:`model` builds the device model from the same arrays
through the explicit constructors.  States, invocations and responses are the
integers themselves.

The shapes (:data:`NARROW`, :data:`WIDE`, :data:`KEYED`) and their densities
and seeds are frozen: they were chosen so that the conditions
test_rawtables_host.py asserts on the reference alone hold (every status
reached, deep searches where a memo or pass 2 needs them, and (status, nodes)
changing on most histories once ``on_resp`` is replaced by identity rows).
"""

from __future__ import annotations

import collections
import functools
import random

import numpy as np

import anyshape as an
import explain_ref as xr
import ktablegen as kg
import pending_ref as pr
import tablegen as tg
from linearise_lists import ModelError
from linearise_lists import linearisable as oracle_linearisable

MAX_NODES = tg.MAX_NODES
CRASH = 0.3
# the check batches of every shape: tablegen setting -> histories
BATCHES = {"3x10": 200, "4x16": 150, "6x24": 60}
ANY_SETTINGS = {"6x16": 100, an.RANDOM: 200}

Tables = collections.namedtuple("Tables", "on_inv on_resp post err post_words err_words wide_post wide_err")
# p_err None: no post_err table at all (the NULL branch); high: None, "post" or "err"
Spec = collections.namedtuple("Spec", "ns ni nr p_post p_err high init seed")

NARROW = {
    "n_max": Spec(256, 32, 32, 0.2, 0.005, None, 255, 21),    # the 80 KB blob, response bit 31, state 255
    "n_r32": Spec(7, 3, 32, 0.15, 0.01, None, 0, 3),          # a full response word on few states
    "n_r2": Spec(5, 32, 2, 0.6, 0.03, "post", 0, 3),          # n_inv >> n_resp; the pending mask
    "n_noerr": Spec(200, 5, 9, 0.45, None, "post", 0, 4),     # post_err == NULL, garbage above bit 8
    "n_errhi": Spec(6, 4, 5, 0.4, 0.03, "err", 0, 5),         # high post_err bits neither raise nor mask
    "n_deep": Spec(3, 2, 2, 0.6, 0.1, None, 0, 62),           # thousands of nodes, pass 2, the memos, budget
    "n_1inv": Spec(2, 1, 31, 0.1, 0.03, "post", 0, 15),       # one invocation symbol, many allowed responses
    "n_one": Spec(1, 1, 1, 1.0, None, None, 0, 8),            # every dimension 1
    "c_odd": Spec(5, 4, 3, 0.5, 0.04, "post", 0, 50),         # (the component of k_odd)
}
WIDE = {
    "w_3w": Spec(300, 40, 70, 0.05, 0.005, "err", 0, 11),     # post_words 3; responses in words 1 and 2
    "w_max_state": Spec(65536, 2, 33, 0.1, None, None, 65535, 12),      # 16-bit states; bit 0 of word 1
    "w_256": Spec(3, 256, 256, 0.02, 0.003, None, 0, 13),     # post_words 8; codes 128..255
    "w_64": Spec(5, 3, 64, 0.06, 0.02, None, 0, 14),          # a full last word
    "w_65": Spec(5, 3, 65, 0.06, 0.02, "post", 0, 15),        # a last word with one bit
}
# the narrow shapes that also run as wide tables (equal results, array for array)
TWINS = {"w_n_r32": "n_r32", "w_n_deep": "n_deep", "w_n_r2": "n_r2"}
# id -> (component, keys, model0)
KEYED = {
    "k_max": ("n_max", 8, (255, 0, 17, 255, 128, 3, 254, 1)),
    "k_deep": ("n_deep", 8, None),
    "k_odd": ("c_odd", 3, None),
    "k_one": ("n_r32", 1, None),
}
DEEP = ("n_deep", "n_1inv", "k_deep")       # at least one budget, ten searches beyond pass 1's 256 nodes


def tables(seed, ns, ni, nr, p_post, p_err, high_bits):
    """``on_inv`` / ``on_resp`` uniform over 0..ns-1, the boolean cubes
    ``post[s][i][r]`` / ``err[s][i][r]`` with the given densities, and the
    packed uint32 words: narrow ``[ns][ni]`` (None beyond 32 responses) and
    wide ``[ns][ni][ceil(nr/32)]``.  ``high_bits`` "post" sets every bit at or
    above ``nr`` of every post word (wide: of the last word) and none of
    post_err's, "err" the reverse, None neither.  The cubes never hold them."""
    assert high_bits in (None, "post", "err")
    rng = np.random.default_rng(seed)
    on_inv = rng.integers(0, ns, size=(ns, ni))
    on_resp = rng.integers(0, ns, size=(ns, nr))
    post = rng.random((ns, ni, nr)) < p_post
    err = rng.random((ns, ni, nr)) < (p_err or 0.0)
    pw = (nr + 31) // 32
    high = np.zeros(pw, dtype=np.uint32)
    if nr % 32:
        high[-1] = (0xFFFFFFFF << (nr % 32)) & 0xFFFFFFFF

    def pack(cube, with_high):
        padded = np.zeros((ns, ni, pw * 32), dtype=np.uint64)
        padded[:, :, :nr] = cube
        words = (padded.reshape(ns, ni, pw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=3).astype(np.uint32)
        return words | high if with_high else words

    wide_post, wide_err = pack(post, high_bits == "post"), pack(err, high_bits == "err")
    narrow = (wide_post[:, :, 0].copy(), wide_err[:, :, 0].copy()) if nr <= 32 else (None, None)
    return Tables(on_inv, on_resp, post, err, narrow[0], narrow[1], wide_post, wide_err)


def spec(name):
    name = TWINS.get(name, name)
    return NARROW[name] if name in NARROW else WIDE[name]


@functools.lru_cache(maxsize=None)
def tables_of(name):
    sp = spec(name)
    return tables(sp.seed, sp.ns, sp.ni, sp.nr, sp.p_post, sp.p_err, sp.high)


def closures(name, identity_resp=False, ignore_err=False):
    """A fresh tablegen-style dict for the shape ``name`` (its ``real`` holds
    a seeded generator of its own); a keyed id gives the product
    (``ktablegen.product``) of its component from its model0.
    ``identity_resp`` / ``ignore_err``: the variants that show the inputs
    depend on ``on_resp`` / ``post_err`` (a response leaves the state alone /
    nothing raises); the generated system (``real``) stays the true one."""
    if name in KEYED:
        comp, K, model0 = KEYED[name]
        p = kg.product(closures(comp, identity_resp, ignore_err), K)
        p["name"] = name
        if model0 is not None:
            p["init"] = model0
        return p
    sp, t = spec(name), tables_of(name)
    on_inv, on_resp, post, err = t.on_inv, t.on_resp, t.post, t.err
    has_err = sp.p_err is not None and not ignore_err

    def transition(s, ev):
        kind, x = ev
        if kind == "L":
            return int(on_inv[s, x])
        return s if identity_resp else int(on_resp[s, x])

    def postcondition(s, i, r):
        if has_err and err[s, i, r]:
            raise ModelError(f"raw table: ({s}, {i}, {r}) raises")
        return bool(post[s, i, r])

    rng = random.Random(f"rawtables/real/{name}")
    every = list(range(sp.nr))

    def real(s, i):
        ok = [r for r in every if post[s, i, r] and not err[s, i, r]]
        r = rng.choice(ok or every)
        return int(on_resp[on_inv[s, i], r]), r

    return dict(name=TWINS.get(name, name), transition=transition, postcondition=postcondition, init=sp.init,
                invs=list(range(sp.ni)), resps=every, real=real)


@functools.lru_cache(maxsize=None)
def model(name, wide=None):
    """The device model of a shape, from the arrays of :func:`tables_of`
    through the explicit constructor: a TableModel, a WideTableModel (the
    WIDE shapes and the TWINS) or a KeyedTableModel."""
    from qsmd.models import KeyedTableModel, TableModel, WideTableModel
    if name in KEYED:
        comp, K, _ = KEYED[name]
        return KeyedTableModel(model(comp), K)
    sp, t = spec(name), tables_of(name)
    wide = (name in WIDE or name in TWINS) if wide is None else wide
    cls = WideTableModel if wide else TableModel
    words, errw = (t.wide_post, t.wide_err) if wide else (t.post_words, t.err_words)
    return cls(list(range(sp.ns)), list(range(sp.ni)), list(range(sp.nr)), t.on_inv, t.on_resp, words,
               None if sp.p_err is None else errw, init_state=sp.init)


def model0_of(name):
    """The model0 a keyed shape is generated and checked from (None: init_model)."""
    return KEYED[name][2] if name in KEYED else None


# ---------------------------------------------------------------------------
# histories and references (each computed once, shared, never changed)
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def histories(name, setting):
    return tg.gen_batch(closures(name), setting, BATCHES[setting])


def _oracle(c, hists):
    return [oracle_linearisable(c["transition"], c["postcondition"], c["init"], h, MAX_NODES) for h in hists]


@functools.lru_cache(maxsize=None)
def check_case(name, setting):
    """(histories, [(status, nodes, path)]) of one check batch."""
    hists = histories(name, setting)
    return hists, _oracle(closures(name), hists)


@functools.lru_cache(maxsize=None)
def variant_ref(name, setting, variant):
    """The same batch under the "identity_resp" / "ignore_err" closures."""
    return _oracle(closures(name, **{variant: True}), histories(name, setting))


@functools.lru_cache(maxsize=None)
def crash_case(name, setting):
    """The check batch with clients crashed, and pending_ref's results."""
    rng = random.Random(f"rawtables/crash/{name}/{setting}")
    hists = [pr.crash(h, rng, CRASH) for h in histories(name, setting)]
    c = closures(name)
    return hists, [pr.linearisable_pending(c, h, MAX_NODES) for h in hists]


@functools.lru_cache(maxsize=None)
def anyshape_case(name, setting):
    """anyshape's histories, the check call's reference and the pending one's."""
    c = closures(name)
    hists = an.batch(c, setting, ANY_SETTINGS[setting])
    return hists, _oracle(c, hists), [pr.linearisable_pending(c, h, MAX_NODES) for h in hists]


@functools.lru_cache(maxsize=None)
def explain_case(name, setting):
    hists = histories(name, setting)
    return hists, xr.explain_all(closures(name), hists, MAX_NODES)


def pass2_expected(ref, budget):
    """The histories pass 2 takes at a "table_budget" (0: a single pass)."""
    return sum(1 for r in ref if r[1] > budget or (r[0] == "budget" and r[1] >= budget)) if budget else 0


def allowed_bits(name, s, i):
    """The responses the cubes allow at (s, i), as a bitset."""
    t = tables_of(name)
    return sum(1 << r for r in range(spec(name).nr) if t.post[s, i, r] and not t.err[s, i, r])


def pending_walk(name, n, start=None, first_pid=0):
    """``n`` invocations, each on a pid of its own (from ``first_pid``), none
    answered, chosen so that the search's first descent assumes one of
    *several* allowed symbols at every level: from the state ``start`` (the
    initial one), an invocation with at least two allowed responses, the state
    stepped with the lowest of them (the first the search tries).  Returns
    (history, states): ``states[d]`` is the state after ``d`` levels.  A
    shorter walk is a prefix of a longer one."""
    sp, t = spec(name), tables_of(name)
    rng = random.Random(f"rawtables/walk/{name}/{start}")
    s = sp.init if start is None else start
    h, states = [], [s]
    for pid in range(first_pid, first_pid + n):
        several = [i for i in range(sp.ni) if bin(allowed_bits(name, s, i)).count("1") >= 2]
        assert several, (name, s)
        i = rng.choice(several)
        a = allowed_bits(name, s, i)
        h.append((pid, tg.L(i)))
        s = int(t.on_resp[t.on_inv[s, i], (a & -a).bit_length() - 1])
        states.append(s)
    return h, states
