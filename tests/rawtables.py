"""Random raw tables whose responses move the state: the inputs of
test_rawtables_host.py, test_gpu_rawtables.py and
test_gpu_rawtables_kpending_local.py.

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
:data:`KEYED_LOCAL` and the helpers at the end of the file are the inputs of
the keyed pending call's local mode
(tests/test_gpu_rawtables_kpending_local.py).
"""

from __future__ import annotations

import collections
import functools
import random

import numpy as np

import anyshape as an
import explain_ref as xr
import kpendinglocal_ref as klr
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
# The shapes of the keyed pending call's local mode (knob "kpending_local"), apart from KEYED so that the
# parametrisations over KEYED do not grow: two-key products whose *parts* pass pass 1's 256 nodes and reach a
# low max_nodes, and eight-key products for keyed_walk.  k8_r2's model0 holds every state of n_r2.
KEYED_LOCAL = {
    "k2_deep": ("n_deep", 2, None),
    "k2_r32": ("n_r32", 2, None),
    "k8_1inv": ("n_1inv", 8, None),
    "k8_r2": ("n_r2", 8, (0, 3, 1, 4, 2, 0, 4, 1)),
}
LOCAL_SHAPES = ("k_max", "k_deep", "k_odd", "k2_deep", "k2_r32")    # every history of their crashed batches splits
LOW_NODES = 40                              # the low max_nodes at which parts of k2_deep / k2_r32 are `budget`
# The crash draws of the KEYED_LOCAL ids carry this suffix in their seed string.  Without it 2 of k2_deep's and 1
# of k2_r32's 410 crashed histories are `error` on the product and `lin` key by key (ERROR_LIN_KAT is one of
# them), which happened at 5 of 12 suffixes tried on k2_deep and at 5 of 12 on k2_r32; "/3" is the first at which
# neither shape has such a history, so that test_rawtables_host.py can assert on whole batches that the product
# and the local mode disagree in two ways only.  The choice looked at the two restatements alone.
LOCAL_CRASH_SALT = "/3"
# k2_r32: `error` after 20 nodes on the product, `lin` key by key (key 0: 9 nodes, key 1: 11).  The product
# search, after a failure on key 0, backtracks into other orders of key 1's operations and meets an entry of
# post_err there; key 1's own search is linearisable on its first order and never visits it.
ERROR_LIN_KAT = [
    (0, ("L", (1, 2))), (0, ("R", 28)), (0, ("L", (0, 1))), (3, ("L", (0, 2))), (1, ("L", (0, 0))), (3, ("R", 0)),
    (1, ("R", 27)), (3, ("L", (0, 1))), (0, ("R", 12)), (2, ("L", (0, 1))), (2, ("R", 19)), (0, ("L", (0, 0))),
    (2, ("L", (1, 1))), (1, ("L", (0, 2))), (3, ("R", 8)), (3, ("L", (0, 1))), (3, ("R", 29)), (0, ("R", 11)),
    (3, ("L", (1, 1))), (0, ("L", (0, 2))), (0, ("R", 2)), (3, ("R", 30))]


def keyed_spec(name):
    """(component, keys, model0) of an id of KEYED or KEYED_LOCAL, else None."""
    return KEYED.get(name) or KEYED_LOCAL.get(name)


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
    if keyed_spec(name):
        comp, K, model0 = keyed_spec(name)
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
    if keyed_spec(name):
        comp, K, _ = keyed_spec(name)
        return KeyedTableModel(model(comp), K)
    sp, t = spec(name), tables_of(name)
    wide = (name in WIDE or name in TWINS) if wide is None else wide
    cls = WideTableModel if wide else TableModel
    words, errw = (t.wide_post, t.wide_err) if wide else (t.post_words, t.err_words)
    return cls(list(range(sp.ns)), list(range(sp.ni)), list(range(sp.nr)), t.on_inv, t.on_resp, words,
               None if sp.p_err is None else errw, init_state=sp.init)


def model0_of(name):
    """The model0 a keyed shape is generated and checked from (None: init_model)."""
    return keyed_spec(name)[2] if keyed_spec(name) else None


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
def crashed(name, setting):
    """The check batch with clients crashed."""
    salt = LOCAL_CRASH_SALT if name in KEYED_LOCAL else ""
    rng = random.Random(f"rawtables/crash/{name}/{setting}{salt}")
    return [pr.crash(h, rng, CRASH) for h in histories(name, setting)]


@functools.lru_cache(maxsize=None)
def crash_case(name, setting):
    """The check batch with clients crashed, and pending_ref's results."""
    hists = crashed(name, setting)
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


# ---------------------------------------------------------------------------
# the keyed pending call's local mode (tests/kpendinglocal_ref.py)
# ---------------------------------------------------------------------------

def inits_of(name):
    """The per-key start states of a keyed id."""
    comp, K, model0 = keyed_spec(name)
    return (spec(comp).init,) * K if model0 is None else tuple(model0)


def local_parts(name, hist, max_nodes, c=None):
    """The restatement on one history, part by part: None when it does not
    split, else ([(key, status, nodes)], [path]) in ascending key order, every
    part searched with the component's closures ``c`` from its key's model0
    state."""
    comp, K, _ = keyed_spec(name)
    c = closures(comp) if c is None else c
    split = klr.split(c, K, hist)
    if split is None:
        return None
    init = inits_of(name)
    found = [(k, pr.linearisable_pending(c, klr.unkeyed(sub), max_nodes, init[k])) for k, sub in split]
    return [(k, st, nd) for k, (st, nd, _) in found], [path for _, (_, _, path) in found]


@functools.lru_cache(maxsize=None)
def local_crash_case(name, setting, max_nodes=MAX_NODES, variant=None):
    """The crashed batch of :func:`crash_case` under the local mode's
    restatement: (histories, per history [(key, status, nodes)] of its parts
    -- None for a history that does not split --, per history the combined
    (status, nodes), per history the parts' paths).  ``variant``: the
    "identity_resp" / "ignore_err" closures."""
    comp = keyed_spec(name)[0]
    c = closures(comp, **({variant: True} if variant else {}))
    hists = crashed(name, setting)
    found = [local_parts(name, h, max_nodes, c) for h in hists]
    parts = [None if f is None else f[0] for f in found]
    combined = [None if p is None else klr.combine([(st, nd) for _, st, nd in p]) for p in parts]
    return hists, parts, combined, [None if f is None else f[1] for f in found]


def keyed_walk(name, per_key):
    """A keyed history of pending invocations only: every key gets
    :func:`pending_walk`'s walk of ``per_key`` invocations on the component
    from that key's model0 state, on pids of its own (key k: pids k * per_key
    ...), the invocations rewritten to ``(k, i)``, the keys interleaved
    round-robin.  Returns (history, the per-key end states)."""
    comp, K, _ = keyed_spec(name)
    walks, ends = [], []
    for k, s in enumerate(inits_of(name)):
        h, states = pending_walk(comp, per_key, start=s, first_pid=k * per_key)
        walks.append([(pid, tg.L((k, i))) for pid, (_, i) in h])
        ends.append(states[-1])
    return [walks[k][d] for d in range(per_key) for k in range(K)], ends


def empty_allowed(name):
    """The (s, i) of a component at which no response is allowed although the
    packed ``post`` word is not zero: its only bits are at or above ``n_resp``
    or ones that ``post_err`` removes."""
    sp, t = spec(name), tables_of(name)
    return [(s, i) for s in range(sp.ns) for i in range(sp.ni)
            if allowed_bits(name, s, i) == 0 and int(t.post_words[s, i]) != 0]


WALK_PER_KEY = 16                           # 8 keys x 16 pending invocations: the 128 events of the widest class
SHORT_WALK = 3


def failing_walk(name, per_key=SHORT_WALK):
    """:func:`keyed_walk` with ``per_key`` invocations per key and, on the
    highest key, one completed operation of a pid of its own at the end: the
    first (invocation, response) in table order that the walk's end state on
    that key neither allows nor raises on and with which the restatement finds
    the key's part `nonlin`.  Returns (history, the key, (inv, resp))."""
    comp, K, _ = keyed_spec(name)
    sp, t, c = spec(comp), tables_of(comp), closures(comp)
    walk, ends = keyed_walk(name, per_key)
    k, end = K - 1, ends[K - 1]
    for i in range(sp.ni):
        for r in range(sp.nr):
            if (allowed_bits(comp, end, i) >> r) & 1 or t.err[end, i, r]:
                continue
            h = walk + [(K * per_key, tg.L((k, i))), (K * per_key, tg.R(r))]
            if dict((key, st) for key, st, _ in local_parts(name, h, MAX_NODES, c)[0])[k] == "nonlin":
                return h, k, (i, r)
    raise AssertionError(name)


def empty_allowed_histories(name):
    """For every (s, i) of :func:`empty_allowed` on the component whose state
    ``s`` is some key's model0 state (the first such key, k), three histories:
    the pending invocation ``(k, i)`` alone; with a complete, allowed
    operation on the next key; with a complete operation on key k itself that
    ``s`` allows.  [(s, i, k, [h1, h2, h3])]."""
    comp, K, _ = keyed_spec(name)
    sp, init = spec(comp), inits_of(name)

    def allowed_op(s):
        j = next(j for j in range(sp.ni) if allowed_bits(comp, s, j))
        a = allowed_bits(comp, s, j)
        return j, (a & -a).bit_length() - 1

    out = []
    for s, i in empty_allowed(comp):
        if s not in init:
            continue
        k = init.index(s)
        k2 = (k + 1) % K
        alone = [(0, tg.L((k, i)))]
        j2, r2 = allowed_op(init[k2])
        j, r = allowed_op(s)
        out.append((s, i, k, [alone, alone + [(1, tg.L((k2, j2))), (1, tg.R(r2))],
                              alone + [(1, tg.L((k, j))), (1, tg.R(r))]]))
    return out


@functools.lru_cache(maxsize=None)
def walk_case(name):
    """The walk batch of a KEYED_LOCAL id: the 128-event walk, the short walk
    with one failing key, the :func:`empty_allowed_histories`; with the local
    restatement's parts and combined results and the product's
    (pending_ref on the product closures)."""
    hists = [keyed_walk(name, WALK_PER_KEY)[0], failing_walk(name)[0]]
    for _, _, _, three in empty_allowed_histories(name):
        hists += three
    parts = [local_parts(name, h, MAX_NODES)[0] for h in hists]
    combined = [klr.combine([(st, nd) for _, st, nd in p]) for p in parts]
    c = closures(name)
    return hists, parts, combined, [pr.linearisable_pending(c, h, MAX_NODES) for h in hists]
