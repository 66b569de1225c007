"""Histories of any shape for the table-model tests: ill-formed ones, pids
shared by several operations in flight, pending invocations, stray and leading
responses -- everything ``tablegen.gen_history`` (and the device generators)
never emit, and the four rules of the reference that only matter then
(``takeInvocations`` stops at the first response, ``filter1`` removes the pid's
first invocation, ``findResponse => []`` is no node, undo by Lemma L1).

TEST INFRASTRUCTURE ONLY.

A model is any ``tablegen``-style closure dict with ``real`` (``tablegen``'s
own, ``wtablegen``'s, a ``ktablegen.product``).  Everything is deterministic
from a string seed.

Two families:

* **bent** (:func:`bent`): ``tablegen.gen_history`` on ``clients`` clients,
  the clients mapped onto ``pids_out`` pids (several operations of one pid in
  flight), then 0..3 mutations drawn with the weights :data:`MUTATIONS` (a
  response dropped, a stray response, a lone invocation, an event moved or
  duplicated, a response moved to the front, several responses delayed), cut
  to 128 events.
* **random** (:func:`random_history`): 0..16 events on 1..5 pids, each an
  invocation with probability 0.6, symbols drawn uniformly.

:func:`exactly` cuts or extends a history to a given length, :func:`census`
names the features a history has.

The settings (:data:`SETTINGS`) measured with ``max_nodes =
tablegen.MAX_NODES`` against ``oracle/linearise_lists.linearisable``; per
setting the histories with each feature (two_in_flight / stray_resp / pending /
resp_first), the status counts, the histories over 256 nodes and the median
node count:

    model       setting  n     2fl   stray  pend  rfirst  lin   nonlin  error  budget  >256  median
    register    6x14     400   350   121    139   64      74    303     0      23      106   24
    register    6x16     400   359   142    156   68      78    283     0      39      123   30
    register    8x24     200   199   69     78    39      23    135     0      42      89    122
    register    2x62     100   70    35     35    20      8     72      0      20      34    40
    register    random   500   330   338    430   179     50    450     0      0       0     0
    lock        6x14     400   349   134    180   84      47    246     102    5       42    7
    lock        6x16     400   352   132    157   75      44    229     112    15      64    6
    lock        8x24     200   198   69     93    42      19    96      66     19      43    8
    lock        2x62     100   63    32     36    15      4     60      31     5       17    17
    lock        random   500   335   338    433   173     52    356     92     0       0     0
    kv          6x14     400   351   126    140   65      55    310     0      35      136   44
    kv          6x16     400   359   121    145   52      110   235     0      55      149   46
    kv          8x24     200   199   61     88    34      24    88      0      88      126   4069
    kv          2x62     100   77    42     43    22      12    65      0      23      34    37
    kv          random   500   335   342    416   180     58    442     0      0       1     0
    register^4  6x14     400   356   109    131   40      77    297     0      26      131   34
    register^4  6x16     400   362   138    157   73      94    253     0      53      143   31
    register^4  8x24     200   198   70     76    33      27    108     0      65      102   283
    register^4  2x62     100   74    29     45    16      9     65      0      26      43    71
    register^4  random   500   334   344    426   186     45    455     0      0       0     0
    lock^8      6x14     400   349   128    155   70      27    208     160    5       48    5
    lock^8      6x16     400   347   116    140   61      32    181     172    15      65    7
    lock^8      8x24     200   198   65     79    37      7     89      91     13      42    9
    lock^8      2x62     100   64    25     37    12      1     46      49     4       13    6
    lock^8      random   500   347   334    444   187     44    347     109    0       0     0
"""

from __future__ import annotations

import random

import tablegen as tg

L, R = tg.L, tg.R
MAX_EVENTS = 128

# (clients, operations, pids_out, p_bug, histories)
SETTINGS = {"6x14": (6, 14, 5, 0.1, 400), "6x16": (6, 16, 5, 0.06, 400), "8x24": (8, 24, 6, 0.05, 200),
            "2x62": (2, 62, 2, 0.04, 100)}
RANDOM = "random"
RANDOM_COUNT = 500
ALL_SETTINGS = tuple(SETTINGS) + (RANDOM,)
SEED = "anyshape/1"

# the mutations of the bent family and the weight each is drawn with (16 in
# all, 1.5 draws a history on average).  "move a response to the front" has a
# rate of its own, RESP_FRONT: without it a leading response is rare.
# "delay_responses" moves 1..DELAY_MAX responses to later places: the
# operations then overlap many others, which is what lengthens a search (the
# candidates of a node are the invocations before the first remaining
# response), while strays, leading responses and, on the lock models, the
# raising Unlock end searches early.  It is drawn most often: without it, and
# with fewer clients and pids than these settings have (3 clients x 10
# operations on 2 pids was tried: 0.5 % to 2.5 % over 256 nodes whatever the
# weights), a history of the 32-event class hardly ever counts more than 256
# nodes, and pass 2 and the memo would not run there.
RESP_FRONT = 2
DELAY_MAX = 10
MUTATIONS = (("drop_response", 1), ("stray_response", 1), ("lone_invocation", 1), ("move_event", 2),
             ("duplicate_event", 1), ("response_to_front", RESP_FRONT), ("delay_responses", 8))
FEATURES = ("two_in_flight", "stray_resp", "pending", "resp_first")


def _pid_for(rng, h, fresh_ok=True):
    used = sorted({p for p, _ in h})
    if not used or (fresh_ok and rng.random() < 0.5):
        return max(used, default=-1) + 1
    return rng.choice(used)


def _mutate(model, rng, h, kind):
    resps = [k for k, (_, (x, _)) in enumerate(h) if x == "R"]
    if kind == "drop_response":
        if resps:
            del h[rng.choice(resps)]
    elif kind == "stray_response":
        h.insert(rng.randrange(len(h) + 1), (_pid_for(rng, h), R(rng.choice(model["resps"]))))
    elif kind == "lone_invocation":
        h.insert(rng.randrange(len(h) + 1), (_pid_for(rng, h), L(rng.choice(model["invs"]))))
    elif kind == "move_event":
        if h:
            e = h.pop(rng.randrange(len(h)))
            h.insert(rng.randrange(len(h) + 1), e)
    elif kind == "duplicate_event":
        if h:
            h.insert(rng.randrange(len(h) + 1), h[rng.randrange(len(h))])
    elif kind == "response_to_front":
        if resps:
            h.insert(0, h.pop(rng.choice(resps)))
    elif kind == "delay_responses":
        for _ in range(rng.randint(1, DELAY_MAX)):
            resps = [k for k, (_, (x, _)) in enumerate(h) if x == "R"]
            if resps:
                k = rng.choice(resps)
                e = h.pop(k)
                h.insert(rng.randint(k, len(h)), e)
    else:
        raise ValueError(kind)


def bent(model, rng, clients, ops, pids_out, p_bug):
    """One history of the bent family."""
    base = tg.gen_history(model, rng, clients, ops, p_bug)
    order = list(range(clients))
    rng.shuffle(order)
    pid_of = {c: k % pids_out for k, c in enumerate(order)}
    h = [(pid_of[c], e) for c, e in base]
    kinds, weights = zip(*MUTATIONS)
    for _ in range(rng.randrange(4)):
        _mutate(model, rng, h, rng.choices(kinds, weights)[0])
    return h[:MAX_EVENTS]


def random_history(model, rng):
    """One history of the random family."""
    n_pids = rng.randint(1, 5)
    out = []
    for _ in range(rng.randint(0, 16)):
        pid = rng.randrange(n_pids)
        if rng.random() < 0.6:
            out.append((pid, L(rng.choice(model["invs"]))))
        else:
            out.append((pid, R(rng.choice(model["resps"]))))
    return out


def batch(model, setting, n=None, seed=SEED):
    """The histories of one setting (a key of SETTINGS, or RANDOM) for `model`."""
    rng = random.Random(f"{seed}/{model['name']}/{setting}")
    if setting == RANDOM:
        return [random_history(model, rng) for _ in range(RANDOM_COUNT if n is None else n)]
    clients, ops, pids_out, p_bug, n0 = SETTINGS[setting]
    return [bent(model, rng, clients, ops, pids_out, p_bug) for _ in range(n0 if n is None else n)]


def exactly(h, n):
    """`h` cut to its first n events or, when shorter, extended to n events
    with its own events repeated from the start (so every symbol stays one of
    the model's).  A cut in the middle of an operation is itself what makes
    the result ill-formed."""
    if len(h) >= n:
        return list(h[:n])
    if not h:
        raise ValueError("an empty history cannot be extended")
    return list(h) + [h[k % len(h)] for k in range(n - len(h))]


def census(h):
    """The names (of FEATURES) of what `h` has: an invocation of a pid with
    one already unanswered, a response of a pid with none unanswered, an
    invocation never answered, a response as the first event."""
    open_ = {}
    out = set()
    for pid, (kind, _) in h:
        if kind == "L":
            open_[pid] = open_.get(pid, 0) + 1
            if open_[pid] > 1:
                out.add("two_in_flight")
        elif open_.get(pid, 0) > 0:
            open_[pid] -= 1
        else:
            out.add("stray_resp")
    if any(open_.values()):
        out.add("pending")
    if h and h[0][1][0] == "R":
        out.add("resp_first")
    return out
