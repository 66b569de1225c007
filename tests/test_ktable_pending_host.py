"""The rule that lets pending invocations take effect, on the keyed product
model, on the host: tests/pending_ref.py over
tests/ktablegen.py's product closures against hand-derived known answers,
against the definition (some completion of the history is linearisable by the
literal oracle), against the per-key verdicts (locality) and against today's
oracle where the two must agree; and replay_witness for keyed models with
assumed levels."""

import functools
import itertools
import random

import pytest

import ktablegen as kg
import pending_ref as pr
import tablegen as tg
from linearise_lists import linearisable as oracle_linearisable
from qsmd.linearisability import replay_witness
from qsmd.models import KeyedTableModel, TableModel

L, R = tg.L, tg.R
REG = tg.REGISTER


def W(k, v):
    return L((k, ("Write", v)))


def Rd(k):
    return L((k, "Read"))


def Val(v):
    return R(("Val", v))


@functools.lru_cache(maxsize=None)
def prod(K):
    return kg.product(REG, K)


@functools.lru_cache(maxsize=None)
def keyed(K):
    return KeyedTableModel(TableModel.from_closures(REG["transition"], REG["postcondition"], REG["init"],
                                                    REG["invs"], REG["resps"]), K)


def today(model, h, max_nodes=0):
    return oracle_linearisable(model["transition"], model["postcondition"], model["init"], h, max_nodes)


def ops(path):
    return [(pid, inv, resp) for pid, inv, resp, _ in path]


# ------------------------------------------------------------------ 1. KATs

KAT_SEEN = [(0, W(2, 1)), (1, Rd(2)), (1, Val(1))]
KAT_OTHER_KEY = [(0, W(2, 1)), (1, Rd(1)), (1, Val(1))]
KAT_TWO_KEYS = [(0, W(0, 1)), (1, W(7, 2)), (2, Rd(7)), (2, Val(2)), (2, Rd(0)), (2, Val(1))]
KAT_TWO_KEYS_SWAPPED = [(0, W(0, 1)), (1, W(7, 2)), (2, Rd(7)), (2, Val(1)), (2, Rd(0)), (2, Val(2))]
# (history, K, status, nodes)
KATS = [(KAT_SEEN, 4, "lin", 2), (KAT_OTHER_KEY, 4, "nonlin", 3), (KAT_TWO_KEYS, 8, "lin", 4),
        (KAT_TWO_KEYS_SWAPPED, 8, "nonlin", 9)]


def test_known_answers():
    for h, K, status, nodes in KATS:
        assert pr.linearisable_pending(prod(K), h)[:2] == (status, nodes), h
    # the crashed client's write on key 2 took effect: the read of key 2 saw it
    assert today(prod(4), KAT_SEEN)[0] == "nonlin"
    path = pr.linearisable_pending(prod(4), KAT_SEEN)[2]
    assert path == [(0, (2, ("Write", 1)), "Ok", True), (1, (2, "Read"), ("Val", 1), False)]
    # both pending writes assumed, each on its own key
    path = pr.linearisable_pending(prod(8), KAT_TWO_KEYS)[2]
    assert [a for *_, a in path] == [True, True, False, False]


# ----------------------------------------------------------- 2. the definition

N_DEF = 300
CRASH_DEF = 0.4


@functools.lru_cache(maxsize=None)
def crashed_def():
    rng = random.Random(f"kpending/def/register^2/3x8/{CRASH_DEF}")
    return [pr.crash(tg.gen_history(prod(2), rng, 3, 8, 0.15), rng, CRASH_DEF) for _ in range(N_DEF)]


def completions(model, h):
    """Every pending invocation either deleted or answered by one symbol, the
    answers appended at the end."""
    pend = pr.pending_invocations(h)
    assert len(pend) <= 3
    for choice in itertools.product([None] + list(model["resps"]), repeat=len(pend)):
        gone = {k for k, c in zip(pend, choice) if c is None}
        out = [e for k, e in enumerate(h) if k not in gone]
        out += [(h[k][0], R(c)) for k, c in zip(pend, choice) if c is not None]
        yield out


def test_verdict_is_some_completion_is_linearisable():
    model = prod(2)
    hists = crashed_def()
    flipped = with_pending = 0
    keys = set()
    for i, h in enumerate(hists):
        got = pr.linearisable_pending(model, h)[0]
        assert got in ("lin", "nonlin")
        want = any(today(model, c)[0] == "lin" for c in completions(model, h))
        assert (got == "lin") == want, i
        with_pending += bool(pr.pending_invocations(h))
        flipped += got == "lin" and today(model, h)[0] == "nonlin"
        keys |= {h[k][1][1][0] for k in pr.pending_invocations(h)}
    print("histories with a pending invocation:", with_pending, "nonlin -> lin:", flipped)
    assert with_pending > N_DEF // 2 and flipped > 0 and keys == {0, 1}


# ------------------------------------------------------------------ 3. locality

LOCAL_NODES = 200000
LOCALITY = [(4, "3x10", 400), (4, "4x16", 300), (2, "4x16", 300)]


def split_by_key(h):
    """The per-key sub-histories of a client history (every pid's events
    alternate invocation, response, ..., maybe ending in an invocation): an
    operation is an invocation and its pid's next response, if it has one."""
    open_key, parts = {}, {}
    for pid, (kind, x) in h:
        if kind == "L":
            assert pid not in open_key
            k, inv = x
            open_key[pid] = k
            parts.setdefault(k, []).append((pid, L(inv)))
        else:
            parts[open_key.pop(pid)].append((pid, (kind, x)))
    return parts


@pytest.mark.parametrize("K,setting,n", LOCALITY)
def test_locality(K, setting, n):
    """The product verdict is the conjunction of the per-key verdicts on the
    component: a pending invocation on one key helps no other."""
    model = prod(K)
    rng = random.Random(f"kloc/register/{K}/{setting}")
    seen, several = set(), 0
    for i, h in enumerate(tg.gen_batch(model, setting, n)):
        h = pr.crash(h, rng, 0.4)
        whole = pr.linearisable_pending(model, h, LOCAL_NODES)[0]
        parts = split_by_key(h)
        per_key = [pr.linearisable_pending(REG, sub, LOCAL_NODES)[0] for _, sub in sorted(parts.items())]
        assert whole != "budget" and "budget" not in per_key, i
        assert (whole == "lin") == all(v == "lin" for v in per_key), (i, whole, per_key)
        seen.add(whole)
        several += len(parts) > 1 and bool(pr.pending_invocations(h))
    assert seen == {"lin", "nonlin"} and several > n // 3


# ---------------------------------------- 4. replay_witness with assumed levels

def test_replay_of_an_assumed_witness():
    m4, m8 = keyed(4), keyed(8)
    ok, val = m4.resps.index("Ok"), lambda v: m4.resps.index(("Val", v))
    assert replay_witness(m4, KAT_SEEN, [0, 1], None, assumed=[ok, None])
    assert replay_witness(m8, KAT_TWO_KEYS, [0, 1, 2, 4], None, assumed=[ok, ok, None, None])
    # the reference's paths, as witnesses: the chosen events and the assumed symbols
    w1 = [(0, W(0, 1)), (0, R("Ok")), (0, W(5, 2))]
    hists = [w1 + [(1, Rd(5)), (1, Val(0))], w1 + [(1, Rd(5)), (1, Val(0)), (1, Rd(0)), (1, Val(1))],
             KAT_SEEN, KAT_TWO_KEYS] + [h for h in crashed_def()[:60]]
    accepted = with_assumed = 0
    for n, h in enumerate(hists):
        K = 8 if n < 4 else 2
        st, _, path = pr.linearisable_pending(prod(K), h)
        if st != "lin":
            continue
        removed, wit, asm = set(), [], []
        for pid, inv, resp, assumed in path:
            # (a client history: the chosen event is the pid's first remaining invocation)
            j = next(i for i, (p, (k, _)) in enumerate(h) if i not in removed and k == "L" and p == pid)
            assert h[j][1][1] == inv
            removed.add(j)
            if not assumed:
                removed.add(next(i for i, (p, (k, _)) in enumerate(h) if i not in removed and k == "R" and p == pid))
            wit.append(j)
            asm.append(keyed(K).resps.index(resp) if assumed else None)
        assert pr.witness_ops(keyed(K).resps, h, wit, asm) == path
        assert replay_witness(keyed(K), h, wit, None, assumed=asm), h
        accepted += 1
        with_assumed += any(a is not None for a in asm)
    assert accepted > 20 and with_assumed > 10
    # a model0 with a different state per key
    assert replay_witness(m4, [(0, W(1, 3)), (1, Rd(2)), (1, Val(2))], [1, 0], (0, 1, 2, 3), assumed=[None, ok])
    assert not replay_witness(m4, [(0, W(1, 3)), (1, Rd(2)), (1, Val(2))], [1, 0], None, assumed=[None, ok])
    # an assumed level where the pid still has a response
    assert not replay_witness(m4, KAT_SEEN, [0, 1], None, assumed=[ok, val(1)])
    # a symbol the key's state does not allow (Val 0 for a Write; Val 1 for a Read of key 1 at state 0)
    assert not replay_witness(m4, KAT_SEEN, [0, 1], None, assumed=[val(0), None])
    assert not replay_witness(m4, [(0, Rd(1))], [0], None, assumed=[val(1)])
    assert replay_witness(m4, [(0, Rd(1))], [0], None, assumed=[val(0)])
    assert replay_witness(m4, [(0, Rd(1))], [0], (0, 1, 0, 0), assumed=[val(1)])
    # an assumed list of the wrong length
    assert not replay_witness(m4, KAT_SEEN, [0, 1], None, assumed=[ok])
    assert not replay_witness(m4, KAT_SEEN, [0, 1], None, assumed=[ok, None, None])
    # the pending write on another key does not help; a Write left over is no leaf
    assert not replay_witness(m4, KAT_OTHER_KEY, [0, 1], None, assumed=[ok, None])
    assert not replay_witness(m4, KAT_SEEN, [], None, assumed=[])
    # (without `assumed`: today's rule, unchanged)
    assert not replay_witness(m4, KAT_SEEN, [0, 1])


# ------------------------------------------------------- 5. complete histories

@pytest.mark.parametrize("K", [2, 4])
def test_complete_histories_are_todays(K):
    model = prod(K)
    seen = set()
    for h in tg.gen_batch(model, "3x10", 300) + tg.gen_batch(model, "4x16", 100):
        assert not pr.pending_invocations(h)
        st, nodes, path = pr.linearisable_pending(model, h, tg.MAX_NODES)
        assert (st, nodes, ops(path)) == today(model, h, tg.MAX_NODES)
        assert not any(a for *_, a in path)
        seen.add(st)
    assert {"lin", "nonlin"} <= seen
