"""The rule that lets pending invocations take effect, on the
host: tests/pending_ref.py against hand-derived known answers, against the
definition (some completion of the history is linearisable by the literal
oracle) and against today's oracle where the two must agree."""

import functools
import itertools
import random

import pytest

import pending_ref as pr
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd.linearisability import replay_witness
from qsmd.models import TableModel

L, R = tg.L, tg.R
REG, LOCK = tg.REGISTER, tg.LOCK


def today(model, h, max_nodes=0):
    return oracle_linearisable(model["transition"], model["postcondition"], model["init"], h, max_nodes)


def ops(path):
    return [(pid, inv, resp) for pid, inv, resp, _ in path]


# ------------------------------------------------------------------ 1. KATs

KAT_WRITE_SEEN = [(0, L(("Write", 1))), (1, L("Read")), (1, R(("Val", 1)))]
KAT_WRITE_UNSEEN = [(0, L(("Write", 1))), (1, L("Read")), (1, R(("Val", 0)))]
KAT_LONE_UNLOCK = [(0, L("Unlock"))]
KAT_UNLOCK_AND_FAILURE = [(0, L("Unlock")), (1, L("Lock")), (1, R("Busy"))]


def test_kat_pending_write_was_seen():
    """The crashed client's write took effect: the read saw it.  Root: the
    Write has no response, so Ok is assumed (node 1, state 1); the Read's
    Val 1 holds there (node 2), a leaf."""
    assert today(REG, KAT_WRITE_SEEN)[0] == "nonlin"
    st, nodes, path = pr.linearisable_pending(REG, KAT_WRITE_SEEN)
    assert (st, nodes) == ("lin", 2)
    assert path == [(0, ("Write", 1), "Ok", True), (1, "Read", ("Val", 1), False)]


def test_kat_pending_write_not_seen_yet():
    """Write assumed first (node 1), Read -> Val 0 fails at state 1 (node 2);
    back at the root the Read holds at state 0 (node 3), then the Write is
    assumed after it (node 4)."""
    st, nodes, path = pr.linearisable_pending(REG, KAT_WRITE_UNSEEN)
    assert (st, nodes) == ("lin", 4)
    assert path == [(1, "Read", ("Val", 0), False), (0, ("Write", 1), "Ok", True)]


def test_kat_nothing_allowed():
    """Unlock of the unlocked lock raises whatever the response: no symbol is
    allowed, the root has no child.  With no response in the history that is
    `every operation dropped`; beside a completed operation that fails it is
    the reference's root `any []`."""
    assert pr.allowed(LOCK, False, "Unlock") == []
    assert pr.linearisable_pending(LOCK, KAT_LONE_UNLOCK) == ("lin", 0, [])
    assert pr.linearisable_pending(LOCK, KAT_UNLOCK_AND_FAILURE) == ("nonlin", 1, [])
    assert today(LOCK, KAT_LONE_UNLOCK)[0] == "nonlin"


def test_replay_of_an_assumed_witness():
    m = TableModel.from_closures(REG["transition"], REG["postcondition"], REG["init"], REG["invs"], REG["resps"])
    ok = m.resps.index("Ok")
    assert replay_witness(m, KAT_WRITE_SEEN, [0, 1], None, assumed=[ok, None])
    assert replay_witness(m, KAT_WRITE_UNSEEN, [1, 0], None, assumed=[None, ok])
    # the Read's response cannot be assumed (its pid has one), Val 0 is not allowed for a Write,
    # the Read does not hold after the Write, and a Write left over is no leaf
    assert not replay_witness(m, KAT_WRITE_SEEN, [0, 1], None, assumed=[ok, m.resps.index(("Val", 1))])
    assert not replay_witness(m, KAT_WRITE_SEEN, [0, 1], None, assumed=[m.resps.index(("Val", 0)), None])
    assert not replay_witness(m, KAT_WRITE_UNSEEN, [0, 1], None, assumed=[ok, None])
    assert not replay_witness(m, KAT_WRITE_UNSEEN, [1], None, assumed=[None])
    lock = TableModel.from_closures(LOCK["transition"], LOCK["postcondition"], LOCK["init"], LOCK["invs"],
                                    LOCK["resps"], raises=OracleModelError)
    assert replay_witness(lock, KAT_LONE_UNLOCK, [], None, assumed=[])
    assert not replay_witness(lock, KAT_UNLOCK_AND_FAILURE, [], None, assumed=[])
    # (without `assumed`: today's rule, unchanged)
    assert not replay_witness(m, KAT_WRITE_SEEN, [0, 1])


# ----------------------------------------------------------- 2. the definition

N_DEF = 400
CRASH_DEF = 0.4


@functools.lru_cache(maxsize=None)
def crashed(name, clients, n_ops, p_bug, p_crash, n):
    model = {"register": REG, "lock": LOCK}[name]
    rng = random.Random(f"pending/{name}/{clients}x{n_ops}/{p_bug}/{p_crash}")
    return [pr.crash(tg.gen_history(model, rng, clients, n_ops, p_bug), rng, p_crash) for _ in range(n)]


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
    hists = crashed("register", 3, 8, 0.15, CRASH_DEF, N_DEF)
    assert len(hists) >= 400
    flipped = with_pending = 0
    for i, h in enumerate(hists):
        got = pr.linearisable_pending(REG, h)[0]
        assert got in ("lin", "nonlin")
        want = any(today(REG, c)[0] == "lin" for c in completions(REG, h))
        assert (got == "lin") == want, i
        with_pending += bool(pr.pending_invocations(h))
        flipped += got == "lin" and today(REG, h)[0] == "nonlin"
    print("histories with a pending invocation:", with_pending, "nonlin -> lin:", flipped)
    assert with_pending > N_DEF // 2 and flipped > 0


# ---------------------------------------------------------------- 3. monotone

@pytest.mark.parametrize("name", ["register", "lock"])
def test_monotone(name):
    """Where today's oracle says lin, the new rule says lin or (raise tables:
    an assumed operation can lead to a raising postcondition) error."""
    model = {"register": REG, "lock": LOCK}[name]
    seen = set()
    for h in crashed(name, 3, 8, 0.15, CRASH_DEF, N_DEF) + crashed(name, 4, 12, 0.05, 0.3, 200):
        if today(model, h)[0] == "lin":
            got = pr.linearisable_pending(model, h)[0]
            assert got in (("lin", "error") if name == "lock" else ("lin",)), h
            seen.add(got)
    print(name, sorted(seen))
    assert "lin" in seen


# ------------------------------------------------------- 4. complete histories

@pytest.mark.parametrize("name", ["register", "lock"])
def test_complete_histories_are_todays(name):
    model = {"register": REG, "lock": LOCK}[name]
    seen = set()
    for h in tg.gen_batch(model, "3x10", 300) + tg.gen_batch(model, "4x16", 100):
        assert not pr.pending_invocations(h)
        st, nodes, path = pr.linearisable_pending(model, h, tg.MAX_NODES)
        assert (st, nodes, ops(path)) == today(model, h, tg.MAX_NODES)
        assert not any(a for *_, a in path)
        seen.add(st)
    assert {"lin", "nonlin"} <= seen
