"""The keyed pending call's local mode (knob "kpending_local")
on the host: tests/kpendinglocal_ref.py against hand-derived known answers,
KeyedTableModel.split_history(pending=True) against the reference split, the
local verdict against the product's (tests/pending_ref.py on the product
closures) where the two must agree, the histories the product leaves `budget`,
a component with post_err, and complete histories against the check call's
local mode (tests/ktablelocal_ref.py)."""

import collections
import functools
import random

import pytest

import anyshape as an
import kpendinglocal_ref as klr
import ktablegen as kg
import ktablelocal_ref as lref
import pending_ref as pr
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from qsmd.models import KeyedTableModel, TableModel

L, R = tg.L, tg.R
REG, LOCK = tg.REGISTER, tg.LOCK
MAXN = tg.MAX_NODES


def W(k, v):
    return L((k, ("Write", v)))


def Rd(k):
    return L((k, "Read"))


def Val(v):
    return R(("Val", v))


@functools.lru_cache(maxsize=None)
def prod(name, K):
    return kg.product({"register": REG, "lock": LOCK}[name], K)


@functools.lru_cache(maxsize=None)
def keyed(name, K):
    c = {"register": REG, "lock": LOCK}[name]
    return KeyedTableModel(TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"],
                                                    c["resps"], raises=OracleModelError), K)


# ------------------------------------------------------------------ 1. KATs

KAT_SEEN = [(0, W(2, 1)), (1, Rd(2)), (1, Val(1))]
KAT_OTHER_KEY = [(0, W(2, 1)), (1, Rd(1)), (1, Val(1))]
KAT_TWO_KEYS = [(0, W(0, 1)), (1, W(7, 2)), (2, Rd(7)), (2, Val(2)), (2, Rd(0)), (2, Val(1))]
KAT_TWO_KEYS_SWAPPED = [(0, W(0, 1)), (1, W(7, 2)), (2, Rd(7)), (2, Val(1)), (2, Rd(0)), (2, Val(2))]
KAT_PENDING_ONLY = [(0, W(0, 1)), (1, W(3, 2)), (2, Rd(3))]
KAT_PENDING_PART_BESIDE_A_FAILING_KEY = [(0, W(0, 1)), (1, Rd(2)), (1, Val(3))]
KAT_LONE_PENDING_PID = [(0, W(1, 2)), (0, R("Ok")), (1, Rd(1)), (2, Rd(1)), (2, Val(2)), (0, Rd(3)), (0, Val(1))]
# (history, K, status, nodes), derived by hand per key:
#   SEEN                all on key 2: the assumed Write (1), the Read (2)
#   OTHER_KEY           key 1: the Read of 1 at 0 fails (1); key 2: the Write alone, assumed (1)
#   TWO_KEYS            keys 0 and 7: the assumed Write, then the Read (2 each)
#   TWO_KEYS_SWAPPED    keys 0 and 7: Write (1), Read fails (2), Read first fails (3) -- each
#   PENDING_ONLY        key 0: the Write (1); key 3: the Write (1), the Read assumed Val 2 (2)
#   PENDING_PART...     key 0: the Write (1), lin; key 2: the Read of 3 at 0 fails (1)
#   LONE_PENDING_PID    key 1: Write (1), p1's Read assumed Val 2 (2), p2's Read (3); key 3: Read of 1 at 0 fails (1)
KATS = [(KAT_SEEN, 4, "lin", 2), (KAT_OTHER_KEY, 4, "nonlin", 2), (KAT_TWO_KEYS, 8, "lin", 4),
        (KAT_TWO_KEYS_SWAPPED, 8, "nonlin", 6), (KAT_PENDING_ONLY, 4, "lin", 3),
        (KAT_PENDING_PART_BESIDE_A_FAILING_KEY, 4, "nonlin", 2), (KAT_PENDING_ONLY, 8, "lin", 3),
        (KAT_LONE_PENDING_PID, 4, "nonlin", 4), (KAT_LONE_PENDING_PID, 8, "nonlin", 4), ([], 4, "lin", 0)]
# rule 2 per part, on lock^4: a pending Unlock of an unlocked lock has no allowed symbol -- its part has no
# response and a root without a child (lin, 0 nodes); key 2's Lock of a free lock answered Busy fails (1)
KAT_RULE2 = [(0, L((1, "Unlock"))), (1, L((2, "Lock"))), (1, R("Busy"))]


def test_known_answers():
    for h, K, status, nodes in KATS:
        assert klr.check(REG, K, h) == (status, nodes), h
    assert klr.check(LOCK, 4, KAT_RULE2) == ("nonlin", 1)
    assert klr.check(LOCK, 4, KAT_RULE2[:1]) == ("lin", 0)
    # the parts themselves
    assert klr.split(REG, 8, KAT_TWO_KEYS) == [(0, [(0, W(0, 1)), (2, Rd(0)), (2, Val(1))]),
                                               (7, [(1, W(7, 2)), (2, Rd(7)), (2, Val(2))])]
    assert klr.split(REG, 4, KAT_LONE_PENDING_PID) == [(1, KAT_LONE_PENDING_PID[:5]), (3, KAT_LONE_PENDING_PID[5:])]
    # the product's answers: the verdicts are the same, the nodes are not
    assert [pr.linearisable_pending(prod("register", K), h)[:2] for h, K, _, _ in KATS[:4]] == [
        ("lin", 2), ("nonlin", 3), ("lin", 4), ("nonlin", 9)]


# ------------------------------------------- 2. the host split against the reference

def refused():
    """Histories that must stay on the product route, by reason."""
    long = an.exactly(tg.gen_batch(prod("register", 4), "6x24", 1)[0], 130)
    return {"too_long": [long],
            "symbol": [[(0, L((1, ("Write", 9)))), (0, R("Ok"))], [(0, W(1, 1)), (0, R("Nope"))],
                       [(0, L("Read")), (0, Val(0))]],
            "key": [[(0, W(4, 1)), (0, R("Ok"))], [(0, W(-1, 1))], [(0, L((True, "Read")))]],
            "lone_response": [[(0, R("Ok"))], [(0, W(0, 1)), (0, R("Ok")), (0, R("Ok"))],
                              [(1, W(0, 1)), (0, Val(0)), (0, Rd(0))]],
            "two_in_flight": [[(0, W(0, 1)), (0, W(1, 1)), (0, R("Ok")), (0, R("Ok"))],
                              [(0, W(0, 1)), (0, R("Ok")), (0, Rd(2)), (0, Rd(2))],     # after a pending one
                              [(0, Rd(3)), (0, Rd(3))]]}


@functools.lru_cache(maxsize=None)
def split_inputs():
    p = prod("register", 4)
    rng = random.Random("kpending-local/split")
    hists = [pr.crash(h, rng, 0.4) for h in tg.gen_batch(p, "4x16", 200) + tg.gen_batch(p, "3x10", 200)]
    hists += tg.gen_batch(p, "4x16", 50, seed=7)                    # complete
    for setting in an.ALL_SETTINGS:                                 # any-shape and shared-pid histories
        hists += an.batch(p, setting, 100)
    for group in refused().values():
        hists += group
    return hists


def test_refusal_reasons():
    assert set(refused()) == set(klr.REASONS)
    for reason, group in refused().items():
        for h in group:
            assert klr.refusal(REG, 4, h) == reason, h
            assert klr.split(REG, 4, h) is None and klr.check(REG, 4, h) is None


def test_split_history_pending_equals_the_reference_split():
    m = keyed("register", 4)
    hists = split_inputs()
    reasons = collections.Counter()
    split = pending_split = 0
    for h in hists:
        want = klr.split(REG, 4, h)
        assert m.split_history(h, pending=True) == want, h
        reasons[klr.refusal(REG, 4, h)] += 1
        if want is not None:
            split += 1
            pending_split += bool(pr.pending_invocations(h))
            # every event once, every part in history order
            assert sorted(e for _, sub in want for e in map(id, sub)) == sorted(map(id, h))
    print("split:", split, "with a pending invocation:", pending_split, "refused:", dict(reasons))
    assert all(reasons[r] for r in klr.REASONS) and split > 400 and pending_split > 150


def test_split_history_default_is_unchanged():
    m = keyed("register", 4)
    differs = 0
    for h in split_inputs():
        want = lref.split(REG, 4, h)
        assert m.split_history(h) == want and m.split_history(h, pending=False) == want, h
        differs += want != m.split_history(h, pending=True)
    assert differs > 150                # (the histories that end a pid on an invocation)


# ------------------------------------------------------------------ 3. locality

LOCAL_NODES = 200000
LOCALITY = [(4, "3x10", 400), (4, "4x16", 300), (2, "4x16", 300)]


@pytest.mark.parametrize("K,setting,n", LOCALITY)
def test_locality(K, setting, n):
    """The settings of test_ktable_pending_host.py::test_locality: the local
    verdict is the product's, no `budget` on either side, none left out."""
    model = prod("register", K)
    rng = random.Random(f"kloc/register/{K}/{setting}")
    seen, several = set(), 0
    for i, h in enumerate(tg.gen_batch(model, setting, n)):
        h = pr.crash(h, rng, 0.4)
        whole = pr.linearisable_pending(model, h, LOCAL_NODES)[0]
        local = klr.check(REG, K, h, LOCAL_NODES)
        assert local is not None, i
        assert whole != "budget" and local[0] != "budget", i
        assert local[0] == whole, (i, whole, local)
        seen.add(whole)
        several += len(klr.split(REG, K, h)) > 1 and bool(pr.pending_invocations(h))
    assert seen == {"lin", "nonlin"} and several > n // 3


# ------------------------------------------------------------ 4. budget decided

@functools.lru_cache(maxsize=None)
def crashed(name, K, setting, n, p_crash=0.3):
    p = prod(name, K)
    rng = random.Random(f"kpending-local/{name}/{K}/{setting}")
    return [pr.crash(h, rng, p_crash) for h in tg.gen_batch(p, setting, n)]


def test_decides_what_the_product_leaves_budget():
    hists = crashed("register", 8, "6x24", 60)
    pairs = collections.Counter()
    nodes = [0, 0]
    for i, h in enumerate(hists):
        whole, n_whole, _ = pr.linearisable_pending(prod("register", 8), h, MAXN)
        local, n_local = klr.check(REG, 8, h, MAXN)
        pairs[(whole, local)] += 1
        nodes[0] += n_whole
        nodes[1] += n_local
        if whole != "budget":
            assert local == whole, (i, whole, local)
    print("(product, per key):", dict(pairs), "nodes:", nodes)
    decided = sum(n for (whole, local), n in pairs.items() if whole == "budget" and local != "budget")
    assert decided >= 1
    assert sum(1 for h in hists if pr.pending_invocations(h)) > 20


# ------------------------------------------------------- 5. a post_err component

def test_post_err_component():
    hists = crashed("lock", 4, "4x16", 300)
    pairs = collections.Counter()
    for i, h in enumerate(hists):
        whole = pr.linearisable_pending(prod("lock", 4), h, MAXN)[0]
        local = klr.check(LOCK, 4, h, MAXN)[0]
        pairs[(whole, local)] += 1
        if not {whole, local} & {"error", "budget"}:
            assert local == whole, (i, whole, local)
    print("(product, per key):", dict(pairs))
    assert pairs[("lin", "lin")] > 50 and pairs[("nonlin", "nonlin")] > 30 and pairs[("error", "error")] > 30
    # lin against the rest does not move
    assert all(n == 0 for (a, b), n in pairs.items() if (a == "lin") != (b == "lin") and "budget" not in (a, b))


# ------------------------------------------------------- 6. complete histories

@pytest.mark.parametrize("name,K", [("register", 4), ("lock", 4), ("register", 8)])
def test_complete_histories_equal_the_check_calls_local_mode(name, K):
    c = {"register": REG, "lock": LOCK}[name]
    seen = set()
    for h in tg.gen_batch(prod(name, K), "4x16", 200) + tg.gen_batch(prod(name, K), "3x10", 100):
        assert not pr.pending_invocations(h)
        got = klr.check(c, K, h, MAXN)
        assert got is not None and got == lref.check(c, K, h, MAXN)
        assert klr.split(c, K, h) == lref.split(c, K, h)
        seen.add(got[0])
    assert {"lin", "nonlin"} <= seen
