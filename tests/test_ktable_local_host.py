"""The keyed model's local mode on the host (no GPU): KeyedTableModel.split_history
against the literal restatement (tests/ktablelocal_ref.py), and the theorem the
mode rests on -- a splittable history is linearisable on the product model
exactly when every key's part is -- on the literal oracle."""

import functools
import random

import pytest

import ktablegen as kg
import ktablelocal_ref as ref
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd.models import KeyedTableModel, TableModel

COMPONENTS = {"register": tg.REGISTER, "lock": tg.LOCK}
THEOREM_MAX_NODES = 200_000


@functools.lru_cache(maxsize=None)
def keyed(name, K):
    c = COMPONENTS[name]
    comp = TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                    raises=OracleModelError)
    return KeyedTableModel(comp, K)


def batch(name, K, clients, ops, p_bug, n, seed=tg.SEED):
    """tablegen's generator under the project's seed.  The theorem tests need
    the product oracle to decide every history within THEOREM_MAX_NODES; that
    depends on the batch alone (about one 4-key history in 600 at p_bug 0.05
    does not, under other seeds), not on anything under test."""
    p = kg.product(COMPONENTS[name], K)
    rng = random.Random(f"{seed}/{name}/{K}/{clients}x{ops}/{p_bug}")
    return p, [tg.gen_history(p, rng, clients, ops, p_bug) for _ in range(n)]


def same_split(name, K, h):
    got, want = keyed(name, K).split_history(h), ref.split(COMPONENTS[name], K, h)
    assert got == want, h
    return got


# ------------------------------------------------------------ split_history

@pytest.mark.parametrize("name,K,clients,ops", [("register", 2, 4, 16), ("register", 8, 6, 24), ("lock", 4, 3, 10)])
def test_split_history_on_generated_batches(name, K, clients, ops):
    _, hists = batch(name, K, clients, ops, 0.05, 200)
    for h in hists:
        parts = same_split(name, K, h)
        assert parts is not None                      # the generator's histories are complete
        assert [k for k, _ in parts] == sorted({x[0] for _, (kind, x) in h if kind == "L"})
        assert sum(len(s) for _, s in parts) == len(h)
        for k, sub in parts:                          # history order kept, events unchanged
            it = iter(h)
            assert all(e in it for e in sub)
            assert all(x[0] == k for _, (kind, x) in sub if kind == "L")


W = ("Write", 1)


def test_split_history_edge_cases():
    inv = lambda p, k, i=W: (p, ("L", (k, i)))        # noqa: E731
    ok = lambda p: (p, ("R", "Ok"))                   # noqa: E731
    # not splittable
    assert same_split("register", 4, [inv(0, 1), ok(0), inv(1, 2)]) is None               # a pending invocation
    assert same_split("register", 4, [ok(0), inv(0, 1), ok(0)]) is None                   # a lone response
    assert same_split("register", 4, [inv(0, 1), ok(0), ok(0)]) is None
    assert same_split("register", 4, [inv(0, 1), inv(0, 2), ok(0), ok(0)]) is None        # a shared pid, overlapping
    assert same_split("register", 4, [inv(0, 4), ok(0)]) is None                          # key >= n_keys
    assert same_split("register", 4, [inv(0, 1, ("Write", 9)), ok(0)]) is None            # unknown invocation
    assert same_split("register", 4, [inv(0, 1), (0, ("R", "Nope"))]) is None             # unknown response
    too_long = [e for p in range(65) for e in (inv(p, 0), ok(p))]
    assert len(too_long) == 130 and same_split("register", 4, too_long) is None
    # splittable
    assert same_split("register", 4, []) == []
    turns = [inv(0, 3), ok(0), inv(0, 1), ok(0), inv(0, 3), ok(0)]                        # a shared pid strictly in turn
    assert same_split("register", 4, turns) == [(1, turns[2:4]), (3, turns[0:2] + turns[4:6])]
    one = [inv(0, 2), inv(1, 2), ok(1), ok(0)]
    assert same_split("register", 4, one) == [(2, one)]                                   # one key only
    assert same_split("register", 1, [inv(0, 0), ok(0)]) == [(0, [inv(0, 0), ok(0)])]
    each = [inv(p, p) for p in range(8)] + [ok(p) for p in reversed(range(8))]
    assert same_split("register", 8, each) == [(p, [inv(p, p), ok(p)]) for p in range(8)]  # every operation its own key
    # a response goes with its pid's invocation, whatever lies between
    mixed = [inv(0, 1), inv(1, 0), ok(0), inv(0, 0), ok(1), ok(0)]
    assert same_split("register", 2, mixed) == [(0, [mixed[1], mixed[3], mixed[4], mixed[5]]),
                                                (1, [mixed[0], mixed[2]])]


# -------------------------------------------------------------- the theorem

def product_verdicts(p, hists):
    return [oracle_linearisable(p["transition"], p["postcondition"], p["init"], h, THEOREM_MAX_NODES)[0]
            for h in hists]


@pytest.mark.parametrize("K,p_bug", [(2, 0.03), (4, 0.05)])
def test_local_verdict_equals_the_product_verdict(K, p_bug):
    p, hists = batch("register", K, 4, 16, p_bug, 600)
    want = product_verdicts(p, hists)
    got = [ref.check(tg.REGISTER, K, h, THEOREM_MAX_NODES) for h in hists]
    assert all(g is not None for g in got)
    assert "budget" not in want and "budget" not in {g[0] for g in got}
    assert [g[0] for g in got] == want
    assert {"lin", "nonlin"} <= set(want)


def test_with_post_err_lin_on_one_side_iff_lin_on_the_other():
    p, hists = batch("lock", 4, 4, 16, 0.05, 600)
    want = product_verdicts(p, hists)
    got = [ref.check(tg.LOCK, 4, h, THEOREM_MAX_NODES)[0] for h in hists]
    assert "budget" not in want and "budget" not in got
    assert [g == "lin" for g in got] == [w == "lin" for w in want]
    assert {"lin", "nonlin", "error"} <= set(want)
