"""The CPU references of the table path's state memo (tests/tablememo.py)
against the literal oracle, and the known answers of the deep histories the
GPU tests run (tests/test_gpu_table_memo.py)."""

import random

import pytest

import tablegen as tg
import tablememo as tm
from linearise_lists import linearisable as oracle_linearisable


def generated(model, n):
    rng = random.Random(f"memo-host/{model['name']}")
    out = []
    for k in range(n):
        c, ops, p = ((4, 12, 0.05), (3, 10, 0.1), (2, 8, 0.05), (4, 12, 0.3))[k % 4]
        out.append(tg.gen_history(model, rng, c, ops, p))
    return out


@pytest.mark.parametrize("model", [tg.REGISTER, tg.LOCK], ids=["register", "lock"])
def test_helpers_equal_the_oracle(model):
    seen = set()
    for h in generated(model, 150) + [[]]:
        for max_nodes in (0, 7, 50):
            st, nd, path = oracle_linearisable(model["transition"], model["postcondition"], model["init"], h,
                                               max_nodes)
            seen.add(st)
            assert tm.exact_count(model, h, max_nodes) == (st, nd)
            for entries in (0, 2, 64):
                assert tm.memo_dfs(model, h, entries, max_nodes) == (st, nd, path), (h, max_nodes, entries)
    assert {"lin", "nonlin", "budget"} <= seen
    if model is tg.LOCK:
        assert "error" in seen


@pytest.mark.parametrize("name", sorted(tm.DEEP))
def test_deep_constants(name):
    model, hist, events, status, nodes, states = tm.DEEP[name]
    assert len(hist) == events
    stats = {}
    st, nd = tm.exact_count(model, hist, 0, stats)
    if name in tm.DEEP_EXACT:               # beyond u64: the device's answer is the u64 budget
        assert (st, nd) == ("nonlin", tm.DEEP_EXACT[name]) and nd > tm.U64
        assert tm.exact_count(model, hist, tm.U64) == ("budget", tm.U64)
    else:
        assert (st, nd) == (status, nodes)
    if states is not None:
        assert stats["states"] == states
    info = {}
    got = tm.memo_dfs(model, hist, 1024, 0, info)
    assert got[:2] == (status, nodes) and info["hits"] > 0 and info["iterations"] < 6000
    assert (got[2] != []) == (status == "lin")


def test_small_deep_rows_equal_the_oracle():
    for name in ("lock_deep_3_2", "lin_deep_4_3", "lock_deep_4_3"):
        model, hist, _, status, nodes, _ = tm.DEEP[name]
        st, nd, path = oracle_linearisable(model["transition"], model["postcondition"], model["init"], hist)
        assert (st, nd) == (status, nodes)
        for entries in (2, 16, 1024):
            assert tm.memo_dfs(model, hist, entries, 0) == (st, nd, path)


def test_budget_inside_a_hit():
    model, hist = tm.DEEP["reads_4x4"][:2]
    for max_nodes in (1000, 100000, 467007, 467008, 467009):
        info = {}
        want = ("budget", max_nodes) if max_nodes < 467008 else ("nonlin", 467008)
        assert tm.memo_dfs(model, hist, 1024, max_nodes, info)[:2] == want
        assert tm.exact_count(model, hist, max_nodes) == want
        assert info["hits"] > 0
