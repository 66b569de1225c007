"""The CPU references of the pending search's state memo (tests/pendingmemo.py)
against the literal rule (tests/pending_ref.py), and the known answers of the
deep crashed histories the GPU tests run (tests/test_gpu_table_pending_memo.py)."""

import functools

import pytest

import pending_ref as pr
import pendingmemo as pm
import tablegen as tg
from test_pending_host import CRASH_DEF, N_DEF, crashed

ENTRIES = (0, 2, 64, 1024)
LIMITS = (0, 7, 50)


@functools.lru_cache(maxsize=None)
def literal(name, max_nodes):
    model, hist = pm.DEEP[name][:2]
    return pr.linearisable_pending(model, hist, max_nodes)


def test_exact_count_equals_the_literal_rule_on_crashed_histories():
    hists = crashed("register", 3, 8, 0.15, CRASH_DEF, N_DEF)
    assert len(hists) == 400
    seen = set()
    for i, h in enumerate(hists + [[], [(0, tg.L(("Write", 1)))]]):
        for max_nodes in LIMITS:
            st, nd, path = pr.linearisable_pending(tg.REGISTER, h, max_nodes)
            seen.add(st)
            assert pm.exact_count_pending(tg.REGISTER, h, max_nodes) == (st, nd), (i, max_nodes)
            for entries in ENTRIES:
                assert pm.pending_memo_dfs(tg.REGISTER, h, entries, max_nodes) == (st, nd, path), (i, max_nodes, entries)
    assert {"lin", "nonlin", "budget"} <= seen


@pytest.mark.parametrize("name", pm.SMALL)
def test_small_rows_equal_the_literal_rule(name):
    model, hist, _, status, nodes, _ = pm.DEEP[name]
    assert literal(name, 0)[:2] == (status, nodes)
    for max_nodes in (0, 1, nodes // 2, nodes - 1, nodes, nodes + 1):
        st, nd, path = literal(name, max_nodes)
        assert pm.exact_count_pending(model, hist, max_nodes) == (st, nd)
        for entries in ENTRIES:
            assert pm.pending_memo_dfs(model, hist, entries, max_nodes) == (st, nd, path), (max_nodes, entries)
    if status == "lin":
        assert any(a for *_, a in literal(name, 0)[2])          # an assumed operation on the path


def test_the_root_rule():
    """No response event and no child at the root: every operation dropped."""
    h = [(0, tg.L("Unlock"))]
    assert pr.linearisable_pending(tg.LOCK, h) == ("lin", 0, [])
    assert pm.exact_count_pending(tg.LOCK, h) == ("lin", 0)
    for entries in ENTRIES:
        assert pm.pending_memo_dfs(tg.LOCK, h, entries, 0) == ("lin", 0, [])


@pytest.mark.parametrize("name", sorted(pm.DEEP))
def test_deep_constants(name):
    model, hist, events, status, nodes, states = pm.DEEP[name]
    assert len(hist) == events
    pending = pr.pending_invocations(hist)
    assert pending and not {hist[k][0] for k in pending} & {p for k, (p, _) in enumerate(hist) if k not in pending}
    stats = {}
    st, nd = pm.exact_count_pending(model, hist, 0, stats)
    if name in pm.DEEP_EXACT:               # beyond u64: the device's answer is the u64 budget
        assert (st, nd) == ("nonlin", pm.DEEP_EXACT[name]) and nd > pm.U64
        assert pm.exact_count_pending(model, hist, pm.U64) == ("budget", pm.U64)
    else:
        assert (st, nd) == (status, nodes)
    if states is not None:
        assert stats["states"] == states
    # (a table of 0, 2 or 64 entries walks most of a deep tree: only where that is affordable)
    for entries in ENTRIES if nodes < 100000 else (1024,):
        info = {}
        got = pm.pending_memo_dfs(model, hist, entries, 0, info)
        assert got[:2] == (status, nodes) and (info["hits"] > 0 or entries < 1024)
        assert (got[2] != []) == (status == "lin")
    assert info["iterations"] < 20000       # (entries 1024)
    if status == "lin":                     # the path replays under the literal rule's semantics
        assert any(a for *_, a in got[2]) and len(got[2]) == len([e for e in hist if e[1][0] == "L"])


def test_budget_inside_a_hit():
    model, hist, _, _, exact, _ = pm.DEEP["crashed_reads_4x4_1"]
    info = {}
    pm.pending_memo_dfs(model, hist, 1024, 0, info)
    before, count = max(info["trace"], key=lambda t: t[1])
    inside = before + count // 2
    assert count > 2 and before < inside < before + count
    for max_nodes in (inside, exact - 1, exact, exact + 1):
        info = {}
        want = ("budget", max_nodes) if max_nodes < exact else ("nonlin", exact)
        assert pm.pending_memo_dfs(model, hist, 1024, max_nodes, info)[:2] == want
        assert pm.exact_count_pending(model, hist, max_nodes) == want
        assert info["hits"] > 0
    # the plain walk agrees where it can be afforded
    assert pm.pending_memo_dfs(model, hist, 0, inside)[:2] == ("budget", inside)
