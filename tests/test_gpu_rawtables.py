"""GPU parity of every table search on random raw tables whose responses move
the state (tests/rawtables.py): csrc/table.hip, csrc/wtable.hip,
csrc/ktable.hip, csrc/tpending.hip, csrc/kpending.hip with their memo, explain
and local-mode variants, against the literal restatements
(oracle/linearise_lists.py, tests/pending_ref.py, tests/explain_ref.py,
tests/ktablelocal_ref.py) run with closures that read the raw arrays.

The named models of the other modules all have an identity ``on_resp``, one
allowed response per (state, invocation) and no table bit at or above
``n_resp``; these are the tests in which the fourth table, words of ``post``
with several bits, post_err overlapping post and garbage above ``n_resp``
decide verdicts (tests/test_rawtables_host.py asserts that they do, on the
reference alone).  Every comparison is exact -- status, node count, witness
operations, assumed bytes, totals -- and no history is left out: the device
runs with the reference's max_nodes, and a `budget` verdict must match with
nodes == max_nodes."""

import numpy as np
import pytest

import anyshape as an
import ktablelocal_ref as kref
import pending_ref as pr
import rawtables as rt
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import filter1, find_response, take_invocations
from qsmd import codec, device
from qsmd.linearisability import explain_batch, tuple_or
from qsmd.models import KeyedTableModel, WideTableModel
from test_gpu_ktable import run_host as run_host5
from test_gpu_ktable_local import CODE, assert_equal
from test_gpu_ktable_pending import assert_results as assert_pending5
from test_gpu_ktable_pending import run_device as run_pending_device5
from test_gpu_ktable_pending import run_host as run_pending_host5
from test_gpu_table import EXH, MAXN, assert_results, run_device, witness_path
from test_gpu_table import run_host as run_host3
from test_gpu_table_pending import assert_results as assert_pending3
from test_gpu_table_pending import budget_knob, levels, same
from test_gpu_table_pending import run_device as run_pending_device3
from test_gpu_table_pending import run_host as run_pending_host3
from test_gpu_wtable import run_host as run_host4

pytestmark = pytest.mark.gpu

L, R = tg.L, tg.R
assert MAXN == rt.MAX_NODES
NARROW = [n for n in rt.NARROW if n != "c_odd"]
SHAPES = NARROW + list(rt.WIDE) + list(rt.KEYED)
SETTINGS = list(rt.BATCHES)
BUDGETS = (256, 0, 4)


@pytest.fixture(scope="module")
def ctx():
    """This module's own context (a keyed table, once set, cannot be taken
    away, and the session's context must stay without one: see
    test_gpu_ktable.py)."""
    c = device.Context(0, time_limit_ms=60000)
    yield c
    c.close()


def run_host(ctx, m, hists, model0=None):
    if isinstance(m, KeyedTableModel):
        return run_host5(ctx, m, hists, model0)
    return (run_host4 if isinstance(m, WideTableModel) else run_host3)(ctx, m, hists, model0)


def equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def check_both(ctx, name, hists, ref, budgets=BUDGETS):
    """The check call through the host and the device entry against the
    reference, in both passes; the count of pass 2 is the predicted one."""
    m, model0 = rt.model(name), rt.model0_of(name)
    for budget in budgets:
        with budget_knob(ctx, budget):
            batch, st, nd, w, tot = run_host(ctx, m, hists, model0)
            pass2 = ctx.table_pass2()
            assert_results(m, hists, ref, st, nd, w, batch.hdr, model0, tot)
            assert pass2 == rt.pass2_expected(ref, budget), budget
            dev = run_device(ctx, batch.hdr, batch.events, m.pack_model0(model0, {}), model_id=m.model_id)
            assert equal((st, nd, w, tot), dev), budget
    return batch, st, nd, w, tot


# ------------------------------------------------------------- 1. the check call

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", SHAPES)
def test_check_call(ctx, name, setting):
    assert ctx.get_param("table_budget") == 256
    hists, ref = rt.check_case(name, setting)
    check_both(ctx, name, hists, ref)
    assert not ctx.timed_out()


@pytest.mark.parametrize("twin", list(rt.TWINS))
def test_wide_twins_equal_the_narrow_tables(ctx, twin):
    narrow, wide = rt.model(rt.TWINS[twin]), rt.model(twin)
    assert isinstance(wide, WideTableModel) and not isinstance(narrow, WideTableModel)
    ctx.set_table(narrow)
    ctx.set_wide_table(wide)
    for setting in SETTINGS:
        hists, ref = rt.check_case(rt.TWINS[twin], setting)
        batch = codec.encode(narrow, hists)
        assert not batch.encode_errors and (batch.hdr["model_id"] == 3).all()
        hdr4 = batch.hdr.copy()
        hdr4["model_id"] = 4
        for budget in BUDGETS:
            with budget_knob(ctx, budget):
                a = ctx.check_arrays(3, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
                b = ctx.check_arrays(4, hdr4, batch.events, None, EXH, MAXN, witness=True)
                assert ctx.table_pass2() == rt.pass2_expected(ref, budget)
            assert equal(a, b)
        assert_results(wide, hists, ref, b[0], b[1], b[2], hdr4, None, b[3])
    assert not ctx.timed_out()


def on_key_0(hists):
    return [[(p, (k, (0, x)) if k == "L" else (k, x)) for p, (k, x) in h] for h in hists]


def test_one_key_equals_model_3(ctx):
    narrow, keyed = rt.model("n_r32"), rt.model("k_one")
    assert keyed.component is narrow and keyed.n_keys == 1
    for setting in SETTINGS:
        hists, ref = rt.check_case("n_r32", setting)
        for budget in BUDGETS:
            with budget_knob(ctx, budget):
                a = run_host3(ctx, narrow, hists)[1:]
                b = run_host5(ctx, keyed, on_key_0(hists))[1:]
            assert equal(a, b)
        # and the pending entries
        hists, ref = rt.crash_case("n_r32", setting)
        a = run_pending_host3(ctx, narrow, hists)[1:]
        b = run_pending_host5(ctx, keyed, on_key_0(hists))[1:]
        assert same(a, b)
    assert not ctx.timed_out()


# ---------------------------------------------------------------------- 2. memos

@pytest.mark.parametrize("name", ["n_deep", "n_1inv", "w_n_deep", "w_256", "k_deep"])
def test_memo(ctx, name):
    """The state memo of pass 2 (64 entries): every array equal to the plain
    call's and to the reference's.  The key is (remaining events, state), the
    state after a response that moved it."""
    m, model0 = rt.model(name), rt.model0_of(name)
    knob = "ktable_memo" if isinstance(m, KeyedTableModel) else "table_memo"
    hits = 0
    for setting in SETTINGS:
        hists, ref = rt.check_case(rt.TWINS.get(name, name), setting)
        for budget in (256, 4):
            with budget_knob(ctx, budget):
                plain = run_host(ctx, m, hists, model0)
                assert ctx.table_memo_hits() == 0
                ctx.set_param(knob, 64)
                try:
                    batch, st, nd, w, tot = run_host(ctx, m, hists, model0)
                    hits_here = ctx.table_memo_hits()
                    pass2 = ctx.table_pass2()
                    dev = run_device(ctx, batch.hdr, batch.events, m.pack_model0(model0, {}), model_id=m.model_id)
                finally:
                    ctx.set_param(knob, 0)
            assert equal((st, nd, w, tot), plain[1:]) and equal((st, nd, w, tot), dev)
            assert_results(m, hists, ref, st, nd, w, batch.hdr, model0, tot)
            assert pass2 == rt.pass2_expected(ref, budget)
            print(name, setting, budget, "pass 2:", pass2, "memo hits:", hits_here)
            if setting == "6x24":
                assert hits_here > 0, budget
            hits += hits_here
    assert hits > 0 and not ctx.timed_out()


# -------------------------------------------------------------------- 3. explain

def stuck_reference(c, hist, path, model):
    """The operations that could not follow the reported path: the candidates
    of the node at its end (the reference's takeInvocations / filter1 /
    findResponse on the remaining events) and why each is no way on."""
    def without_invocation(es, pid):
        return filter1(lambda e: not (e[0] == pid and e[1][0] == "L"), es)
    es = list(hist)
    for pid, _, _ in path:
        es = find_response(pid, without_invocation(es, pid))[0][1]
    out = []
    for pid, inv in take_invocations(es):
        found = find_response(pid, without_invocation(es, pid))
        if not found:
            out.append((pid, inv, None, "no response"))
            continue
        resp = found[0][0]
        try:
            outcome = "passes" if c["postcondition"](model, inv, resp) else "postcondition false"
        except OracleModelError:
            outcome = "raises"
        out.append((pid, inv, resp, outcome))
    return out


@pytest.mark.parametrize("setting", ["3x10", "6x24"])
@pytest.mark.parametrize("name", ["n_r32", "n_deep", "w_3w", "k_deep"])
def test_explain(ctx, name, setting):
    m, model0, c = rt.model(name), rt.model0_of(name), rt.closures(name)
    hists, ref = rt.explain_case(name, setting)
    assert [r[:2] for r in ref] == [r[:2] for r in rt.check_case(name, setting)[1]]
    for budget in BUDGETS:
        with budget_knob(ctx, budget):
            res = explain_batch(m, hists, model0, max_nodes=MAXN, ctx=ctx)
            assert ctx.table_pass2() == rt.pass2_expected(ref, budget)
        for i, (h, (st_r, nd_r, ops_r, model_r)) in enumerate(zip(hists, ref)):
            got = (res.verdict(i), int(res.nodes[i]), witness_path(h, res.path_of(i)), int(res.depth[i]),
                   tuple_or(res.state_of(i)))
            assert got == (st_r, nd_r, ops_r, len(ops_r), tuple_or(model_r)), (budget, i)
            if budget == 256:
                e = res.explanation(i)
                assert (e.status, e.prefix, tuple_or(e.model)) == (st_r, ops_r, tuple_or(model_r)), i
                assert e.stuck == stuck_reference(c, h, ops_r, model_r), i
    seen = {r[0] for r in ref}
    assert {"lin", "nonlin"} <= seen and any(r[0] != "lin" and len(r[2]) > 0 for r in ref)
    assert not ctx.timed_out()


# -------------------------------------------------------------------- 4. pending

def pending_both(ctx, name, hists, ref, budgets=BUDGETS, memo=0):
    """The pending entry of a narrow or a keyed shape, host and device entry,
    against pending_ref; with `memo`, also equal to the plain call's arrays.
    Returns the last host result and the memo hits."""
    m, model0 = rt.model(name), rt.model0_of(name)
    keyed = isinstance(m, KeyedTableModel)
    hits = 0
    for budget in budgets:
        with budget_knob(ctx, budget):
            if keyed:
                batch, *got = run_pending_host5(ctx, m, hists, model0)
                pass2 = ctx.table_pass2()
                assert_pending5(m, hists, ref, *got[:4], batch.hdr, got[4], MAXN, model0)
                dev = run_pending_device5(ctx, batch.hdr, batch.events, m.pack_model0(model0, {}))
            else:
                batch, *got = run_pending_host3(ctx, m, hists)
                pass2 = ctx.table_pass2()
                assert_pending3(m, hists, ref, *got[:4], batch.hdr, got[4])
                dev = run_pending_device3(ctx, batch.hdr, batch.events)
            assert same(tuple(got), dev), budget
            assert pass2 == rt.pass2_expected(ref, budget), budget
            if memo:
                assert ctx.pending_memo_hits() == 0
                ctx.set_param("pending_memo", memo)
                try:
                    _, *again = run_pending_host3(ctx, m, hists)
                    hits += ctx.pending_memo_hits()
                    assert ctx.table_pass2() == pass2
                    dev = run_pending_device3(ctx, batch.hdr, batch.events)
                finally:
                    ctx.set_param("pending_memo", 0)
                assert same(tuple(again), tuple(got)) and same(tuple(again), dev), budget
    return batch, got, hits


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", NARROW + list(rt.KEYED))
def test_pending(ctx, name, setting):
    hists, ref = rt.crash_case(name, setting)
    pending_both(ctx, name, hists, ref)
    assert not ctx.timed_out()


@pytest.mark.parametrize("name", ["n_deep", "n_1inv"])
def test_pending_memo(ctx, name):
    hits = 0
    for setting in SETTINGS:
        hists, ref = rt.crash_case(name, setting)
        hits_here = pending_both(ctx, name, hists, ref, memo=64)[2]
        print(name, setting, "pending memo hits:", hits_here)
        hits += hits_here
    assert hits > 0 and not ctx.timed_out()


@pytest.mark.parametrize("k", [20, 40, 100])
@pytest.mark.parametrize("name", ["n_1inv", "n_r2"])
def test_depth_of_one_level_per_invocation(ctx, name, k):
    """k pids with a pending invocation each -- at every one several symbols
    are allowed and the allowed word carries bits at and above n_resp -- then
    one completed operation whose answer the walk's end allows (or does not):
    k + 1 levels on k + 2 events; the width class filled; invocations only."""
    m, sp, t = rt.model(name), rt.spec(name), rt.tables_of(name)
    ev = {20: 32, 40: 64, 100: 128}[k]
    assert sp.high == "post" and all(int(w) >> sp.nr for w in m.post.ravel())
    walk, states = rt.pending_walk(name, ev)
    head, state = walk[:k], states[k]
    last = next(i for i in range(sp.ni) if rt.allowed_bits(name, state, i))
    a = rt.allowed_bits(name, state, last)
    good = (a & -a).bit_length() - 1
    bad = next((r for r in range(sp.nr) if not (a >> r) & 1 and not t.err[state, last, r]), None)
    h = head + [(k, L(last)), (k, R(good))]
    assert len(h) == k + 2 and k + 1 > len(h) // 2
    # the width class filled: more pending invocations between the last invocation and its response
    # (n_ev - 1 levels), and a history of pending invocations only (n_ev levels: no terminator)
    more = rt.pending_walk(name, ev - len(h), start=int(t.on_resp[t.on_inv[state, last], good]), first_pid=k + 1)[0]
    h2 = h[:-1] + more + h[-1:]
    h3 = walk
    assert len(h2) == len(h3) == ev
    hists = [h, h2, h3] + ([head + [(k, L(last)), (k, R(bad))]] if bad is not None else [])
    c = rt.closures(name)
    ref = [pr.linearisable_pending(c, x, MAXN) for x in hists]
    assert (ref[0][0], ref[0][1], len(ref[0][2])) == ("lin", k + 1, k + 1)
    assert (ref[1][0], ref[1][1], len(ref[1][2])) == ("lin", ev - 1, ev - 1)
    assert (ref[2][0], ref[2][1], len(ref[2][2])) == ("lin", ev, ev)
    batch, got, _ = pending_both(ctx, name, hists, ref)
    wit, asm = levels(batch.hdr, 0, got[2], got[3])
    assert wit == list(range(k + 1)) and asm[-1] is None and all(x is not None and x < sp.nr for x in asm[:-1])
    assert len(levels(batch.hdr, 2, got[2], got[3])[0]) == ev
    assert not ctx.timed_out()


# ----------------------------------------------------------------- 5. local mode

@pytest.mark.parametrize("name", ["k_deep", "k_odd", "k_max"])
def test_local_mode(ctx, name):
    """Knob "ktable_local": every key's part searched on its own from that
    key's model0 state, the status of the lowest failing key, the node counts
    summed (include/qsmd.h), against the restatement with the component's
    closures."""
    comp, K, model0 = rt.KEYED[name]
    m, c = rt.model(name), rt.closures(comp)
    for setting in SETTINGS:
        hists, product_ref = rt.check_case(name, setting)
        batch = codec.encode(m, hists, model0)
        assert not batch.encode_errors
        want = kref.check_arrays(c, K, batch.hdr, batch.events, MAXN, model0)
        assert all(w is not None for w in want)
        assert want == [kref.check(c, K, h, MAXN, model0) for h in hists]
        want = [(CODE[s], n) for s, n in want]
        if ctx.keyed_table is not m:
            ctx.set_keyed_table(m)
        for budget in BUDGETS:
            with budget_knob(ctx, budget):
                ctx.set_param("ktable_local", 1)
                try:
                    st, nd, _, tot = ctx.check_arrays(5, batch.hdr, batch.events, m.pack_model0(model0, {}), EXH, MAXN)
                    split = ctx.ktable_local_last()
                finally:
                    ctx.set_param("ktable_local", 0)
            assert_equal(want, len(hists), st, nd, tot, split)
        # the verdicts agree with the product search wherever both decide
        for (s, _), r in zip(want, product_ref):
            assert s == CODE[r[0]] or r[0] == "budget" or s == CODE["budget"] or {s, CODE[r[0]]} <= {0, 2}
    assert not ctx.timed_out()


# ------------------------------------------------------------------ 6. any shape

@pytest.mark.parametrize("setting", list(rt.ANY_SETTINGS))
@pytest.mark.parametrize("name", ["n_r32", "w_3w", "k_odd"])
def test_anyshape(ctx, name, setting):
    hists, ref, pending_ref = rt.anyshape_case(name, setting)
    feats = set()
    for s in rt.ANY_SETTINGS:
        feats |= set().union(*(an.census(h) for h in rt.anyshape_case(name, s)[0]))
    assert feats == set(an.FEATURES)
    check_both(ctx, name, hists, ref)
    if name != "w_3w":
        pending_both(ctx, name, hists, pending_ref)
    assert not ctx.timed_out()


# ------------------------------------------- 7. replacing tables between calls

def test_replacing_tables_between_calls(ctx):
    """A smaller table after a larger one: nothing of the larger one's
    leftovers (LDS, the device blob) is read."""
    for name in ("n_max", "n_one", "n_r2", "n_one", "n_max", "n_r2"):
        hists, ref = rt.check_case(name, "4x16")
        check_both(ctx, name, hists, ref, budgets=(256,))
        hists, ref = rt.crash_case(name, "4x16")
        pending_both(ctx, name, hists, ref, budgets=(256,))
    for name in ("k_max", "k_odd", "k_one", "k_max", "k_one", "k_odd"):
        hists, ref = rt.check_case(name, "3x10")
        check_both(ctx, name, hists, ref, budgets=(256,))
        hists, ref = rt.crash_case(name, "3x10")
        pending_both(ctx, name, hists, ref, budgets=(256,))
    assert not ctx.timed_out()
