"""GPU tests of the table path's exact-count state memo (csrc/table.hip, knob
"table_memo"): pass 2 records every failed subtree under its
full key (remaining events, state) and counts it on the next visit, so
status, node count and witness stay the reference's while a tree of 1e18
nodes is decided in a few thousand iterations.

The references are tests/tablememo.py (the exact count by recursion over the
states, and the literal mirror of the kernel's step) and, for generated
batches, the literal oracle as in test_gpu_table.py."""

import random

import numpy as np
import pytest

import tablegen as tg
import tablememo as tm
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device
from qsmd.linearisability import ModelError, linearisable, linearisable_batch, replay_witness
from qsmd.models import TableModel
from test_gpu_table import (EXH, MAXN, assert_results, oracle, parity_case, run_device, run_host, seq_history,
                            table, witness_path)

pytestmark = pytest.mark.gpu

U64 = tm.U64
DEEP_LIMIT_MS = 5000        # a cap, not a measurement: a broken memo ends as BUDGET instead of hanging


class knobs:
    """Set table knobs / the time limit; restore all of them on exit."""

    def __init__(self, ctx, time_limit_ms=None, **params):
        self.ctx, self.params, self.ms = ctx, params, time_limit_ms

    def __enter__(self):
        self.saved = {k: self.ctx.get_param(k) for k in ("table_memo", "table_memo_grid", "table_budget")}
        if self.ms is not None:
            self.ctx.set_time_limit_ms(self.ms)
        for k, v in self.params.items():
            self.ctx.set_param(k, v)
        return self.ctx

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.ctx.set_param(k, v)
        self.ctx.set_time_limit_ms(60000)
        return False


def witness_of(hdr, wit, i):
    o, n = int(hdr[i]["ev_off"]), int(hdr[i]["n_ev"])
    w = []
    for x in wit[o:o + n]:
        if x == codec.WITNESS_END:
            break
        w.append(int(x))
    return w


def check_deep(ctx, names, entries, max_nodes=0, want=None, relabel=None):
    """The DEEP rows `names`, one batch per model, through both entries."""
    for model in (tg.REGISTER, tg.LOCK):
        rows = [n for n in names if tm.DEEP[n][0] is model]
        if not rows:
            continue
        m = table(model["name"])
        hists = [tm.DEEP[n][1] for n in rows]
        if relabel:
            hists = [[(relabel + p, e) for p, e in h] for h in hists]
        with knobs(ctx, DEEP_LIMIT_MS, table_memo=entries):
            batch, st, nd, w, tot = run_host(ctx, m, hists, max_nodes=max_nodes, flags=EXH)
            hits = ctx.table_memo_hits()
            timed = ctx.timed_out()
            st2, nd2, w2, tot2 = run_device(ctx, batch.hdr, batch.events, max_nodes=max_nodes)
            hits2 = ctx.table_memo_hits()
        assert not timed
        assert np.array_equal(st, st2) and np.array_equal(nd, nd2) and np.array_equal(w, w2) and tot == tot2
        for i, n in enumerate(rows):
            exp = want[n] if want else tm.DEEP[n][3:5]
            got = (codec.STATUS_NAMES[int(st[i])], int(nd[i]))
            print(n, entries, got, exp)
            assert got == tuple(exp), (n, got, exp)
            if got[0] == "lin":
                wit = witness_of(batch.hdr, w, i)
                assert replay_witness(m, hists[i], wit, None), n
                assert witness_path(hists[i], wit) == [(p + (relabel or 0), a, b) for p, a, b in
                                                       tm.memo_dfs(model, tm.DEEP[n][1], entries, max_nodes)[2]]
        assert tot["nodes"] == int(np.sum(nd, dtype=np.uint64))
        assert hits > 0 and hits2 > 0, (hits, hits2)


# ------------------------------------------------------------------- 1. the knob

def test_knob(ctx):
    m = table("register")
    hists, ref = parity_case("register", "3x10")
    assert ctx.get_param("table_memo") == 0 and ctx.get_param("table_memo_grid") == 0
    before = run_host(ctx, m, hists)
    with knobs(ctx):
        ctx.set_param("table_memo", 64)
        ctx.set_param("table_memo", 0)
        after = run_host(ctx, m, hists)
        assert ctx.table_memo_hits() == 0
        assert all(np.array_equal(x, y) for x, y in zip(before[1:4], after[1:4])) and before[4] == after[4]
        for bad in (3, 1, 1 << 21):
            with pytest.raises(device.DeviceError) as e:
                ctx.set_param("table_memo", bad)
            assert "failed (-1)" in str(e.value)
            assert ctx.get_param("table_memo") == 0
        ctx.set_param("table_memo", 1 << 20)        # (accepted; no call made with it)
        ctx.set_param("table_memo", 2)
        batch, st, nd, w, tot = run_host(ctx, m, hists[:64])
        assert_results(m, hists[:64], ref[:64], st, nd, w, batch.hdr, None, tot)
    assert ctx.get_param("table_memo") == 0


# ---------------------------------------------------------------- 2. deep cases

def test_deep_cases(ctx):
    check_deep(ctx, sorted(tm.DEEP), 1024)


@pytest.mark.parametrize("name", sorted(tm.DEEP))
def test_deep_linearisable_call(ctx, name):
    model, hist, _, status, _, _ = tm.DEEP[name]
    m = table(model["name"])
    with knobs(ctx, DEEP_LIMIT_MS):
        if status == "error":
            with pytest.raises(ModelError):
                linearisable(m.transition, m.postcondition, model["init"], hist, ctx=ctx, table_memo=1024)
        elif status == "budget":        # more than 2^64 - 1 nodes: undecided
            res = linearisable_batch(m, [hist], ctx=ctx, table_memo=1024)
            assert res.verdict(0) == "budget" and int(res.nodes[0]) == U64
        else:
            assert linearisable(m.transition, m.postcondition, model["init"], hist, ctx=ctx,
                                table_memo=1024) == (status == "lin")
        assert ctx.get_param("table_memo") == 0 and not ctx.timed_out()
        # (a search within pass 1's budget never reaches the memo pass: lock_deep_3_2 alone)
        assert (ctx.table_memo_hits() > 0) == (tm.DEEP[name][4] > ctx.get_param("table_budget"))


# --------------------------------------------------------------- 3. lossy tables

@pytest.mark.parametrize("entries", [2, 16])
def test_lossy_tables(ctx, entries):
    check_deep(ctx, ["reads_4x4", "lin_deep_4_3", "lock_deep_4_3"], entries)


# -------------------------------------------------------- 4. budget inside a hit

@pytest.mark.parametrize("name,max_nodes,want", [
    ("reads_4x4", 1000, ("budget", 1000)), ("reads_4x4", 100000, ("budget", 100000)),
    ("reads_4x4", 467007, ("budget", 467007)), ("reads_4x4", 467008, ("nonlin", 467008)),
    ("reads_4x4", 467009, ("nonlin", 467008)), ("lin_deep_4_3", 52304, ("budget", 52304)),
    ("lin_deep_4_3", 52305, ("lin", 52305)), ("reads_4x8", 10**9, ("budget", 10**9))])
def test_budget_inside_a_hit(ctx, name, max_nodes, want):
    assert tm.exact_count(tm.DEEP[name][0], tm.DEEP[name][1], max_nodes) == want
    check_deep(ctx, [name], 1024, max_nodes=max_nodes, want={name: want})


# ---------------------------------------------------------- 5. whole-path parity

@pytest.mark.parametrize("setting", ["3x10", "4x16"])
@pytest.mark.parametrize("name", ["register", "lock"])
def test_whole_path_parity(ctx, name, setting):
    m = table(name)
    hists, ref = parity_case(name, setting)
    default = ctx.get_param("table_budget")
    for budget, sizes in ((1, (2, 64, 4096)), (default, (64,))):
        with knobs(ctx, table_budget=budget):
            run_host(ctx, m, hists)
            pass2_off = ctx.table_pass2()
            assert ctx.table_memo_hits() == 0
            for entries in sizes:
                ctx.set_param("table_memo", entries)
                batch, st, nd, w, tot = run_host(ctx, m, hists)
                assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)
                assert ctx.table_memo_hits() > 0 and ctx.table_pass2() == pass2_off
                st2, nd2, w2, tot2 = run_device(ctx, batch.hdr, batch.events)
                assert np.array_equal(st, st2) and np.array_equal(nd, nd2) and np.array_equal(w, w2)
                assert tot == tot2
    assert not ctx.timed_out()


# ------------------------------------------------------ 6. slot reuse and epochs

@pytest.mark.parametrize("entries", [2, 64])
def test_one_lane_slot_serves_several_histories(ctx, entries):
    m = table("register")
    hists, ref = parity_case("register", "3x10")
    hists, ref = hists[:300], ref[:300]
    with knobs(ctx, table_budget=1, table_memo=entries, table_memo_grid=1):
        batch, st, nd, w, tot = run_host(ctx, m, hists)
        assert ctx.table_pass2() > 64 and ctx.table_memo_hits() > 0
    assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)


def test_tables_and_batches_between_calls(ctx):
    reg = table("register")
    odd = TableModel.from_closures(tg.reg_transition,
                                   lambda s, i, r: tg.reg_postcondition((s + 1) % 4 if i == "Read" else s, i, r),
                                   0, tg.REG_INVS, tg.REG_RESPS)
    hists = tg.gen_batch(tg.REGISTER, "3x10", 256, seed=21)
    other = tg.gen_batch(tg.REGISTER, "3x10", 256, seed=22)
    batch = codec.encode(reg, hists)
    refs = {k: [oracle_linearisable(mod.transition, mod.postcondition, 0, h, MAXN) for h in hists]
            for k, mod in (("reg", reg), ("odd", odd))}
    with knobs(ctx, table_budget=1, table_memo=64, table_memo_grid=2):
        # the same arrays, the same lane slots, another table: judged by its own
        for key, mod in (("reg", reg), ("odd", odd), ("reg", reg)):
            ctx.set_table(mod)
            st, nd, w, tot = ctx.check_arrays(3, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
            assert_results(mod, hists, refs[key], st, nd, w, batch.hdr, None, tot)
            assert ctx.table_memo_hits() > 0
        # two different batches of equal shape, back to back
        for hs in (hists, other, hists):
            b, st, nd, w, tot = run_host(ctx, reg, hs)
            assert_results(reg, hs, refs["reg"] if hs is hists else oracle("register", hs), st, nd, w, b.hdr,
                           None, tot)


# ------------------------------------------------------------ 7. classes and pids

def test_mixed_classes(ctx):
    names = ["reads_4x4", "reads_4x8", "reads_8x4", "reads_1x24_4x10", "reads_4x16", "lin_deep_4_3",
             "lin_deep_4_7", "lin_deep_4_9"]
    deep = [(tm.DEEP[n][1], tm.DEEP[n][3:5]) for n in names]
    short = [seq_history("register", n, s) for s in range(20) for n in (8, 32, 40, 64, 70, 128, 0)]
    items = deep + list(zip(short, [r[:2] for r in oracle("register", short, max_nodes=0)]))
    random.Random(7).shuffle(items)
    m = table("register")
    with knobs(ctx, DEEP_LIMIT_MS, table_memo=1024):
        batch, st, nd, w, tot = run_host(ctx, m, [h for h, _ in items], max_nodes=0)
        assert not ctx.timed_out() and ctx.table_memo_hits() > 0
    for i, (h, want) in enumerate(items):
        assert (codec.STATUS_NAMES[int(st[i])], int(nd[i])) == tuple(want), i
        if want[0] == "lin":
            assert replay_witness(m, h, witness_of(batch.hdr, w, i), None), i
    assert tot["budget"] == 1


def test_pids_100_to_127(ctx):
    check_deep(ctx, ["reads_8x4", "lin_deep_4_7", "lock_deep_4_7"], 1024, relabel=100)
