"""GPU tests of the keyed path's exact-count state memo (csrc/ktable.hip, knob
"ktable_memo"): pass 2 records every failed subtree under its
full key (remaining events, the 64-bit state) and counts it on the next visit,
so status, node count and witness stay the reference's while a tree of 1e18
nodes is decided in a few thousand iterations.

The references are tests/ktablememo.py (the exact count on the product
closures, and the literal mirror of the kernel's step) and, for generated
batches, the literal oracle on the product closures as in test_gpu_ktable.py."""

import random

import numpy as np
import pytest

import ktablegen as kg
import ktablememo as km
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device
from qsmd.linearisability import ModelError, linearisable, linearisable_batch, replay_witness
from qsmd.models import KeyedTableModel, TableModel
from test_gpu_ktable import keyed, oracle, parity_case, prod, run_host
from test_gpu_table import EXH, MAXN, assert_results, run_device, witness_path
from test_gpu_table import parity_case as parity_case3
from test_gpu_table import run_host as run_host3
from test_gpu_table import table as table3

pytestmark = pytest.mark.gpu

DEEP_LIMIT_MS = 5000        # a cap, not a measurement: a broken memo ends as BUDGET instead of hanging
KNOBS = ("ktable_memo", "table_memo", "table_memo_grid", "table_budget")


@pytest.fixture(scope="module")
def ctx():
    """This module's own context (a keyed table, once set, cannot be taken
    away: see test_gpu_ktable.py)."""
    c = device.Context(0, time_limit_ms=60000)
    yield c
    c.close()


class knobs:
    """Set table knobs / the time limit; restore all of them on exit."""

    def __init__(self, ctx, time_limit_ms=None, **params):
        self.ctx, self.params, self.ms = ctx, params, time_limit_ms

    def __enter__(self):
        self.saved = {k: self.ctx.get_param(k) for k in KNOBS}
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


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def check_kdeep(ctx, names, entries, max_nodes=0, want=None, relabel=0, budget=None):
    """The KDEEP rows `names`, one batch per component (on its 8-key product:
    a row on fewer keys leaves the others alone), through both entries."""
    for comp in ("register", "lock"):
        rows = [n for n in names if km.KDEEP[n][0] == comp]
        if not rows:
            continue
        m = keyed(comp, 8)
        hists = [[(relabel + p, e) for p, e in km.KDEEP[n][2]] for n in rows]
        extra = {} if budget is None else {"table_budget": budget}
        with knobs(ctx, DEEP_LIMIT_MS, ktable_memo=entries, **extra):
            batch, st, nd, w, tot = run_host(ctx, m, hists, max_nodes=max_nodes, flags=EXH)
            hits = ctx.table_memo_hits()
            timed = ctx.timed_out()
            st2, nd2, w2, tot2 = run_device(ctx, batch.hdr, batch.events, max_nodes=max_nodes, model_id=5)
            hits2 = ctx.table_memo_hits()
        assert not timed
        assert same((st, nd, w, tot), (st2, nd2, w2, tot2))
        for i, n in enumerate(rows):
            exp = want[n] if want else km.KDEEP[n][4:6]
            got = (codec.STATUS_NAMES[int(st[i])], int(nd[i]))
            print(n, entries, got, exp)
            assert got == tuple(exp), (n, got, exp)
            if got[0] == "lin":
                wit = witness_of(batch.hdr, w, i)
                assert replay_witness(m, hists[i], wit, None), n
                assert witness_path(hists[i], wit) == [(p + relabel, a, b) for p, a, b in
                                                       km.mirror(n, entries, max_nodes)[2]]
        assert tot["nodes"] == int(np.sum(nd, dtype=np.uint64))
        assert hits > 0 and hits2 > 0, (hits, hits2)


# ------------------------------------------------------------------- 1. the knob

def test_knob(ctx):
    assert ctx.get_param("ktable_memo") == 0 and ctx.get_param("table_memo") == 0
    for bad in (3, 1, 1 << 21):
        with pytest.raises(device.DeviceError) as e:
            ctx.set_param("ktable_memo", bad)
        assert "failed (-1)" in str(e.value)
        assert ctx.get_param("ktable_memo") == 0
    with knobs(ctx):
        ctx.set_param("ktable_memo", 1 << 20)       # (accepted; no call made with it)
        assert ctx.get_param("ktable_memo") == 1 << 20
        with pytest.raises(device.DeviceError):
            ctx.set_param("ktable_memo", 6)
        assert ctx.get_param("ktable_memo") == 1 << 20
    assert ctx.get_param("ktable_memo") == 0


def test_knob_does_not_reach_model_3(ctx):
    m3 = table3("register")
    hists, ref = parity_case3("register", "3x10")
    with knobs(ctx, table_budget=1):
        before = run_host3(ctx, m3, hists)
        assert ctx.table_pass2() > 0
        ctx.set_param("ktable_memo", 64)
        after = run_host3(ctx, m3, hists)
        assert ctx.table_memo_hits() == 0 and ctx.table_pass2() > 0
    assert same(before[1:], after[1:])
    assert_results(m3, hists, ref, after[1], after[2], after[3], after[0].hdr, None, after[4])


def test_knob_off_is_the_plain_search(ctx):
    m = keyed("register", 4)
    hists, ref = parity_case("register", 4, "3x10")
    with knobs(ctx, table_budget=1):
        assert ctx.get_param("ktable_memo") == 0
        batch, *off = run_host(ctx, m, hists)
        assert ctx.table_memo_hits() == 0 and ctx.table_pass2() > 0
        ctx.set_param("table_memo", 64)             # the other paths' knob: no effect on model 5
        _, *off2 = run_host(ctx, m, hists)
        assert ctx.table_memo_hits() == 0 and ctx.table_pass2() > 0
        ctx.set_param("ktable_memo", 64)
        ctx.set_param("table_budget", 0)            # a single pass: no pass 2, no memo
        _, *one = run_host(ctx, m, hists)
        assert ctx.table_memo_hits() == 0 and ctx.table_pass2() == 0
    assert same(off, off2) and same(off, one)
    assert_results(m, hists, ref, off[0], off[1], off[2], batch.hdr, None, off[3])


# ---------------------------------------------------------------- 2. deep rows

def test_deep_rows(ctx):
    check_kdeep(ctx, sorted(km.KDEEP), 4096)


# ----------------------------------------------------------- 3. the drop-in call

@pytest.mark.parametrize("name", sorted(km.KDEEP))
def test_deep_linearisable_call(ctx, name):
    comp, _, hist, _, status, nodes, _ = km.KDEEP[name]
    m = keyed(comp, 8)
    with knobs(ctx, DEEP_LIMIT_MS):
        if status == "error":
            with pytest.raises(ModelError):
                linearisable(m.transition, m.postcondition, None, hist, ctx=ctx, table_memo=4096)
        else:
            assert linearisable(m.transition, m.postcondition, None, hist, ctx=ctx,
                                table_memo=4096) == (status == "lin")
        assert ctx.get_param("ktable_memo") == 0 and ctx.get_param("table_memo") == 0 and not ctx.timed_out()
        # (a search within pass 1's budget never reaches the memo pass)
        assert (ctx.table_memo_hits() > 0) == (nodes > ctx.get_param("table_budget"))
        res = linearisable_batch(m, [hist], ctx=ctx, table_memo=4096)
        assert (res.verdict(0), int(res.nodes[0])) == (status, nodes)
        assert ctx.get_param("ktable_memo") == 0


# --------------------------------------------------------------- 4. lossy tables

@pytest.mark.parametrize("entries", sorted(km.LOSSY))
def test_lossy_tables(ctx, entries):
    check_kdeep(ctx, km.LOSSY[entries], entries, budget=1)


# -------------------------------------------------------- 5. budget inside a hit

@pytest.mark.parametrize("name,max_nodes,want", km.BUDGET_CASES)
def test_budget_inside_a_hit(ctx, name, max_nodes, want):
    assert want == (("budget", max_nodes) if max_nodes < km.KDEEP[name][5] else km.KDEEP[name][4:6])
    check_kdeep(ctx, [name], 4096, max_nodes=max_nodes, want={name: want})


# ---------------------------------------------------------- 6. whole-path parity

@pytest.mark.parametrize("name,K,setting", [("register", 4, "3x10"), ("register", 4, "4x16"), ("lock", 8, "4x16"),
                                            ("register", 8, "4x16")])
def test_whole_path_parity(ctx, name, K, setting):
    m = keyed(name, K)
    hists, ref = parity_case(name, K, setting)
    default = ctx.get_param("table_budget")
    for budget, sizes in ((1, (2, 64, 4096)), (default, (64,))):
        with knobs(ctx, table_budget=budget):
            run_host(ctx, m, hists)
            pass2_off = ctx.table_pass2()
            assert ctx.table_memo_hits() == 0
            for entries in sizes:
                ctx.set_param("ktable_memo", entries)
                batch, st, nd, w, tot = run_host(ctx, m, hists)
                assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)
                assert ctx.table_memo_hits() > 0 and ctx.table_pass2() == pass2_off
                assert same((st, nd, w, tot), run_device(ctx, batch.hdr, batch.events, model_id=5))
    assert not ctx.timed_out()


# --------------------------------------------- 7. slot reuse and stale entries

@pytest.mark.parametrize("entries", [2, 64])
def test_one_lane_slot_serves_several_histories(ctx, entries):
    m = keyed("register", 4)
    hists, ref = parity_case("register", 4, "3x10")
    hists, ref = hists[:300], ref[:300]
    with knobs(ctx, table_budget=1, ktable_memo=entries, table_memo_grid=1):
        batch, st, nd, w, tot = run_host(ctx, m, hists)
        assert ctx.table_pass2() > 64 and ctx.table_memo_hits() > 0
    assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)


def odd_closures():
    """The register whose Read sees the value one higher."""
    return dict(tg.REGISTER, name="odd",
                postcondition=lambda s, i, r: tg.reg_postcondition((s + 1) % 4 if i == "Read" else s, i, r))


def test_tables_keys_and_model0_between_calls(ctx):
    """The same arrays in the same lane slots under another component table,
    another n_keys and another model0, back to back: each judged by its own."""
    odd = odd_closures()
    odd4 = KeyedTableModel(TableModel.from_closures(odd["transition"], odd["postcondition"], 0, tg.REG_INVS,
                                                    tg.REG_RESPS, raises=OracleModelError), 4)
    reg4, reg8 = keyed("register", 4), keyed("register", 8)
    hists = tg.gen_batch(prod("register", 4), "3x10", 256, seed=21)
    batch = codec.encode(reg4, hists)
    assert not batch.encode_errors
    start = (3, 0, 2, 1)

    def ref_of(p, init):
        return [oracle_linearisable(p["transition"], p["postcondition"], init, h, MAXN) for h in hists]

    refs = {"reg4": ref_of(prod("register", 4), (0,) * 4), "odd4": ref_of(kg.product(odd, 4), (0,) * 4),
            "reg8": ref_of(prod("register", 8), (0,) * 8), "start": ref_of(prod("register", 4), start)}
    assert [r[:2] for r in refs["reg4"]] != [r[:2] for r in refs["odd4"]]
    assert [r[:2] for r in refs["reg4"]] != [r[:2] for r in refs["start"]]
    with knobs(ctx, table_budget=1, ktable_memo=64, table_memo_grid=2):
        for key, m, model0 in (("reg4", reg4, None), ("odd4", odd4, None), ("reg8", reg8, None),
                               ("start", reg4, start), ("reg4", reg4, None)):
            ctx.set_keyed_table(m)
            st, nd, w, tot = ctx.check_arrays(5, batch.hdr, batch.events, m.pack_model0(model0, {}), EXH, MAXN,
                                              witness=True)
            assert_results(m, hists, refs[key], st, nd, w, batch.hdr, model0, tot)
            assert ctx.table_memo_hits() > 0


def test_model_3_and_model_5_alternate(ctx):
    m3, m5 = table3("register"), keyed("register", 4)
    h3, ref3 = parity_case3("register", "3x10")
    h5, ref5 = parity_case("register", 4, "3x10")
    h3, ref3, h5, ref5 = h3[:256], ref3[:256], h5[:256], ref5[:256]
    with knobs(ctx, table_budget=1, ktable_memo=64, table_memo=64, table_memo_grid=2):
        for _ in range(2):
            batch, st, nd, w, tot = run_host3(ctx, m3, h3)
            assert_results(m3, h3, ref3, st, nd, w, batch.hdr, None, tot)
            assert ctx.table_memo_hits() > 0
            batch, st, nd, w, tot = run_host(ctx, m5, h5)
            assert_results(m5, h5, ref5, st, nd, w, batch.hdr, None, tot)
            assert ctx.table_memo_hits() > 0


# ------------------------------------------------------------ 8. model0 and pids

def test_model0(ctx):
    start = (0, 1, 0, 2, 3, 1, 2, 3)            # keys 4-7 (the state's high word) non-initial
    m = keyed("register", 8)
    hists = tg.gen_batch(dict(prod("register", 8), init=start), "4x16", 400, seed=9)
    ref = oracle("register", 8, hists, model0=start)
    assert [r[:2] for r in ref] != [r[:2] for r in oracle("register", 8, hists)]
    with knobs(ctx, table_budget=1, ktable_memo=64):
        batch, st, nd, w, tot = run_host(ctx, m, hists, start)
        assert ctx.table_memo_hits() > 0
        assert_results(m, hists, ref, st, nd, w, batch.hdr, start, tot)
        assert same((st, nd, w, tot), run_device(ctx, batch.hdr, batch.events, m.pack_model0(start, {}), model_id=5))
    assert {0, 1} <= set(st.tolist())


def test_pids_100_to_127(ctx):
    check_kdeep(ctx, ["klin_deep_2_3_2", "kreads_8_4x4_k7373", "kreads_8_4x12", "klock_deep_8_4_10"], 4096,
                relabel=100)


# -------------------------------------------------------------- 9. mixed classes

def test_mixed_classes(ctx):
    names = [n for n in sorted(km.KDEEP) if km.KDEEP[n][0] == "register"]
    assert {0, 1, 2} == {(km.KDEEP[n][3] > 32) + (km.KDEEP[n][3] > 64) for n in names}
    deep = [(km.KDEEP[n][2], km.KDEEP[n][4:6]) for n in names]
    p = prod("register", 8)
    short = [tg.gen_history(p, random.Random(f"kmemo/short/{n}/{s}"), 2, n // 2, 0.03)
             for s in range(20) for n in (8, 32, 40, 64, 70, 128, 0)]
    # (some of the 128-event ones have 1e7 nodes: the exact count, not the oracle's walk)
    items = deep + [(h, km.tm.exact_count(p, h, 0)) for h in short]
    random.Random(7).shuffle(items)
    m = keyed("register", 8)
    with knobs(ctx, DEEP_LIMIT_MS, ktable_memo=4096):
        batch, st, nd, w, tot = run_host(ctx, m, [h for h, _ in items], max_nodes=0)
        assert not ctx.timed_out() and ctx.table_memo_hits() > 0
    for i, (h, want) in enumerate(items):
        assert (codec.STATUS_NAMES[int(st[i])], int(nd[i])) == tuple(want), i
        if want[0] == "lin":
            assert replay_witness(m, h, witness_of(batch.hdr, w, i), None), i
    assert tot["budget"] == 0 and tot["nodes"] == int(np.sum(nd, dtype=np.uint64))
