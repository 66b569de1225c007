"""GPU tests of the pending search's exact-count state memo (csrc/tpending.hip,
knob "pending_memo"): the deep crashed histories against their
known answers (tests/pendingmemo.py), and every output of the memo call against
the plain pending call, bit for bit, through the host and the device entry."""

import numpy as np
import pytest

import pending_ref as pr
import pendingmemo as pm
import tablegen as tg
from qsmd import codec, device
from qsmd.linearisability import linearisable, linearisable_batch
from test_gpu_table import CLOSURES, EXH, MAXN, table
from test_gpu_table import run_host as run_check_host
from test_gpu_table_pending import crash_case, levels, run_device, run_host, same

pytestmark = pytest.mark.gpu

L, R = tg.L, tg.R
KNOBS = ("pending_memo", "table_memo", "table_memo_grid", "table_budget")


class knobs:
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


def both(ctx, m, hists, max_nodes):
    """The host entry's outputs, checked equal to the device entry's; and the hits."""
    batch, *host = run_host(ctx, m, hists, max_nodes)
    hits = ctx.pending_memo_hits()
    dev = run_device(ctx, batch.hdr, batch.events, max_nodes)
    # (run_device reads the totals as signed 64-bit words: a node total of 2^64 - 1 comes back as -1)
    dev = dev[:4] + ({k: v & pm.U64 for k, v in dev[4].items()},)
    assert same(tuple(host), dev)
    assert ctx.pending_memo_hits() == hits
    return batch, tuple(host), hits


# ------------------------------------------------------------------ 1. deep rows

@pytest.mark.parametrize("name", sorted(pm.DEEP))
def test_deep_rows(ctx, name):
    model, hist, _, status, nodes, _ = pm.DEEP[name]
    m = table(model["name"])
    info = {}
    _, _, path = pm.pending_memo_dfs(model, hist, 1024, 0, info)
    # (pass 1's budget below the smallest row's 27 nodes: every row reaches pass 2)
    with knobs(ctx, 20000, pending_memo=1024, table_budget=4):
        batch, (st, nd, w, asm, tot), hits = both(ctx, m, [hist], 0)
        assert not ctx.timed_out()
    assert (codec.STATUS_NAMES[int(st[0])], int(nd[0])) == (status, nodes)
    assert hits == info["hits"] > 0
    if status == "lin":
        wit, a = levels(batch.hdr, 0, w, asm)
        assert pr.witness_ops(m.resps, hist, wit, a) == path and any(x is not None for x in a)
    assert tot["nodes"] == nodes


# ------------------------------------------- 2. bit-identity against the plain call

@pytest.mark.parametrize("setting", ["3x10", "4x16", "6x24"])
@pytest.mark.parametrize("name", ["register", "lock", "counter"])
def test_equals_the_plain_call(ctx, name, setting):
    m = table(name)
    hists, _ = crash_case(name, setting)
    hit = 0
    for budget in (256, 4, 0):
        with knobs(ctx, table_budget=budget):
            batch, *plain = run_host(ctx, m, hists)
            assert ctx.pending_memo_hits() == 0
            pass2 = ctx.table_pass2()
        for entries in (2, 64, 1024):
            with knobs(ctx, table_budget=budget, pending_memo=entries):
                _, got, hits = both(ctx, m, hists, MAXN)
                assert same(got, tuple(plain)), (budget, entries)
                assert ctx.table_pass2() == pass2
                assert hits == 0 if budget == 0 else True
                hit += hits
    assert not ctx.timed_out()
    if setting == "6x24":
        assert hit > 0


# ------------------------------------------- 3. the budget inside a recorded subtree

def test_budget_inside_a_recorded_subtree(ctx):
    model, hist, _, _, exact, _ = pm.DEEP["crashed_reads_4x4_1"]
    m = table("register")
    info = {}
    pm.pending_memo_dfs(model, hist, 1024, 0, info)
    before, count = max(info["trace"], key=lambda t: t[1])
    inside = before + count // 2
    assert before < inside < before + count
    for max_nodes in (exact - 1, exact, exact + 1, inside):
        want = pm.exact_count_pending(model, hist, max_nodes)
        mirror = {}
        assert pm.pending_memo_dfs(model, hist, 1024, max_nodes, mirror)[:2] == want
        with knobs(ctx, 20000):
            _, plain, _ = both(ctx, m, [hist], max_nodes)
        with knobs(ctx, 20000, pending_memo=1024):
            _, got, hits = both(ctx, m, [hist], max_nodes)
        assert same(got, plain) and hits == mirror["hits"] > 0
        assert (codec.STATUS_NAMES[int(got[0][0])], int(got[1][0])) == want
        assert got[4]["budget"] == (want[0] == "budget")
    # a count beyond 2^64: the budget of u64
    model, hist = pm.DEEP["crashed_reads_4x15_2"][:2]
    with knobs(ctx, 20000, pending_memo=1024):
        _, got, hits = both(ctx, m, [hist], 0)
        assert not ctx.timed_out()
    assert (codec.STATUS_NAMES[int(got[0][0])], int(got[1][0])) == ("budget", pm.U64) and hits > 0


# ------------------------------------------------------------------ 4. levels

def test_levels(ctx):
    m = table("register")
    hists = [pm.writes_only(n) for n in (32, 33, 64, 65, 128)]
    # one crashed history per class filled to n_ev - 1 events
    hists += [pm.crashed_reads([2] * 7, 3), pm.crashed_lin_deep(3, 10)[:63], pm.crashed_reads([4] * 15, 2) + [(9, L("Read"))] * 5]
    assert [len(h) for h in hists[5:]] == [31, 63, 127]
    for budget in (256, 4):
        with knobs(ctx, 20000, table_budget=budget):
            batch, plain, _ = both(ctx, m, hists, 200000)
        with knobs(ctx, 20000, table_budget=budget, pending_memo=64):
            _, got, _ = both(ctx, m, hists, 200000)
        assert same(got, plain)
        for i, n in enumerate((32, 33, 64, 65, 128)):
            assert (codec.STATUS_NAMES[int(got[0][i])], int(got[1][i])) == ("lin", n)
            assert levels(batch.hdr, i, got[2], got[3])[0] == list(range(n))
    for i in (5, 6, 7):
        want = pm.exact_count_pending(tg.REGISTER, hists[i], 200000)
        assert (codec.STATUS_NAMES[int(got[0][i])], int(got[1][i])) == want


# ------------------------------------------------------------ 5. the LDS fallback

def test_lds_fallback_of_the_largest_table(ctx):
    """The mod-256 counter's 80 KB of tables: the 128-event class's memo kernel
    would need 112 KB of columns beside them, so that class runs the plain
    kernel; the two narrower classes still run the memo."""
    m = table("counter")
    adds = [(i, L(1)) for i in range(100)]
    wide = [adds + [(100, L(0)), (100, R(100 % 32))], adds + [(100, L(0)), (100, R(5))]]

    def wrong(k):      # k pending `add 1`, then a completed `add 0` no order explains
        return [(i, L(1)) for i in range(k)] + [(k, L(0)), (k, R(31))] * 2

    with knobs(ctx, table_budget=4):
        for hists, hit in ((wide, False), ([wrong(5)], True), ([wrong(5) + [(90, L(1))] * 30], True),
                           (wide + [wrong(5), wrong(5) + [(90, L(1))] * 30], True)):
            ctx.set_param("pending_memo", 0)
            _, plain, _ = both(ctx, m, hists, MAXN)
            ctx.set_param("pending_memo", 64)
            _, got, hits = both(ctx, m, hists, MAXN)
            assert same(got, plain)
            assert (hits > 0) == hit, (len(hists), hits)
    assert not ctx.timed_out()


# ------------------------------------------------------------------ 6. table reuse

def deep_batch(seed, n=200):
    """n distinct deep histories (pass 2 takes them all; exact counts below the limit or `budget`)."""
    out = []
    for k in range(n):
        a, b = (seed + k) % 4 + 1, (seed + k // 4) % 3 + 2
        out.append(pm.crashed_reads([a, b, 3, (k % 5) + 1], 1 + k % 2) if k % 3 else pm.crashed_lin_deep(b, 2 + k % 3))
    return out


def test_table_reuse(ctx):
    m = table("register")
    b1, b2 = deep_batch(0), deep_batch(7)
    limit = 50000
    with knobs(ctx, table_budget=4):
        plain1, plain2 = run_host(ctx, m, b1, limit)[1:], run_host(ctx, m, b2, limit)[1:]
    with knobs(ctx, table_budget=4, pending_memo=64, table_memo_grid=1):
        got1 = run_host(ctx, m, b1, limit)[1:]
        assert ctx.pending_memo_hits() > 0 and ctx.table_pass2() > 150
        got2 = run_host(ctx, m, b2, limit)[1:]
        assert same(got1, plain1) and same(got2, plain2)
        fresh = device.Context(0, time_limit_ms=60000)
        try:
            fresh.set_param("table_budget", 4)
            fresh.set_param("pending_memo", 64)
            fresh.set_param("table_memo_grid", 1)
            assert same(run_host(fresh, m, b2, limit)[1:], got2)
        finally:
            fresh.close()
    # a check call with table_memo between pending calls with pending_memo, one context
    complete = tg.gen_batch(tg.REGISTER, "6x24", 200)
    with knobs(ctx):
        check0 = run_check_host(ctx, m, complete)[1:]
    with knobs(ctx, table_memo=64, pending_memo=64, table_budget=4):
        for _ in range(2):
            got = run_check_host(ctx, m, complete)[1:]
            assert all(np.array_equal(x, y) for x, y in zip(got[:3], check0[:3])) and got[3] == check0[3]
            assert same(run_host(ctx, m, b1, limit)[1:], plain1)
    assert not ctx.timed_out()


# ------------------------------------------------------ 7. refusals and isolation

def test_refusals_and_isolation(ctx):
    m = table("register")
    ctx.set_table(m)
    for bad in (3, 1 << 21, 1):
        with pytest.raises(device.DeviceError, match="pending_memo: 0 .off. or a power of two"):
            ctx.set_param("pending_memo", bad)
    assert ctx.get_param("pending_memo") == 0
    hist = pm.DEEP["crashed_lin_deep_4_3"][1]
    complete = tg.gen_batch(tg.REGISTER, "6x24", 100)
    # table_memo does not reach the pending call
    with knobs(ctx, table_memo=64, table_budget=4):
        _, plain, hits = both(ctx, m, [hist], 0)
        assert hits == 0 and ctx.table_memo_hits() == 0
    # pending_memo does not reach the check call
    with knobs(ctx, table_budget=4):
        check0 = run_check_host(ctx, m, complete)[1:]
        assert ctx.table_memo_hits() == 0
    with knobs(ctx, table_budget=4, pending_memo=64):
        got = run_check_host(ctx, m, complete)[1:]
        assert ctx.table_memo_hits() == 0
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], check0[:3])) and got[3] == check0[3]
        _, got, hits = both(ctx, m, [hist], 0)
        assert same(got, plain) and hits > 0 and ctx.table_memo_hits() == 0
    # the Python interface
    tr, post = m.transition, m.postcondition
    with pytest.raises(ValueError):
        linearisable(tr, post, None, hist, ctx=ctx, pending_memo=64)
    with pytest.raises(ValueError):
        linearisable_batch(m, [hist], ctx=ctx, pending_memo=64)
    assert linearisable(tr, post, None, hist, ctx=ctx, pending="complete", pending_memo=64)
    assert ctx.pending_memo_hits() > 0 and ctx.get_param("pending_memo") == 0
    res = linearisable_batch(m, [hist], ctx=ctx, pending="complete", pending_memo=1024, witness=True)
    assert res.verdict(0) == "lin" and int(res.nodes[0]) == 75026 and ctx.get_param("pending_memo") == 0
