"""GPU parity of qsmd_check_kpending_batch (csrc/kpending.hip): the keyed table
search that lets pending invocations take effect, against the literal
restatement on lists (tests/pending_ref.py) run on the product closures
(tests/ktablegen.py) -- status, node count, the witness's operations, the
assumed bytes, replay_witness and the totals, through the host and the device
entry.  No history is left out: the device runs with the reference's
max_nodes, and a `budget` verdict must match too (nodes == max_nodes)."""

import ctypes
import functools
import random

import numpy as np
import pytest

import anyshape as an
import pending_ref as pr
import pendingmemo as pm
import tablegen as tg
from qsmd import codec, device
from qsmd.linearisability import linearisable, linearisable_batch, replay_witness
from qsmd.models import KeyedTableModel
from test_gpu_ktable import component, keyed, prod
from test_gpu_ktable import run_host as run_check_host
from test_gpu_table import rc_of
from test_gpu_table_pending import budget_knob, levels, pick_closures, pick_table, same
from test_ktable_pending_host import KAT_OTHER_KEY, KAT_SEEN, KAT_TWO_KEYS, KAT_TWO_KEYS_SWAPPED, Rd, Val, W

pytestmark = pytest.mark.gpu

L, R = tg.L, tg.R
EXH = device.QSMD_FLAG_EXHAUSTIVE
MAXN = tg.MAX_NODES
NONE = device.QSMD_ASSUMED_NONE
CRASH = 0.3


@pytest.fixture(scope="module")
def ctx():
    """This module's own context (a keyed table, once set, cannot be taken
    away, and the session's context must stay without one: see
    test_gpu_ktable.py)."""
    c = device.Context(0, time_limit_ms=60000)
    yield c
    c.close()


def reference(closures, hists, max_nodes=MAXN, model0=None):
    return [pr.linearisable_pending(closures, h, max_nodes, model0) for h in hists]


def run_host(ctx, m, hists, model0=None, max_nodes=MAXN, flags=EXH):
    if ctx.keyed_table is not m:
        ctx.set_keyed_table(m)
    batch = codec.encode(m, hists, model0)
    assert not batch.encode_errors
    st, nd, w, asm, tot = ctx.check_kpending_arrays(batch.hdr, batch.events, m.pack_model0(model0, {}), flags,
                                                    max_nodes, witness=True)
    return batch, st, nd, w, asm, tot


def run_device(ctx, hdr, ev, model0=None, max_nodes=MAXN):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = len(hdr)
    d_hdr = torch.from_numpy(hdr.view(np.uint8).copy()).to(dev)
    d_ev = torch.from_numpy(ev.view(np.uint8).copy()).to(dev)
    d_st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    d_nd = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    d_w = torch.full((max(len(ev), 1),), 0xFF, dtype=torch.uint8, device=dev)
    d_a = torch.full((max(len(ev), 1),), 0xFF, dtype=torch.uint8, device=dev)
    d_tot = torch.zeros(8, dtype=torch.int64, device=dev)
    ctx.check_kpending_device(d_hdr.data_ptr(), n, d_ev.data_ptr(), len(ev), d_st.data_ptr(), d_nd.data_ptr(),
                              d_w.data_ptr(), d_tot.data_ptr(), model0=model0,
                              flags=EXH | device.QSMD_FLAG_WITNESS, max_nodes=max_nodes,
                              stream=torch.cuda.current_stream().cuda_stream, assumed_ptr=d_a.data_ptr())
    torch.cuda.synchronize()
    tot = dict(zip((n for n, _ in device.Totals._fields_), (int(x) for x in d_tot.cpu().numpy())))
    return (d_st.cpu().numpy()[:n], d_nd.cpu().numpy().astype(np.uint64)[:n], d_w.cpu().numpy()[:len(ev)],
            d_a.cpu().numpy()[:len(ev)], tot)


def assert_results(m, hists, ref, st, nd, wit, asm, hdr, tot, max_nodes=MAXN, model0=None):
    assert len(st) == len(hists) == len(ref)
    for i, (h, (st_o, nd_o, path_o)) in enumerate(zip(hists, ref)):
        got = codec.STATUS_NAMES[int(st[i])]
        assert (got, int(nd[i])) == (st_o, nd_o), (i, got, int(nd[i]), st_o, nd_o)
        if got == "budget":
            assert int(nd[i]) == max_nodes
        if got == "lin":
            w, a = levels(hdr, i, wit, asm)
            assert pr.witness_ops(m.resps, h, w, a) == path_o, i
            assert replay_witness(m, h, w, model0, assumed=a), i
    names = [codec.STATUS_NAMES[int(s)] for s in st]
    assert tot["linearisable"] == names.count("lin")
    assert tot["nonlinearisable"] == names.count("nonlin")
    assert tot["model_errors"] == names.count("error")
    assert tot["encode_errors"] == names.count("encode")
    assert tot["budget"] == names.count("budget")
    assert tot["checked"] == names.count("lin") + names.count("nonlin") + names.count("error")
    assert tot["skipped"] == 0 and tot["nodes"] == int(np.sum(nd.astype(np.uint64)))


def check_both(ctx, m, hists, ref, max_nodes=MAXN, model0=None):
    """Host and device entry against the reference."""
    batch, st, nd, w, asm, tot = run_host(ctx, m, hists, model0, max_nodes)
    assert_results(m, hists, ref, st, nd, w, asm, batch.hdr, tot, max_nodes, model0)
    assert same((st, nd, w, asm, tot),
                run_device(ctx, batch.hdr, batch.events, m.pack_model0(model0, {}), max_nodes))
    return batch, st, nd, w, asm


def pass2_expected(ref, budget):
    return sum(1 for r in ref if r[1] > budget or (r[0] == "budget" and r[1] >= budget)) if budget else 0


# ------------------------------------------------------------------ 1. KATs

def test_kats(ctx):
    ok = component("register").resps.index("Ok")
    for K, hists, want in ((4, [KAT_SEEN, KAT_OTHER_KEY], [("lin", 2), ("nonlin", 3)]),
                           (8, [KAT_TWO_KEYS, KAT_TWO_KEYS_SWAPPED], [("lin", 4), ("nonlin", 9)])):
        ref = reference(prod("register", K), hists)
        assert [(r[0], r[1]) for r in ref] == want
        for budget in (256, 0, 4):
            with budget_knob(ctx, budget):
                batch, st, nd, w, asm = check_both(ctx, keyed("register", K), hists, ref)
                assert ctx.table_pass2() == pass2_expected(ref, budget)
        if K == 4:
            assert levels(batch.hdr, 0, w, asm) == ([0, 1], [ok, None])
        else:
            assert levels(batch.hdr, 0, w, asm) == ([0, 1, 2, 4], [ok, ok, None, None])
    # the drop-in: None is today's call, "complete" the new one
    m = keyed("register", 4)
    tr, post = m.transition, m.postcondition
    assert not linearisable(tr, post, None, KAT_SEEN, ctx=ctx)
    assert linearisable(tr, post, None, KAT_SEEN, ctx=ctx, pending="complete")
    assert not linearisable(tr, post, None, KAT_OTHER_KEY, ctx=ctx, pending="complete")
    res = linearisable_batch(m, [KAT_SEEN, KAT_OTHER_KEY], ctx=ctx, witness=True, pending="complete")
    assert [res.verdict(i) for i in range(2)] == ["lin", "nonlin"] and list(res.nodes) == [2, 3]
    assert res.witness_of(0) == [0, 1] and res.assumed_of(0) == [ok, None]
    assert replay_witness(m, KAT_SEEN, res.witness_of(0), None, assumed=res.assumed_of(0))
    assert linearisable_batch(m, [KAT_SEEN], ctx=ctx, witness=True).assumed is None


# ----------------------------------------------- 2. randomised crash batches

# component, keys, setting, histories, the statuses the batch reaches
CRASH_BATCHES = [("register", 4, "3x10", 300, {"lin", "nonlin"}),
                 ("register", 4, "4x16", 300, {"lin", "nonlin", "budget"}),
                 ("lock", 8, "3x10", 300, {"lin", "nonlin", "error"}),
                 ("lock", 8, "4x16", 300, {"lin", "nonlin", "error"}),
                 ("register", 8, "6x24", 150, {"lin", "nonlin", "budget"}),
                 ("counter", 2, "4x16", 200, {"lin", "nonlin", "error"})]


@functools.lru_cache(maxsize=None)
def crash_case(name, K, setting, n):
    """n histories of a tablegen setting on the product with clients crashed,
    and the reference's results (computed once, shared)."""
    p = prod(name, K)
    rng = random.Random(f"kpending/{name}/{K}/{setting}")
    hists = [pr.crash(h, rng, CRASH) for h in tg.gen_batch(p, setting, n)]
    return hists, reference(p, hists)


@pytest.mark.parametrize("name,K,setting,n,statuses", CRASH_BATCHES)
def test_crash_batches(ctx, name, K, setting, n, statuses):
    m = keyed(name, K)
    hists, ref = crash_case(name, K, setting, n)
    assert sum(1 for h in hists if pr.pending_invocations(h)) > n // 3
    assert {r[0] for r in ref} == statuses
    assert any(a for r in ref for *_, a in r[2])
    assert sum(1 for h in hists if len({x[0] for _, (k, x) in h if k == "L"}) > 1) > n // 2
    default = ctx.get_param("table_budget")
    assert default == 256
    for budget in (default, 0, 4):
        with budget_knob(ctx, budget):
            batch, st, nd, w, asm, tot = run_host(ctx, m, hists)
            pass2 = ctx.table_pass2()
            assert_results(m, hists, ref, st, nd, w, asm, batch.hdr, tot)
            assert pass2 == pass2_expected(ref, budget)
            assert same((st, nd, w, asm, tot), run_device(ctx, batch.hdr, batch.events))
    assert not ctx.timed_out()
    # against the check call some verdicts go from nonlin to lin
    _, st0, _, _, _ = run_check_host(ctx, m, hists)
    names0 = [codec.STATUS_NAMES[int(s)] for s in st0]
    assert sum(1 for a, r in zip(names0, ref) if a == "nonlin" and r[0] == "lin") >= 9
    if name == "register" and K == 8:       # the second state register is in use
        assert any(x[0] >= 4 for h in hists for _, (kind, x) in h if kind == "L")
    if name == "counter":                   # the largest table: 80 KB beside the wider stack
        c = component("counter")
        assert c.post_err is not None and len(c.states) == 256


# ------------------------------------------- 3. one key is model 3's pending call

def test_one_key_equals_model_3(ctx):
    reg = component("register")
    rng = random.Random("kpending/one-key")
    hists = [pr.crash(h, rng, CRASH) for h in tg.gen_batch(tg.REGISTER, "4x16", 300)]
    assert sum(1 for h in hists if pr.pending_invocations(h)) > 100
    ctx.set_table(reg)
    b3 = codec.encode(reg, hists)
    m = keyed("register", 1)
    for budget in (256, 0, 4):
        with budget_knob(ctx, budget):
            r3 = ctx.check_pending_arrays(3, b3.hdr, b3.events, None, EXH, MAXN, witness=True)
            r5 = run_host(ctx, m, [[(p, (k, (0, x)) if k == "L" else (k, x)) for p, (k, x) in h] for h in hists])[1:]
            assert same(r5, r3)
    assert {0, 1} <= set(r3[0].tolist()) and np.any((r3[3] != NONE) & (r3[2] != 0xFF))


# ----------------------------------- 4. complete batches equal the keyed check call

@pytest.mark.parametrize("name,K", [("register", 4), ("lock", 8)])
def test_complete_batches_equal_the_check_call(ctx, name, K):
    m = keyed(name, K)
    hists = tg.gen_batch(prod(name, K), "4x16", 300)
    assert not any(pr.pending_invocations(h) for h in hists)
    for budget in (256, 0):
        with budget_knob(ctx, budget):
            batch, st0, nd0, w0, tot0 = run_check_host(ctx, m, hists)
            _, st, nd, w, asm, tot = run_host(ctx, m, hists)
            assert np.array_equal(st, st0) and np.array_equal(nd, nd0) and np.array_equal(w, w0) and tot == tot0
            assert len(asm) == len(batch.events) and np.all(asm == NONE)
            assert same((st, nd, w, asm, tot), run_device(ctx, batch.hdr, batch.events))
    assert {"lin", "nonlin"} <= {codec.STATUS_NAMES[int(s)] for s in st}


# ------------------------------------------- 5. several allowed responses

def test_several_allowed_responses(ctx):
    """The pick model (symbols 3, 7 and 31 with different next states, symbol
    5 masked by post_err) on 2 keys, the Picks and Gets spread over both."""
    import ktablegen as kg
    c, comp = pick_table()
    p = kg.product(dict(pick_closures(), real=None), 2)
    m = KeyedTableModel(comp, 2)
    pick = lambda k: L((k, "Pick"))                                         # noqa: E731
    get = lambda pid, k, v: [(pid, L((k, "Get"))), (pid, R(v))]             # noqa: E731
    reset = lambda pid, k: [(pid, L((k, "Reset"))), (pid, R(0))]            # noqa: E731
    hists = [[(0, pick(v % 2))] + get(1, v % 2, v) for v in (1, 2, 3, 0)]
    # two pending Picks, the second after a Reset: the resume at both levels; and one on each key
    hists.append([(0, pick(1)), *reset(1, 1), (2, pick(1))] + get(3, 1, 3))
    hists.append([(0, pick(0))] + get(1, 0, 2) + [*reset(1, 0), (2, pick(1))] + get(3, 1, 3) + get(3, 0, 0))
    ref = reference(p, hists)
    assert [(r[0], r[1]) for r in ref[:4]] == [("lin", 2), ("lin", 4), ("lin", 6), ("lin", 8)]
    assert [a for *_, a in ref[2][2]] == [True, False] and ref[2][2][0][2] == 31
    assert ref[4][0] == ref[5][0] == "lin"
    rng = random.Random("kpending/pick")
    for _ in range(300):
        h = []
        for _ in range(rng.randint(1, 12)):
            pid, k = rng.randrange(4), rng.randrange(2)
            kind = rng.random()
            if kind < 0.3:
                h.append((pid, pick(k)))
            elif kind < 0.45:
                h += reset(pid, k)
            else:
                h += get(pid, k, rng.choice([0, 1, 2, 3, 3]))
        hists.append(h)
    ref = reference(p, hists)
    picked = {(op[1][0], op[2]) for r in ref for op in r[2] if op[3]}
    assert picked >= {(k, s) for k in (0, 1) for s in (3, 7, 31)}      # the second and the third choice, on both keys
    assert {r[0] for r in ref} == {"lin", "nonlin"}
    for budget in (256, 0, 4):
        with budget_knob(ctx, budget):
            check_both(ctx, m, hists, ref)


# ------------------------------------------------ 6. depth beyond n_ev / 2

@pytest.mark.parametrize("k", [20, 40, 100])
def test_depth_of_one_level_per_invocation(ctx, k):
    """k pids with a pending Write each (pid i on key i % 8), then one
    completed Read of the last write's key and value: k + 1 levels on k + 2
    events; then the width class filled, and invocations only."""
    m, p = keyed("register", 8), prod("register", 8)
    vals = [1 + (i % 3) for i in range(k)]
    last = (k - 1) % 8
    h = [(i, W(i % 8, v)) for i, v in enumerate(vals)] + [(k, Rd(last)), (k, Val(vals[-1]))]
    assert len(h) == k + 2 and k + 1 > len(h) // 2
    ev = {20: 32, 40: 64, 100: 128}[k]
    more = [(i, W(last, vals[-1])) for i in range(k + 1, k + 1 + ev - len(h))]
    h2 = h[:-1] + more + h[-1:]
    h3 = [(i, W(i % 8, 1 + (i % 3))) for i in range(ev)]
    assert len(h2) == len(h3) == ev
    hists = [h, h2, h3]
    ref = reference(p, hists)
    assert (ref[0][0], ref[0][1], len(ref[0][2])) == ("lin", k + 1, k + 1)
    assert (ref[1][0], ref[1][1], len(ref[1][2])) == ("lin", ev - 1, ev - 1)
    assert (ref[2][0], ref[2][1], len(ref[2][2])) == ("lin", ev, ev)
    for budget in (256, 0, 4):
        with budget_knob(ctx, budget):
            batch, st, nd, w, asm = check_both(ctx, m, hists, ref)
            wit, a = levels(batch.hdr, 0, w, asm)
            assert wit == list(range(k + 1)) and a == [m.resps.index("Ok")] * k + [None]
            assert len(levels(batch.hdr, 1, w, asm)[0]) == ev - 1 and len(levels(batch.hdr, 2, w, asm)[0]) == ev


# ------------------------------- 7. the largest table in the widest class

def test_largest_table_in_the_widest_class(ctx):
    """counter^2 (80 KB of component tables with post_err) on 102 events: the
    128-event class's 48 KB of columns beside it in one workgroup.  100 pids
    with a pending `add 1` each on key i % 2, then a completed `add 0` on key 1
    that answers 50 mod 32 (101 nodes) or a wrong value (every order of the
    pending ones fails: `budget`, through pass 2 as well)."""
    m, p = keyed("counter", 2), prod("counter", 2)
    c = component("counter")
    assert c.post_err is not None and c.post.nbytes + c.post_err.nbytes + c.on_inv.nbytes + c.on_resp.nbytes == 80 << 10
    adds = [(i, L((i % 2, 1))) for i in range(100)]
    hists = [adds + [(100, L((1, 0))), (100, R(50 % 32))], adds + [(100, L((1, 0))), (100, R(5))]]
    ref = reference(p, hists)
    assert [(r[0], r[1]) for r in ref] == [("lin", 101), ("budget", MAXN)]
    for budget in (256, 0):
        with budget_knob(ctx, budget):
            check_both(ctx, m, hists, ref)
            assert ctx.table_pass2() == pass2_expected(ref, budget)
    assert not ctx.timed_out()


# ------------- 8. undo across an assumed level after a completed one on another key

def test_undo_of_an_assumed_level_after_a_completed_operation_on_another_key(ctx):
    """p0 writes key 0 (completed), then writes key 5 and crashes; p1 reads
    key 5 as 0.  The search assumes the second write first, fails at the read
    and must come back across the assumed level: byte 5 restored, byte 0 and
    p0's Ok left alone."""
    m, p = keyed("register", 8), prod("register", 8)
    w1 = [(0, W(0, 1)), (0, R("Ok")), (0, W(5, 2))]
    hists = [w1 + [(1, Rd(5)), (1, Val(0))],
             w1 + [(1, Rd(5)), (1, Val(0)), (1, Rd(0)), (1, Val(1))],
             w1 + [(1, Rd(5)), (1, Val(3))],
             w1 + [(1, Rd(5)), (2, Rd(0)), (1, Val(0)), (2, Val(1)), (3, Rd(5)), (3, Val(2))]]
    ref = reference(p, hists)
    assert [(r[0], r[1]) for r in ref] == [("lin", 5), ("lin", 6), ("nonlin", 4), ("lin", 9)]
    assert ref[0][2] == [(0, (0, ("Write", 1)), "Ok", False), (1, (5, "Read"), ("Val", 0), False),
                         (0, (5, ("Write", 2)), "Ok", True)]
    for budget in (256, 0, 2):
        with budget_knob(ctx, budget):
            batch, st, nd, w, asm = check_both(ctx, m, hists, ref)
            assert ctx.table_pass2() == pass2_expected(ref, budget)
            assert levels(batch.hdr, 0, w, asm) == ([0, 3, 2], [None, None, m.resps.index("Ok")])


# ------------------------------------- 9. a model0 with a different state per key

def test_model0_per_key(ctx):
    m, p = keyed("register", 4), prod("register", 4)
    model0 = (3, 0, 2, 1)
    rng = random.Random("kpending/model0")
    hists = [pr.crash(h, rng, CRASH) for h in tg.gen_batch(p, "3x10", 200)]
    hists += [[(0, W(1, 3)), (1, Rd(2)), (1, Val(2))], [(0, W(1, 3)), (1, Rd(2)), (1, Val(0))]]
    ref = reference(p, hists, model0=model0)
    assert [(r[0], r[1]) for r in ref[-2:]] == [("lin", 2), ("nonlin", 3)]
    assert [r[0] for r in ref] != [r[0] for r in reference(p, hists)]
    assert {r[0] for r in ref} == {"lin", "nonlin"}
    for budget in (256, 0, 4):
        with budget_knob(ctx, budget):
            check_both(ctx, m, hists, ref, model0=model0)
    batch = codec.encode(m, hists[-2:], None)
    bad = (ctypes.c_uint32 * 4)(0, 1, len(component("register").states), 0)
    with pytest.raises(device.DeviceError) as e:
        ctx.check_kpending_arrays(batch.hdr, batch.events, bad)
    assert rc_of(e) == -1
    st, nd, _, _, _ = ctx.check_kpending_arrays(batch.hdr, batch.events, None, EXH, MAXN)
    assert [codec.STATUS_NAMES[int(s)] for s in st] == ["nonlin", "lin"]


# ------------------------------------------------------ 10. any-shape histories

ANY_SETTINGS = {"6x14": 200, "6x16": 200, "8x24": 100, "2x62": 60, an.RANDOM: 500}
assert set(ANY_SETTINGS) == set(an.ALL_SETTINGS)


@functools.lru_cache(maxsize=None)
def anyshape_case(setting):
    p = prod("register", 4)
    hists = an.batch(p, setting, ANY_SETTINGS[setting])
    return hists, reference(p, hists)


@pytest.mark.parametrize("setting", list(ANY_SETTINGS))
def test_anyshape(ctx, setting):
    """Shared pids, stray and leading responses: whether a pid has a remaining
    response is decided at the node, and the key of an undo is the chosen
    event's."""
    m = keyed("register", 4)
    hists, ref = anyshape_case(setting)
    feats = set().union(*(an.census(h) for h in hists))
    assert feats == set(an.FEATURES)
    for budget in (256, 0, 4):
        with budget_knob(ctx, budget):
            check_both(ctx, m, hists, ref)
    assert not ctx.timed_out()


# ------------------------------------------------------------ 11. inert knobs

def test_knobs_are_inert(ctx):
    m = keyed("register", 4)
    hists, ref = crash_case("register", 4, "4x16", 300)
    # a model-3 memo call and a local check call first: their counters stand
    reg = component("register")
    deep = pm.DEEP["crashed_lin_deep_4_3"][1]
    assert linearisable(reg.transition, reg.postcondition, None, deep, ctx=ctx, pending="complete", pending_memo=64)
    ctx.set_param("ktable_local", 1)
    complete = codec.encode(m, tg.gen_batch(prod("register", 4), "4x16", 100), None)
    ctx.set_keyed_table(m)
    ctx.check_arrays(5, complete.hdr, complete.events, None, EXH, MAXN)
    ctx.set_param("ktable_local", 0)
    local_last, memo_hits = ctx.ktable_local_last(), ctx.pending_memo_hits()
    assert local_last > 0 and memo_hits > 0
    plain = run_host(ctx, m, hists)
    assert_results(m, hists, ref, *plain[1:5], plain[0].hdr, plain[5])
    knobs = {"ktable_memo": 64, "ktable_local": 1, "pending_memo": 64, "table_memo": 64}
    try:
        for k, v in knobs.items():
            ctx.set_param(k, v)
        got = run_host(ctx, m, hists)
        assert same(got[1:], plain[1:])
        assert same(run_device(ctx, got[0].hdr, got[0].events), plain[1:])
        # without a witness the local mode would take a check call: still the product search
        st, nd, _, _, tot = ctx.check_kpending_arrays(got[0].hdr, got[0].events, None, EXH, MAXN)
        assert np.array_equal(st, plain[1]) and np.array_equal(nd, plain[2]) and tot == plain[5]
        assert ctx.ktable_local_last() == local_last and ctx.pending_memo_hits() == memo_hits
    finally:
        for k in knobs:
            ctx.set_param(k, 0)


# ------------------------------------------------------------------ 12. refusals

def test_refusals(ctx):
    m = keyed("register", 4)
    ctx.set_keyed_table(m)
    batch = codec.encode(m, [KAT_SEEN, KAT_OTHER_KEY, KAT_SEEN], None)
    fresh = device.Context(0, time_limit_ms=60000)
    try:
        with pytest.raises(device.DeviceError, match=r"\(-1\)"):
            fresh.check_kpending_arrays(batch.hdr, batch.events)
    finally:
        fresh.close()
    with pytest.raises(device.DeviceError, match=r"\(-4\)"):
        ctx.check_kpending_arrays(batch.hdr, batch.events, flags=EXH | device.QSMD_FLAG_EARLY_EXIT_BATCH)
    # a key >= n_keys: that history's ENCODE_ERROR, the rest of the batch decided
    ev = batch.events.copy()
    o = int(batch.hdr[1]["ev_off"])
    assert int(ev[o]["a"]) == 2
    ev[o]["a"] = 4
    st, nd, w, asm, tot = ctx.check_kpending_arrays(batch.hdr, ev, None, EXH, MAXN, witness=True)
    assert [codec.STATUS_NAMES[int(s)] for s in st] == ["lin", "encode", "lin"] and list(nd) == [2, 0, 2]
    assert tot["encode_errors"] == 1 and tot["linearisable"] == 2
    from qsmd.models import WideTableModel
    c = tg.REGISTER
    wide = WideTableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"])
    with pytest.raises(NotImplementedError):
        linearisable_batch(wide, [[]], ctx=ctx, pending="complete")
    with pytest.raises(NotImplementedError):
        linearisable_batch("bank", [[]], ctx=ctx, pending="complete")
    with pytest.raises(ValueError):
        linearisable_batch(m, [KAT_SEEN], ctx=ctx, pending="complete", pending_memo=64)
    # the context still serves the call
    st, nd, _, _, _ = ctx.check_kpending_arrays(batch.hdr, batch.events)
    assert [(codec.STATUS_NAMES[int(s)], int(n)) for s, n in zip(st, nd)] == [("lin", 2), ("nonlin", 3), ("lin", 2)]
