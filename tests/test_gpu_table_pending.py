"""GPU parity of qsmd_check_pending_batch (csrc/tpending.hip): the table search
that lets pending invocations take effect, against its literal restatement on
lists (tests/pending_ref.py) -- status, node count, the witness's operations,
the assumed bytes and the totals, through the host and the device entry.  No
history is left out: the device runs with the reference's max_nodes, and a
`budget` verdict must match too (nodes == max_nodes)."""

import functools
import random

import numpy as np
import pytest

import anyshape as an
import pending_ref as pr
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from qsmd import codec, device
from qsmd.linearisability import linearisable, linearisable_batch, replay_witness
from qsmd.models import TableModel
from test_gpu_table import CLOSURES, EXH, MAXN, table
from test_gpu_table import run_host as run_check_host
from test_pending_host import (KAT_LONE_UNLOCK, KAT_UNLOCK_AND_FAILURE, KAT_WRITE_SEEN, KAT_WRITE_UNSEEN)

pytestmark = pytest.mark.gpu

L, R = tg.L, tg.R
NONE = device.QSMD_ASSUMED_NONE
CRASH = 0.3
N_CRASH = 500


def reference(c, hists, max_nodes=MAXN):
    return [pr.linearisable_pending(c, h, max_nodes) for h in hists]


def run_host(ctx, m, hists, max_nodes=MAXN, flags=EXH):
    if ctx.table is not m:
        ctx.set_table(m)
    batch = codec.encode(m, hists, None)
    assert not batch.encode_errors
    st, nd, w, asm, tot = ctx.check_pending_arrays(3, batch.hdr, batch.events, None, flags, max_nodes, witness=True)
    return batch, st, nd, w, asm, tot


def run_device(ctx, hdr, ev, max_nodes=MAXN):
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
    ctx.check_pending_device(3, d_hdr.data_ptr(), n, d_ev.data_ptr(), len(ev), d_st.data_ptr(), d_nd.data_ptr(),
                             d_w.data_ptr(), d_tot.data_ptr(), flags=EXH | device.QSMD_FLAG_WITNESS,
                             max_nodes=max_nodes, stream=torch.cuda.current_stream().cuda_stream,
                             assumed_ptr=d_a.data_ptr())
    torch.cuda.synchronize()
    tot = dict(zip((n for n, _ in device.Totals._fields_), (int(x) for x in d_tot.cpu().numpy())))
    return (d_st.cpu().numpy()[:n], d_nd.cpu().numpy().astype(np.uint64)[:n], d_w.cpu().numpy()[:len(ev)],
            d_a.cpu().numpy()[:len(ev)], tot)


def levels(hdr, i, wit, asm):
    """History i's witness and, per level, the assumed symbol or None."""
    o, n = int(hdr[i]["ev_off"]), int(hdr[i]["n_ev"])
    w = []
    for x in wit[o:o + n]:
        if x == codec.WITNESS_END:
            break
        w.append(int(x))
    return w, [None if x == NONE else int(x) for x in asm[o:o + len(w)]]


def assert_results(m, hists, ref, st, nd, wit, asm, hdr, tot, max_nodes=MAXN):
    assert len(st) == len(hists) == len(ref)
    for i, (h, (st_o, nd_o, path_o)) in enumerate(zip(hists, ref)):
        got = codec.STATUS_NAMES[int(st[i])]
        assert (got, int(nd[i])) == (st_o, nd_o), (i, got, int(nd[i]), st_o, nd_o)
        if got == "budget":
            assert int(nd[i]) == max_nodes
        if got == "lin":
            w, a = levels(hdr, i, wit, asm)
            assert pr.witness_ops(m.resps, h, w, a) == path_o, i
            assert replay_witness(m, h, w, None, assumed=a), i
    names = [codec.STATUS_NAMES[int(s)] for s in st]
    assert tot["linearisable"] == names.count("lin")
    assert tot["nonlinearisable"] == names.count("nonlin")
    assert tot["model_errors"] == names.count("error")
    assert tot["encode_errors"] == names.count("encode")
    assert tot["budget"] == names.count("budget")
    assert tot["checked"] == names.count("lin") + names.count("nonlin") + names.count("error")
    assert tot["skipped"] == 0 and tot["nodes"] == int(np.sum(nd.astype(np.uint64)))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def check_both(ctx, m, hists, ref, max_nodes=MAXN):
    """Host and device entry against the reference."""
    batch, st, nd, w, asm, tot = run_host(ctx, m, hists, max_nodes)
    assert_results(m, hists, ref, st, nd, w, asm, batch.hdr, tot, max_nodes)
    assert same((st, nd, w, asm, tot), run_device(ctx, batch.hdr, batch.events, max_nodes))
    return batch, st, nd, w, asm


class budget_knob:
    def __init__(self, ctx, value):
        self.ctx, self.value = ctx, value

    def __enter__(self):
        self.saved = self.ctx.get_param("table_budget")
        self.ctx.set_param("table_budget", self.value)

    def __exit__(self, *exc):
        self.ctx.set_param("table_budget", self.saved)
        return False


# ------------------------------------------------------------------ 1. KATs

def test_kats(ctx):
    reg, lock = table("register"), table("lock")
    ok = reg.resps.index("Ok")
    hists = [KAT_WRITE_SEEN, KAT_WRITE_UNSEEN]
    ref = reference(tg.REGISTER, hists)
    assert [(r[0], r[1]) for r in ref] == [("lin", 2), ("lin", 4)]
    batch, st, nd, w, asm = check_both(ctx, reg, hists, ref)
    assert levels(batch.hdr, 0, w, asm) == ([0, 1], [ok, None])
    assert levels(batch.hdr, 1, w, asm) == ([1, 0], [None, ok])
    hists = [KAT_LONE_UNLOCK, KAT_UNLOCK_AND_FAILURE]
    ref = reference(tg.LOCK, hists)
    assert ref == [("lin", 0, []), ("nonlin", 1, [])]
    batch, st, nd, w, asm = check_both(ctx, lock, hists, ref)
    assert levels(batch.hdr, 0, w, asm) == ([], [])
    # the drop-in: None is today's call, "complete" the new one
    tr, post = reg.transition, reg.postcondition
    assert not linearisable(tr, post, None, KAT_WRITE_SEEN, ctx=ctx)
    assert linearisable(tr, post, None, KAT_WRITE_SEEN, ctx=ctx, pending="complete")
    assert not linearisable(lock.transition, lock.postcondition, None, KAT_LONE_UNLOCK, ctx=ctx)
    assert linearisable(lock.transition, lock.postcondition, None, KAT_LONE_UNLOCK, ctx=ctx, pending="complete")
    res = linearisable_batch(reg, [KAT_WRITE_SEEN, KAT_WRITE_UNSEEN], ctx=ctx, witness=True, pending="complete")
    assert [res.verdict(i) for i in range(2)] == ["lin", "lin"] and list(res.nodes) == [2, 4]
    assert res.witness_of(1) == [1, 0] and res.assumed_of(1) == [None, ok]
    assert replay_witness(reg, KAT_WRITE_UNSEEN, res.witness_of(1), None, assumed=res.assumed_of(1))
    assert linearisable_batch(reg, [KAT_WRITE_SEEN], ctx=ctx, witness=True).assumed is None


# ----------------------------------------------- 2. randomised crash batches

@functools.lru_cache(maxsize=None)
def crash_case(name, setting):
    """N_CRASH histories of a tablegen setting with clients crashed, and the
    reference's results (computed once, shared)."""
    c = CLOSURES[name]
    rng = random.Random(f"pending/crash/{name}/{setting}")
    hists = [pr.crash(h, rng, CRASH) for h in tg.gen_batch(c, setting, N_CRASH)]
    return hists, reference(c, hists)


@pytest.mark.parametrize("setting", ["3x10", "4x16", "6x24"])
@pytest.mark.parametrize("name", ["register", "lock", "counter"])
def test_crash_batches(ctx, name, setting):
    m = table(name)
    hists, ref = crash_case(name, setting)
    assert sum(1 for h in hists if pr.pending_invocations(h)) > N_CRASH // 3
    default = ctx.get_param("table_budget")
    assert default == 256
    for budget in (default, 0, 4):
        with budget_knob(ctx, budget):
            batch, st, nd, w, asm, tot = run_host(ctx, m, hists)
            pass2 = ctx.table_pass2()
            assert_results(m, hists, ref, st, nd, w, asm, batch.hdr, tot)
            want2 = sum(1 for r in ref if r[1] > budget or (r[0] == "budget" and r[1] >= budget)) if budget else 0
            assert pass2 == want2
            if budget != 0 or setting == "3x10":
                assert same((st, nd, w, asm, tot), run_device(ctx, batch.hdr, batch.events))
    assert not ctx.timed_out()
    assert any(a for r in ref for *_, a in r[2])
    if name == "counter":                   # the largest table: 80 KB beside the wider stack
        assert m.post_err is not None and len(m.states) == 256


# ------------------------------------------- 3. several allowed responses

PICKS = {3: 1, 7: 2, 31: 3}         # the symbols a Pick at state 0 allows -> the state they lead to
MASKED = 5                          # allowed by post, taken back by post_err


def pick_closures():
    def transition(s, ev):
        kind, x = ev
        if kind == "L":
            if x == "Reset":
                return 0
            return "picking" if (x == "Pick" and s == 0) else s
        if s == "picking":
            return PICKS.get(x, 3 if x == MASKED else 0)
        return s

    def postcondition(s, inv, r):
        if inv == "Pick":
            if s == 0 and r == MASKED:
                raise OracleModelError("masked")
            return s == 0 and r in PICKS
        return r == (0 if inv == "Reset" else s)        # Get -> the state

    return dict(name="pick", transition=transition, postcondition=postcondition, init=0,
                invs=["Pick", "Get", "Reset"], resps=list(range(32)))


@functools.lru_cache(maxsize=None)
def pick_table():
    c = pick_closures()
    m = TableModel.from_closures(c["transition"], c["postcondition"], 0, c["invs"], c["resps"],
                                 raises=OracleModelError)
    # the masked symbol: its post bit set as well, so only post_err keeps it out
    m.post[m.state_index[0], m.inv_index["Pick"]] |= np.uint32(1 << MASKED)
    return c, m


def test_several_allowed_responses(ctx):
    c, m = pick_table()
    s0, pick = m.state_index[0], m.inv_index["Pick"]
    allowed = int(m.post[s0, pick]) & ~int(m.post_err[s0, pick])
    assert allowed == sum(1 << r for r in PICKS) and (int(m.post[s0, pick]) >> MASKED) & 1
    assert len({int(m.on_resp[m.on_inv[s0, pick], r]) for r in list(PICKS) + [MASKED]}) == 3
    get = lambda p, v: [(p, L("Get")), (p, R(v))]       # noqa: E731
    hists = [[(0, L("Pick"))] + get(1, v) for v in (1, 2, 3, 0)]
    # two pending Picks, the second after a Reset: the resume at both levels
    hists.append([(0, L("Pick")), (1, L("Reset")), (1, R(0)), (2, L("Pick"))] + get(3, 3))
    hists.append([(0, L("Pick"))] + get(1, 2) + [(1, L("Reset")), (1, R(0)), (2, L("Pick"))] + get(3, 3) + get(3, 1))
    ref = reference(c, hists)
    assert [(r[0], r[1]) for r in ref[:4]] == [("lin", 2), ("lin", 4), ("lin", 6), ("lin", 8)]
    assert [a for *_, a in ref[2][2]] == [True, False] and ref[2][2][0][2] == 31
    rng = random.Random("pending/pick")
    for _ in range(300):
        h = []
        for _ in range(rng.randint(1, 12)):
            p = rng.randrange(4)
            kind = rng.random()
            if kind < 0.3:
                h.append((p, L("Pick")))
            elif kind < 0.45:
                h += [(p, L("Reset")), (p, R(0))]
            else:
                h += get(p, rng.choice([0, 1, 2, 3, 3]))
        hists.append(h)
    ref = reference(c, hists)
    picked = {op[2] for r in ref for op in r[2] if op[3]}
    assert picked >= set(PICKS)                                     # the second and the third choice were needed
    assert {r[0] for r in ref} == {"lin", "nonlin"}
    for budget in (256, 0, 4):
        with budget_knob(ctx, budget):
            check_both(ctx, m, hists, ref)


# ------------------------------------------------ 4. depth beyond n_ev / 2

@pytest.mark.parametrize("k", [20, 40, 100])
def test_depth_of_one_level_per_invocation(ctx, k):
    """k pids with a pending Write each, then one completed Read of the last
    write's value: k + 1 levels on k + 2 events."""
    m = table("register")
    vals = [1 + (i % 3) for i in range(k)]
    h = [(i, L(("Write", v))) for i, v in enumerate(vals)] + [(k, L("Read")), (k, R(("Val", vals[-1])))]
    assert len(h) == k + 2 and k + 1 > len(h) // 2
    # the width class filled: more pending Writes between the Read and its response (n_ev - 1
    # levels), and a history of pending Writes only (n_ev levels: a witness without a terminator)
    ev = {20: 32, 40: 64, 100: 128}[k]
    more = [(i, L(("Write", vals[-1]))) for i in range(k + 1, k + 1 + ev - len(h))]
    h2 = h[:-1] + more + h[-1:]
    h3 = [(i, L(("Write", 1 + (i % 3)))) for i in range(ev)]
    assert len(h2) == len(h3) == ev
    hists = [h, h2, h3]
    ref = reference(tg.REGISTER, hists)
    assert (ref[0][0], ref[0][1], len(ref[0][2])) == ("lin", k + 1, k + 1)
    assert (ref[1][0], ref[1][1], len(ref[1][2])) == ("lin", ev - 1, ev - 1)
    assert (ref[2][0], ref[2][1], len(ref[2][2])) == ("lin", ev, ev)
    for budget in (256, 0, 4):
        with budget_knob(ctx, budget):
            batch, st, nd, w, asm = check_both(ctx, m, hists, ref)
            wit, a = levels(batch.hdr, 0, w, asm)
            assert wit == list(range(k + 1)) and a == [m.resps.index("Ok")] * k + [None]
            assert len(levels(batch.hdr, 1, w, asm)[0]) == ev - 1 and len(levels(batch.hdr, 2, w, asm)[0]) == ev


def test_largest_table_in_the_widest_class(ctx):
    """The mod-256 counter (80 KB of tables with post_err) on 102 events: the
    128-event class's 48 KB of columns beside it in one workgroup.  100 pids
    with a pending `add 1` each, then a completed `add 0` that answers 100 mod
    32 (101 nodes) or a wrong value (every order of the pending ones fails:
    `budget`, through pass 2 as well)."""
    m = table("counter")
    assert m.post_err is not None and m.post.nbytes + m.post_err.nbytes + m.on_inv.nbytes + m.on_resp.nbytes == 80 << 10
    adds = [(i, L(1)) for i in range(100)]
    hists = [adds + [(100, L(0)), (100, R(100 % 32))], adds + [(100, L(0)), (100, R(5))]]
    ref = reference(CLOSURES["counter"], hists)
    assert [(r[0], r[1]) for r in ref] == [("lin", 101), ("budget", MAXN)]
    assert [op[2] for op in ref[0][2][:100]] == [(s + 1) % 32 for s in range(100)]
    for budget in (256, 0):
        with budget_knob(ctx, budget):
            check_both(ctx, m, hists, ref)
    assert not ctx.timed_out()


# ------------------------- 5. undo of an assumed level after a completed one

def test_undo_of_an_assumed_level_after_a_completed_operation(ctx):
    """p0 writes 1 (completed), then writes 2 and crashes; p1 reads 1.  The
    search assumes the second write first, fails at the read and must come
    back across the assumed level: restoring p0's highest removed response
    there would put the first write's Ok back."""
    m = table("register")
    w1 = [(0, L(("Write", 1))), (0, R("Ok")), (0, L(("Write", 2)))]
    hists = [w1 + [(1, L("Read")), (1, R(("Val", 1)))],
             w1 + [(1, L("Read")), (1, R(("Val", 3)))],
             w1 + [(1, L("Read")), (2, L(("Cas", 2, 3))), (1, R(("Val", 1))), (2, R("CasFail"))],
             w1 + [(1, L("Read")), (0, L(("Write", 3))), (1, R(("Val", 2))), (2, L("Read")), (2, R(("Val", 2)))]]
    ref = reference(tg.REGISTER, hists)
    assert (ref[0][0], ref[0][1]) == ("lin", 5)
    assert ref[0][2] == [(0, ("Write", 1), "Ok", False), (1, "Read", ("Val", 1), False), (0, ("Write", 2), "Ok", True)]
    assert ref[1][0] == "nonlin"
    for budget in (256, 0, 2):
        with budget_knob(ctx, budget):
            batch, st, nd, w, asm = check_both(ctx, m, hists, ref)
            assert levels(batch.hdr, 0, w, asm) == ([0, 3, 2], [None, None, m.resps.index("Ok")])


# ------------------------------------------------------ 6. any-shape histories

ANY_SETTINGS = {"6x14": 200, "2x62": 60, an.RANDOM: 500}


@functools.lru_cache(maxsize=None)
def anyshape_case(name, setting):
    c = CLOSURES[name]
    hists = an.batch(c, setting, ANY_SETTINGS[setting])
    return hists, reference(c, hists)


@pytest.mark.parametrize("setting", list(ANY_SETTINGS))
@pytest.mark.parametrize("name", ["register", "lock"])
def test_anyshape(ctx, name, setting):
    """Shared pids, stray and leading responses: whether a pid has a remaining
    response is decided at the node."""
    m = table(name)
    hists, ref = anyshape_case(name, setting)
    feats = set().union(*(an.census(h) for h in hists))
    assert feats == set(an.FEATURES)
    for budget in (256, 0, 4):
        with budget_knob(ctx, budget):
            check_both(ctx, m, hists, ref)
    assert not ctx.timed_out()


# ---------------------------------------------------------- 7. complete batches

@pytest.mark.parametrize("setting", ["4x16", "6x24"])
@pytest.mark.parametrize("name", ["register", "lock"])
def test_complete_batches_equal_the_check_call(ctx, name, setting):
    m = table(name)
    hists = tg.gen_batch(CLOSURES[name], setting, 300)
    assert not any(pr.pending_invocations(h) for h in hists)
    for budget in (256, 0):
        with budget_knob(ctx, budget):
            batch, st0, nd0, w0, tot0 = run_check_host(ctx, m, hists)
            _, st, nd, w, asm, tot = run_host(ctx, m, hists)
            assert np.array_equal(st, st0) and np.array_equal(nd, nd0) and np.array_equal(w, w0) and tot == tot0
            assert len(asm) == len(batch.events) and np.all(asm == NONE)
            assert same((st, nd, w, asm, tot), run_device(ctx, batch.hdr, batch.events))
    assert {"lin", "nonlin"} <= {codec.STATUS_NAMES[int(s)] for s in st}


# ------------------------------------------------------------------ 8. refusals

def test_refusals(ctx):
    m = table("register")
    ctx.set_table(m)
    batch = codec.encode(m, [KAT_WRITE_SEEN], None)
    for model_id in (1, 2, 4, 5):
        with pytest.raises(device.DeviceError, match=r"\(-4\)"):
            ctx.check_pending_arrays(model_id, batch.hdr, batch.events)
    with pytest.raises(device.DeviceError, match=r"\(-4\)"):
        ctx.check_pending_arrays(3, batch.hdr, batch.events, flags=EXH | device.QSMD_FLAG_EARLY_EXIT_BATCH)
    with pytest.raises(device.DeviceError, match=r"\(-1\)"):
        ctx.check_pending_arrays(6, batch.hdr, batch.events)
    fresh = device.Context(0, time_limit_ms=60000)
    try:
        with pytest.raises(device.DeviceError, match=r"\(-1\)"):
            fresh.check_pending_arrays(3, batch.hdr, batch.events)
    finally:
        fresh.close()
    with pytest.raises(NotImplementedError):
        linearisable_batch("bank", [[]], ctx=ctx, pending="complete")
    # the context still serves the call
    st, nd, _, _, _ = ctx.check_pending_arrays(3, batch.hdr, batch.events)
    assert (codec.STATUS_NAMES[int(st[0])], int(nd[0])) == ("lin", 2)
