"""GPU parity of the wide table-driven model (csrc/wtable.hip,
QSMD_MODEL_WTABLE): status, node count and witness of every history against
the literal oracle run with the models' own closures
(oracle/linearise_lists.py), against QSMD_MODEL_TABLE on the models both can
hold, and against tablememo.exact_count for the state memo with 16-bit states.
No history is left out of a comparison: the device runs with the oracle's
max_nodes, and a `budget` verdict must match too (nodes == max_nodes)."""

import ctypes
import functools
import random

import numpy as np
import pytest

import tablegen as tg
import tablememo as tm
import wtablegen as wg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device
from qsmd.linearisability import linearisable, linearisable_batch, replay_witness
from qsmd.models import TableModel

gpu = pytest.mark.gpu

EXH = device.QSMD_FLAG_EXHAUSTIVE
MAXN = tg.MAX_NODES
L, R = tg.L, tg.R
# (setting, histories) of the parity tests
PARITY = (("3x10", 500), ("4x16", 500), ("6x24", 200))


def oracle(name, hists, max_nodes=MAXN, model0=None):
    c = wg.BY_NAME[name]
    init = c["init"] if model0 is None else model0
    return [oracle_linearisable(c["transition"], c["postcondition"], init, h, max_nodes) for h in hists]


@functools.lru_cache(maxsize=None)
def parity_case(name, setting, n):
    """The histories of one generator setting and the oracle's results
    (computed once, shared)."""
    hists = tg.gen_batch(wg.BY_NAME[name], setting, n)
    return hists, oracle(name, hists)


def witness_path(hist, wit):
    """The operations (pid, inv, resp) a witness names (Lemma L1 replay)."""
    removed, path = set(), []
    for j in wit:
        pid, (_, inv) = hist[j]
        r = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "R" and p == pid)
        i0 = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "L" and p == pid)
        path.append((pid, inv, hist[r][1][1]))
        removed |= {i0, r}
    return path


def assert_results(m, hists, ref, status, nodes, wit, hdr, model0=None, totals=None, max_nodes=MAXN):
    assert len(status) == len(hists) == len(ref)
    for i, (h, (st_o, nd_o, path_o)) in enumerate(zip(hists, ref)):
        st = codec.STATUS_NAMES[int(status[i])]
        assert (st, int(nodes[i])) == (st_o, nd_o), (i, st, int(nodes[i]), st_o, nd_o)
        if st == "budget":
            assert int(nodes[i]) == max_nodes
        if st == "lin" and wit is not None:
            o, n = int(hdr[i]["ev_off"]), int(hdr[i]["n_ev"])
            w = []
            for x in wit[o:o + n]:
                if x == codec.WITNESS_END:
                    break
                w.append(int(x))
            assert witness_path(h, w) == path_o, i
            assert replay_witness(m, h, w, model0), i
    if totals is not None:
        names = [codec.STATUS_NAMES[int(s)] for s in status]
        assert totals["linearisable"] == names.count("lin")
        assert totals["nonlinearisable"] == names.count("nonlin")
        assert totals["model_errors"] == names.count("error")
        assert totals["encode_errors"] == names.count("encode")
        assert totals["budget"] == names.count("budget")
        assert totals["checked"] == names.count("lin") + names.count("nonlin") + names.count("error")
        assert totals["skipped"] == 0 and totals["nodes"] == int(np.sum(nodes.astype(np.uint64)))


def run_host(ctx, m, hists, model0=None, max_nodes=MAXN, flags=EXH):
    if ctx.wide_table is not m:
        ctx.set_wide_table(m)
    batch = codec.encode(m, hists, model0)
    assert not batch.encode_errors
    st, nd, w, tot = ctx.check_arrays(4, batch.hdr, batch.events, m.pack_model0(model0, {}), flags, max_nodes,
                                      witness=True)
    return batch, st, nd, w, tot


def run_device(ctx, hdr, ev, model0=None, max_nodes=MAXN, model_id=4):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = len(hdr)
    d_hdr = torch.from_numpy(hdr.view(np.uint8).copy()).to(dev)
    d_ev = torch.from_numpy(ev.view(np.uint8).copy()).to(dev)
    d_st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    d_nd = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    d_w = torch.full((max(len(ev), 1),), 0xFF, dtype=torch.uint8, device=dev)
    d_tot = torch.zeros(8, dtype=torch.int64, device=dev)
    ctx.check_device(model_id, d_hdr.data_ptr(), n, d_ev.data_ptr(), len(ev), d_st.data_ptr(), d_nd.data_ptr(),
                     d_w.data_ptr(), d_tot.data_ptr(), model0=model0, flags=EXH | device.QSMD_FLAG_WITNESS,
                     max_nodes=max_nodes, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tot = dict(zip((n for n, _ in device.Totals._fields_), (int(x) for x in d_tot.cpu().numpy())))
    return (d_st.cpu().numpy()[:n], d_nd.cpu().numpy().astype(np.uint64)[:n], d_w.cpu().numpy()[:len(ev)], tot)


def check_both(ctx, name, hists, model0=None, ref=None):
    """Host and device entry against the oracle."""
    m = wg.wide_table(name)
    ref = ref or oracle(name, hists, model0=model0)
    batch, st, nd, w, tot = run_host(ctx, m, hists, model0)
    assert_results(m, hists, ref, st, nd, w, batch.hdr, model0, tot)
    st2, nd2, w2, tot2 = run_device(ctx, batch.hdr, batch.events, m.pack_model0(model0, {}))
    assert np.array_equal(st, st2) and np.array_equal(nd, nd2) and np.array_equal(w, w2) and tot == tot2
    return st, nd


# --------------------------------------------------- 1. parity with the oracle

@gpu
@pytest.mark.parametrize("setting,n", PARITY)
@pytest.mark.parametrize("name", ["kv", "wcounter"])
def test_parity_with_the_oracle(ctx, name, setting, n):
    hists, ref = parity_case(name, setting, n)
    check_both(ctx, name, hists, ref=ref)
    assert ctx.table_pass2() == sum(1 for r in ref if r[1] > 256 or (r[0] == "budget" and r[1] >= 256))
    assert ctx.get_param("table_budget") == 256 and not ctx.timed_out()


@pytest.mark.parametrize("name", ["kv", "wcounter"])
def test_parity_inputs_reach_every_status_and_wide_states(name):
    seen, high = set(), 0
    for setting, n in PARITY:
        hists, ref = parity_case(name, setting, n)
        seen |= {r[0] for r in ref}
        high += sum(1 for h in hists if max(wg.state_indices_visited(name, h), default=0) >= 256)
    assert {"lin", "nonlin", "budget"} <= seen
    if name == "wcounter":
        assert "error" in seen
    assert high > 0
    m = wg.wide_table(name)
    codes = codec.encode(m, parity_case(name, "4x16", 500)[0]).events["code"]
    assert int(codes.max()) > 31


# ------------------------------------------------ 2. the same results as model 3

def narrow_closures(name):
    c = dict(wg.BY_NAME[name])
    if name == "ticket":                    # a dispenser that was reset before the history
        c["real"] = lambda n, inv: (0, "Ok") if inv == "Reset" else (n + 1, ("Number", n + 1))
        c["gen_init"] = 0
    return c


@gpu
@pytest.mark.parametrize("name", ["register", "lock", "ticket"])
def test_same_results_as_the_narrow_table(ctx, name):
    c = narrow_closures(name)
    narrow = TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                      raises=OracleModelError)
    wide = wg.wide_table(name)
    gen_model = dict(c, init=c.get("gen_init", c["init"]), name=f"{name}/both")
    hists = tg.gen_batch(gen_model, "4x16", 2000)
    batch = codec.encode(narrow, hists)
    assert not batch.encode_errors and (batch.hdr["model_id"] == 3).all()
    hdr4 = batch.hdr.copy()
    hdr4["model_id"] = 4
    ctx.set_table(narrow)
    ctx.set_wide_table(wide)
    a = ctx.check_arrays(3, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
    b = ctx.check_arrays(4, hdr4, batch.events, None, EXH, MAXN, witness=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3] and a[3]["encode_errors"] == 0
    assert {0, 1} <= set(a[0].tolist())
    if name == "lock":
        assert 2 in set(a[0].tolist())


# ------------------------------------------------------------------------ 3. BIG

@gpu
@pytest.mark.parametrize("model0", [65535, None])
def test_big_table(ctx, model0):
    c = wg.BIG if model0 is None else dict(wg.BIG, init=model0)
    hists = tg.gen_batch(c, "3x10", 200)
    st, _ = check_both(ctx, "big", hists, model0=model0)
    assert {0, 1} <= set(st.tolist())
    if model0 is not None:      # the wrap: some state index on both sides of it
        m = wg.wide_table("big")
        batch = codec.encode(m, hists[:8])
        with pytest.raises(device.DeviceError) as e:
            ctx.check_arrays(4, batch.hdr, batch.events, ctypes.c_uint32(65536), EXH, MAXN)
        assert rc_of(e) == -1
        assert linearisable(m.transition, m.postcondition, 65535,
                            [(0, L(1)), (0, R(0)), (0, L(0)), (0, R(0))], ctx=ctx)
        assert not linearisable(m.transition, m.postcondition, 65535, [(0, L(1)), (0, R(1))], ctx=ctx)


# ------------------------------------------------------- 4. width and pid edges

def seq_history(name, n_events, seed, p_bug=0.03):
    """A mostly sequential history (2 clients) of n_events events; an odd
    count ends with an invocation never answered, on a pid of its own."""
    c = wg.BY_NAME[name]
    rng = random.Random(f"wedge/{name}/{n_events}/{seed}")
    h = tg.gen_history(c, rng, 2, n_events // 2, p_bug)
    if n_events % 2:
        h.insert(rng.randrange(len(h) + 1), (2, L(rng.choice(c["invs"]))))
    return h


@gpu
@pytest.mark.parametrize("n_events", [1, 2, 32, 33, 64, 65, 128])
def test_event_count_edges(ctx, n_events):
    hists = [seq_history("kv", n_events, s) for s in range(24)]
    assert all(len(h) == n_events for h in hists)
    st, _ = check_both(ctx, "kv", hists)
    if n_events >= 32:
        assert {0, 1} <= set(st.tolist())


@gpu
def test_more_than_128_events(ctx):
    m = wg.wide_table("kv")
    good = seq_history("kv", 128, 0)
    batch = codec.encode(m, [good, good[:10]])
    # 130 events for history 0, then history 1
    ev = np.concatenate([batch.events[:128], batch.events[:2], batch.events[128:138]])
    hdr = batch.hdr.copy()
    hdr[0] = (0, 130, 2, 4, 0, 0)
    hdr[1] = (130, 10, 2, 4, 1, 0)
    ctx.set_wide_table(m)
    st, nd, _, tot = ctx.check_arrays(4, hdr, ev, None, EXH, MAXN)
    ref = oracle("kv", [good[:10]])[0]
    assert st[0] == codec.STATUS_ENCODE_ERROR and nd[0] == 0
    assert (codec.STATUS_NAMES[int(st[1])], int(nd[1])) == ref[:2]
    assert tot["encode_errors"] == 1 and tot["nodes"] == int(nd[1])


def spread_pids(hist, n_pids):
    """The same operations with operation k on pid k % n_pids."""
    out, cur, k = [], {}, 0
    for pid, (kind, x) in hist:
        if kind == "L":
            cur[pid] = k % n_pids
            k += 1
        out.append((cur[pid], (kind, x)))
    return out


@gpu
@pytest.mark.parametrize("n_pids", [1, 9, 64])
def test_pid_count_edges(ctx, n_pids):
    if n_pids == 64:        # 64 operations, one pid each
        hists = [spread_pids(seq_history("wcounter", 128, s), 64) for s in range(8)]
    elif n_pids == 1:       # every client on one pid (quirk Q1: shared pids)
        hists = [[(0, e) for _, e in h] for h in tg.gen_batch(wg.WCOUNTER, "3x10", 100, seed=7)]
    else:
        rng = random.Random(f"wpids/{n_pids}")
        hists = []
        while len(hists) < 16:
            h = tg.gen_history(wg.WCOUNTER, rng, n_pids, 2 * n_pids, 0.03)
            if len({p for p, _ in h}) == n_pids:
                hists.append(h)
    assert all(len({p for p, _ in h}) == n_pids for h in hists)
    check_both(ctx, "wcounter", hists)


@gpu
def test_mixed_width_classes(ctx):
    hists = []
    for s in range(30):
        hists += [seq_history("wcounter", n, s, p_bug=0.05) for n in (8, 32, 40, 64, 70, 128, 0, 33)]
    random.Random(5).shuffle(hists)
    st, _ = check_both(ctx, "wcounter", hists)
    assert {0, 1, 2} <= set(st.tolist())


@functools.lru_cache(maxsize=None)
def batch_size_case():
    hists = tg.gen_batch(wg.KV, "3x10", 65, seed=99)
    return hists, oracle("kv", hists)


@gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_size_edges(ctx, n):
    hists, ref = batch_size_case()
    st, _ = check_both(ctx, "kv", hists[:n], ref=ref[:n] if n else [])
    assert len(st) == n


# -------------------------------------------------------------------- 5. two passes

@gpu
def test_two_passes_give_the_same_arrays(ctx):
    m = wg.wide_table("kv")
    hists, ref = parity_case("kv", "6x24", 200)
    default = ctx.get_param("table_budget")
    out = {}
    try:
        for budget in (0, 1, 24, 256):
            ctx.set_param("table_budget", budget)
            batch, st, nd, w, tot = run_host(ctx, m, hists)
            out[budget] = (st, nd, w, tot)
            pass2 = ctx.table_pass2()
            if budget == 0:
                assert pass2 == 0
            else:
                assert pass2 == sum(1 for r in ref if r[1] > budget or (r[0] == "budget" and r[1] >= budget)) > 0
    finally:
        ctx.set_param("table_budget", default)
    assert_results(m, hists, ref, *out[0][:3], batch.hdr, None, out[0][3])
    for budget in (1, 24, 256):
        assert all(np.array_equal(x, y) for x, y in zip(out[0][:3], out[budget][:3])) and out[0][3] == out[budget][3]


# ------------------------------------------------------ 6. memo with wide states

def twin_reads(v, widths, answer=None):
    """REG512: Write v and Write v + 256 overlapped, then per round of width w,
    w overlapping reads answered Val (v + 256); the very last answer is Val 0
    (no order explains it).  In the order Write v + 256, Write v the register
    holds v and every read fails at once; in the other order it holds v + 256
    and the rounds are searched: the same remaining events below two states
    that agree in their low eight bits, with different subtree counts."""
    val = ("Val", v + 256 if answer is None else answer)
    h = [(0, L(("Write", v))), (1, L(("Write", v + 256))), (0, R("Ok")), (1, R("Ok"))]
    for w in widths:
        h += [(p, L("Read")) for p in range(w)] + [(p, R(val)) for p in range(w)]
    h[-1] = (h[-1][0], R(("Val", 0)))
    return h


def memo_rule_count(model, hist, state_bits):
    """The reference search with the kernel's memo rule -- a subtree the
    search backtracks out of is recorded with the nodes it counted, a descent
    into a recorded key counts them and backtracks -- in an unbounded table
    whose key keeps only the low ``state_bits`` bits of the state's index."""
    tr, post = model["transition"], model["postcondition"]
    index = wg.wide_table(model["name"]).state_index
    mask, memo = (1 << state_bits) - 1, {}

    def forest(es, state, root):
        kids = tm._children(hist, es)
        if not kids:
            return (not root), 0
        n = 0
        for j, r, es2 in kids:
            n += 1
            inv, resp = hist[j][1][1], hist[r][1][1]
            if not post(state, inv, resp):
                continue
            s2 = tr(tr(state, L(inv)), R(resp))
            key = (es2, index[s2] & mask)
            if key in memo:
                n += memo[key]
                continue
            out, sub = forest(es2, s2, False)
            n += sub
            if out:
                return True, n
            memo[key] = sub
        return False, n

    out, n = forest(tuple(range(len(hist))), model["init"], True)
    return ("lin" if out else "nonlin"), n


MEMO_SHAPES = ([3, 3, 3], [4, 4, 4], [4, 4], [5, 4, 3], [3, 2, 3, 2])


@functools.lru_cache(maxsize=None)
def memo_case():
    """130 histories (one workgroup: each lane slot serves several), the twin
    histories among plain ones, and exact_count's answers."""
    hists = []
    for k in range(130):
        v = (1, 5, 200)[k % 3]
        widths = MEMO_SHAPES[k % len(MEMO_SHAPES)]
        if k % 4 == 3:          # both writes, the reads answered with the low value: the other order is the deep one
            hists.append(twin_reads(v, widths, answer=v))
        else:
            hists.append(twin_reads(v, widths))
    return hists, [tm.exact_count(wg.REG512, h) for h in hists]


def test_memo_inputs_test_the_state_key():
    """A memo that kept eight bits of the state would count these histories
    wrongly: with sixteen the rule is exact."""
    hists, want = memo_case()
    assert all(s == "nonlin" and n > 256 for s, n in want)      # pass 2 takes every one
    for h, w in list(zip(hists, want))[:10]:
        assert memo_rule_count(wg.REG512, h, 16) == w
        assert memo_rule_count(wg.REG512, h, 8)[1] != w[1]
    m = wg.wide_table("reg512")
    assert m.state_index[257] == 257 and len(m.states) == 512


@gpu
@pytest.mark.parametrize("entries", [64, 1024])
def test_memo_with_wide_states(ctx, entries):
    m = wg.wide_table("reg512")
    hists, want = memo_case()
    ctx.set_wide_table(m)
    batch = codec.encode(m, hists)
    plain = ctx.check_arrays(4, batch.hdr, batch.events, None, EXH, 0, witness=True)
    try:
        ctx.set_param("table_memo", entries)
        ctx.set_param("table_memo_grid", 1)
        for _ in range(2):      # a second call: another epoch over the same tables
            st, nd, w, tot = ctx.check_arrays(4, batch.hdr, batch.events, None, EXH, 0, witness=True)
            assert [(codec.STATUS_NAMES[int(s)], int(n)) for s, n in zip(st, nd)] == want
            assert ctx.table_pass2() == len(hists) and ctx.table_memo_hits() > 0
            assert all(np.array_equal(x, y) for x, y in zip(plain[:3], (st, nd, w))) and plain[3] == tot
    finally:
        ctx.set_param("table_memo", 0)
        ctx.set_param("table_memo_grid", 0)


@gpu
def test_memo_decides_a_deep_tree(ctx):
    m = wg.wide_table("reg512")
    h = twin_reads(5, [4] * 7)
    want = tm.exact_count(wg.REG512, h)
    assert want[0] == "nonlin" and want[1] > 10 ** 9 and len(h) == 60
    res = linearisable_batch(m, [h, twin_reads(1, [3, 3])], ctx=ctx, table_memo=1024)
    assert (res.verdict(0), int(res.nodes[0])) == want
    assert (res.verdict(1), int(res.nodes[1])) == tm.exact_count(wg.REG512, twin_reads(1, [3, 3]))
    assert ctx.table_memo_hits() > 0 and not ctx.timed_out()
    assert ctx.get_param("table_memo") == 0 and ctx.wide_table is m


# ---------------------------------------------------------------------- 7. errors

def rc_of(exc):
    return int(str(exc.value).split("failed (")[1].split(")")[0])


def good_batch_still_checks(ctx, set_table=True):
    hists, ref = batch_size_case()
    m = wg.wide_table("kv")
    if set_table:
        batch, st, nd, w, tot = run_host(ctx, m, hists)
    else:                       # with the table the context holds
        batch = codec.encode(m, hists)
        st, nd, w, tot = ctx.check_arrays(4, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
    assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)


@gpu
def test_api_errors(ctx):
    m = wg.wide_table("kv")
    ctx.set_wide_table(m)
    hists, _ = batch_size_case()
    batch = codec.encode(m, hists[:8])
    lib, h = ctx._lib, ctx._h

    # qsmd_wtable_set: everything the kernel will index
    def struct(**kw):
        st = m.c_struct()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    bad_inv = m.on_inv.copy()
    bad_inv[1000, 104] = 1024
    bad_resp = m.on_resp.copy()
    bad_resp[0, 0] = 65535
    cases = [struct(n_states=0), struct(n_states=65537), struct(n_inv=0), struct(n_inv=257), struct(n_resp=0),
             struct(n_resp=257), struct(init_state=1024), struct(on_inv=None), struct(on_resp=None),
             struct(post=None), struct(on_inv=bad_inv.ctypes.data), struct(on_resp=bad_resp.ctypes.data)]
    for st in cases:
        assert lib.qsmd_wtable_set(h, ctypes.byref(st)) == -1
        assert lib.qsmd_last_error(h)
    assert lib.qsmd_wtable_set(h, None) == -1
    # a device copy over QSMD_WTABLE_MAX_BYTES: 2^23 records of two words, and on_resp
    ns, ni = 65536, 128
    z_inv, z_resp, z_post = np.zeros((ns, ni), np.uint16), np.zeros((ns, 1), np.uint16), np.zeros((ns, ni, 1), np.uint32)
    big = struct(n_states=ns, n_inv=ni, n_resp=1, on_inv=z_inv.ctypes.data, on_resp=z_resp.ctypes.data,
                 post=z_post.ctypes.data)
    assert ns * ni * 2 * 4 + ns * 2 > (64 << 20) and lib.qsmd_wtable_set(h, ctypes.byref(big)) == -1
    assert b"QSMD_WTABLE_MAX_BYTES" in lib.qsmd_last_error(h)
    good_batch_still_checks(ctx, set_table=False)       # the previous wide table is still set

    # check calls
    with pytest.raises(device.DeviceError) as e:
        ctx.check_arrays(4, batch.hdr, batch.events, ctypes.c_uint32(1024), EXH, MAXN)
    assert rc_of(e) == -1
    with pytest.raises(device.DeviceError) as e:
        ctx.check_arrays(4, batch.hdr, batch.events, None, EXH | device.QSMD_FLAG_EARLY_EXIT_BATCH, MAXN)
    assert rc_of(e) == -4
    with pytest.raises(device.DeviceError) as e:
        ctx.split_frontier(4, batch.hdr[:1], batch.events)
    assert rc_of(e) == -4
    with pytest.raises(device.DeviceError) as e:
        ctx.check_tasks(4, batch.hdr[:1], batch.events, np.zeros(1, dtype=device.TASK_DTYPE))
    assert rc_of(e) == -4
    with pytest.raises(device.DeviceError) as e:
        ctx.check_arrays(5, batch.hdr, batch.events, None, EXH, MAXN)
    assert rc_of(e) == -1
    good_batch_still_checks(ctx, set_table=False)
    # QSMD_FLAG_MEMO is accepted and changes nothing
    a = ctx.check_arrays(4, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
    b = ctx.check_arrays(4, batch.hdr, batch.events, None, EXH | device.QSMD_FLAG_MEMO, MAXN, witness=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]

    fresh = device.Context(0, time_limit_ms=60000)
    try:
        reg = TableModel.from_closures(tg.reg_transition, tg.reg_postcondition, 0, tg.REG_INVS, tg.REG_RESPS)
        fresh.set_table(reg)                # a narrow table is no wide table
        with pytest.raises(device.DeviceError) as e:
            fresh.check_arrays(4, batch.hdr, batch.events, None, EXH, MAXN)
        assert rc_of(e) == -1
        good_batch_still_checks(fresh)
    finally:
        fresh.close()


@gpu
def test_narrow_and_wide_tables_are_independent(ctx):
    """Alternating calls: setting either table leaves the other as it was."""
    reg = TableModel.from_closures(tg.reg_transition, tg.reg_postcondition, 0, tg.REG_INVS, tg.REG_RESPS)
    lock = TableModel.from_closures(tg.lock_transition, tg.lock_postcondition, False, tg.LOCK_INVS, tg.LOCK_RESPS,
                                    raises=OracleModelError)
    kv, wc = wg.wide_table("kv"), wg.wide_table("wcounter")
    data = {}
    for key, mod, clo in (("reg", reg, tg.REGISTER), ("lock", lock, tg.LOCK), ("kv", kv, wg.KV),
                          ("wc", wc, wg.WCOUNTER)):
        hists = tg.gen_batch(clo, "3x10", 96, seed=21)
        ref = [oracle_linearisable(clo["transition"], clo["postcondition"], clo["init"], h, MAXN) for h in hists]
        data[key] = (mod, hists, codec.encode(mod, hists), ref)

    def check(key):
        mod, hists, batch, ref = data[key]
        st, nd, w, tot = ctx.check_arrays(mod.model_id, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
        assert_results(mod, hists, ref, st, nd, w, batch.hdr, None, tot)

    ctx.set_table(reg)
    ctx.set_wide_table(kv)
    for key in ("reg", "kv", "reg"):
        check(key)
    ctx.set_wide_table(wc)                  # the narrow table stays
    for key in ("reg", "wc"):
        check(key)
    ctx.set_table(lock)                     # the wide table stays
    for key in ("wc", "lock", "wc"):
        check(key)
    assert ctx.table is lock and ctx.wide_table is wc
    # with the memo: the two paths share its tables, call by call
    try:
        ctx.set_param("table_memo", 64)
        ctx.set_param("table_budget", 1)
        for key in ("wc", "lock", "wc", "lock"):
            check(key)
    finally:
        ctx.set_param("table_memo", 0)
        ctx.set_param("table_budget", 256)
    # linearisable_batch sets the table the context does not hold
    res = linearisable_batch(kv, data["kv"][1][:64], max_nodes=MAXN, witness=True, ctx=ctx)
    assert ctx.wide_table is kv and ctx.table is lock
    assert_results(kv, data["kv"][1][:64], data["kv"][3][:64], res.status, res.nodes, res.witness, res.batch.hdr)


@gpu
def test_encode_errors_inside_a_batch(ctx):
    m = wg.wide_table("kv")
    hists = tg.gen_batch(wg.KV, "3x10", 70, seed=11)
    ref = oracle("kv", hists)
    batch = codec.encode(m, hists)
    hdr, ev = batch.hdr.copy(), batch.events.copy()

    def event_of(i, resp):
        o, n = int(hdr[i]["ev_off"]), int(hdr[i]["n_ev"])
        return next(k for k in range(o, o + n) if bool(ev["kp"][k] & 0x80) == resp)

    bad = [3, 17, 40, 64, 69]
    hdr["model_id"][3] = 3                                   # a narrow-table history in a model-4 call
    ev["code"][event_of(17, False)] = len(m.invs)           # an invocation code == n_inv
    ev["code"][event_of(40, True)] = len(m.resps)           # a response code == n_resp
    hdr["n_ev"][64] = 129
    hdr["ev_off"][69] = len(ev) - int(hdr["n_ev"][69]) + 1   # ev_off + n_ev > n_events
    ctx.set_wide_table(m)
    for entry in ("host", "device"):
        if entry == "host":
            st, nd, w, tot = ctx.check_arrays(4, hdr, ev, None, EXH, MAXN, witness=True)
        else:
            st, nd, w, tot = run_device(ctx, hdr, ev)
        for i in bad:
            assert st[i] == codec.STATUS_ENCODE_ERROR and nd[i] == 0, i
        keep = [i for i in range(len(hists)) if i not in bad]
        assert_results(m, [hists[i] for i in keep], [ref[i] for i in keep], st[keep], nd[keep], w, hdr[keep])
        assert tot["encode_errors"] == len(bad) and tot["nodes"] == int(nd.sum())


# ------------------------------------------------------------------- 8. time limit

@gpu
def test_time_limit(ctx):
    """64 reads of one key on 64 pids, fully overlapped, the last answer
    wrong: no order explains it and the search is far beyond any time."""
    m = wg.wide_table("kv")
    read = ("Read", 0)
    h = [(p, L(read)) for p in range(64)] + [(p, R(("Val", 0))) for p in range(63)] + [(63, R(("Val", 1)))]
    ctx.set_wide_table(m)
    batch = codec.encode(m, [h])
    try:
        ctx.set_time_limit_ms(200)
        st, nd, _, tot = ctx.check_arrays(4, batch.hdr, batch.events, None, EXH, 0)
        assert st[0] == codec.STATUS_BUDGET and ctx.timed_out()
        assert int(nd[0]) > 0 and tot["budget"] == 1 and tot["nodes"] == int(nd[0])
    finally:
        ctx.set_time_limit_ms(60000)
    good_batch_still_checks(ctx, set_table=False)
    assert not ctx.timed_out()
