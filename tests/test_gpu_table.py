"""GPU parity of the table-driven model (csrc/table.hip, QSMD_MODEL_TABLE):
status, node count and witness of every history against the literal oracle
run with the models' own closures (oracle/linearise_lists.py), and against the
existing TicketDispenser kernels on the same histories re-encoded for a ticket
table.  No history is left out of a comparison: the device runs with the
oracle's max_nodes, and a `budget` verdict must match too (nodes ==
max_nodes: the search order is the reference's)."""

import ctypes
import functools
import random

import numpy as np
import pytest

import tablegen as tg
from kats import KATS
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device, gen, models
from qsmd.linearisability import linearisable, linearisable_batch, replay_witness
from qsmd.models import TableModel

pytestmark = pytest.mark.gpu

EXH = device.QSMD_FLAG_EXHAUSTIVE
MAXN = tg.MAX_NODES
TICKET_K = 16


def counter_closures():
    """The largest table: a mod-256 counter, 32 x 32 symbols, with post_err."""
    def transition(s, ev):
        return (s + ev[1]) % 256 if ev[0] == "L" else s

    def postcondition(s, i, r):
        if s % 64 == 63 and i == 0:
            raise OracleModelError("counter at 63 mod 64")
        return r == (s + i) % 32

    def real(s, i):
        return (s + i) % 256, (s + i) % 32

    return dict(name="counter", transition=transition, postcondition=postcondition, init=0,
                invs=list(range(32)), resps=list(range(32)), real=real)


CLOSURES = {"register": tg.REGISTER, "lock": tg.LOCK, "ticket": tg.ticket_closures(TICKET_K),
            "counter": counter_closures()}


@functools.lru_cache(maxsize=None)
def table(name):
    c = CLOSURES[name]
    return TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                    raises=OracleModelError)


def oracle(name, hists, max_nodes=MAXN, model0=None):
    c = CLOSURES[name]
    init = c["init"] if model0 is None else model0
    return [oracle_linearisable(c["transition"], c["postcondition"], init, h, max_nodes) for h in hists]


@functools.lru_cache(maxsize=None)
def parity_case(name, setting):
    """The histories of one generator setting and the oracle's results
    (computed once, shared)."""
    hists = tg.gen_batch(CLOSURES[name], setting)
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


def assert_results(m, hists, ref, status, nodes, wit, hdr, model0=None, totals=None):
    assert len(status) == len(hists) == len(ref)
    for i, (h, (st_o, nd_o, path_o)) in enumerate(zip(hists, ref)):
        st = codec.STATUS_NAMES[int(status[i])]
        assert (st, int(nodes[i])) == (st_o, nd_o), (i, st, int(nodes[i]), st_o, nd_o)
        if st == "budget":
            assert int(nodes[i]) == MAXN
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
    if ctx.table is not m:
        ctx.set_table(m)
    batch = codec.encode(m, hists, model0)
    assert not batch.encode_errors
    st, nd, w, tot = ctx.check_arrays(3, batch.hdr, batch.events, m.pack_model0(model0, {}), flags, max_nodes,
                                      witness=True)
    return batch, st, nd, w, tot


def run_device(ctx, hdr, ev, model0=None, max_nodes=MAXN, model_id=3):
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
    m = table(name)
    ref = ref or oracle(name, hists, model0=model0)
    batch, st, nd, w, tot = run_host(ctx, m, hists, model0)
    assert_results(m, hists, ref, st, nd, w, batch.hdr, model0, tot)
    st2, nd2, w2, tot2 = run_device(ctx, batch.hdr, batch.events, m.pack_model0(model0, {}))
    assert np.array_equal(st, st2) and np.array_equal(nd, nd2) and np.array_equal(w, w2) and tot == tot2
    return st, nd


# ------------------------------------------------------------------ 1. KATs

def test_kats_in_table_form(ctx):
    m = table("ticket")
    names = ["KAT1_empty", "KAT2_reference_example", "KAT3_distinct_pids", "KAT4_lone_invocation",
             "KAT5_pending_is_leaf", "KAT6_response_first"]
    hists = [tg.ticket_symbols(KATS[k][1], TICKET_K) for k in names]
    want = [(KATS[k][2], KATS[k][3]) for k in names]
    ref = oracle("ticket", hists)
    assert [(r[0], r[1]) for r in ref] == want
    check_both(ctx, "ticket", hists, ref=ref)
    for h, (status, _) in zip(hists, want):     # one history per call: the drop-in
        assert linearisable(m.transition, m.postcondition, None, h, ctx=ctx) == (status == "lin")


# --------------------------------------------------- 2. parity with the oracle

@pytest.mark.parametrize("setting", sorted(tg.SETTINGS))
@pytest.mark.parametrize("name", ["register", "lock"])
def test_parity_with_the_oracle(ctx, name, setting):
    m = table(name)
    hists, ref = parity_case(name, setting)
    default = ctx.get_param("table_budget")
    assert default > 1
    over = sum(1 for r in ref if r[1] > 1)
    try:
        for budget in (default, 1, 0):
            ctx.set_param("table_budget", budget)
            assert ctx.get_param("table_budget") == budget
            batch, st, nd, w, tot = run_host(ctx, m, hists)
            assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)
            pass2 = ctx.table_pass2()
            if budget == 0:
                assert pass2 == 0
            elif budget == 1:       # every search that counts a second node
                assert pass2 == over > 0
            else:
                assert pass2 == sum(1 for r in ref if r[1] > budget or (r[0] == "budget" and r[1] >= budget))
    finally:
        ctx.set_param("table_budget", default)
    assert not ctx.timed_out()


@pytest.mark.parametrize("name", ["register", "lock"])
def test_parity_inputs_reach_every_status(name):
    seen = set()
    for setting in tg.SETTINGS:
        seen |= {r[0] for r in parity_case(name, setting)[1]}
    assert {"lin", "nonlin", "budget"} <= seen
    if name == "lock":
        assert "error" in seen


# ------------------------------------- 3. cross-check against the ticket kernels

def ticket_as_table(hdr, ev):
    hdr2, ev2 = hdr.copy(), ev.copy()
    hdr2["model_id"] = 3
    resp = (ev["kp"] & 0x80) != 0
    number = resp & (ev["code"] == 0)
    val = ev["val"].astype(np.int64)
    sym = np.where((val >= 1) & (val <= TICKET_K + 1), val, TICKET_K + 2)
    ev2["code"] = np.where(number, sym, np.where(resp, 0, ev["code"])).astype(np.uint8)
    ev2["val"] = 0
    return hdr2, ev2


@pytest.mark.parametrize("start", [None, 3])
def test_cross_check_with_the_ticket_kernels(ctx, start):
    m = table("ticket")
    assert m.resps[0] == "Ok" and m.resps[5] == ("Number", 5) and m.resps[TICKET_K + 2] == "Junk"
    hdr, ev, bug = gen.generate_config("ticket_2x10", 0, 4096, p_bug=0.5)
    assert (hdr["n_pid"] == 1).all() and 1024 < int(bug.sum()) < 3072
    m0 = None if start is None else models.TicketModel(1, 0, start)
    st_t, nd_t, w_t, tot_t = ctx.check_arrays(models.MODEL_TICKET, hdr, ev, m0, EXH, MAXN, witness=True)
    hdr2, ev2 = ticket_as_table(hdr, ev)
    ctx.set_table(m)
    st, nd, w, tot = ctx.check_arrays(3, hdr2, ev2, m.pack_model0(start, {}), EXH, MAXN, witness=True)
    assert np.array_equal(st, st_t) and np.array_equal(nd, nd_t) and np.array_equal(w, w_t)
    assert tot == tot_t
    assert {0, 1} <= set(st.tolist())


# ------------------------------------------------------ 4. edges of every class

def seq_history(name, n_events, seed, p_bug=0.03):
    """A mostly sequential history (2 clients) of n_events events."""
    rng = random.Random(f"edge/{name}/{n_events}/{seed}")
    return tg.gen_history(CLOSURES[name], rng, 2, n_events // 2, p_bug)


@pytest.mark.parametrize("n_events", [0, 2, 32, 34, 64, 66, 128])
def test_event_count_edges(ctx, n_events):
    hists = [seq_history("register", n_events, s) for s in range(24)]
    assert all(len(h) == n_events for h in hists)
    st, _ = check_both(ctx, "register", hists)
    if n_events >= 32:
        assert {0, 1} <= set(st.tolist())


def test_more_than_128_events(ctx):
    m = table("register")
    good = seq_history("register", 128, 0)
    batch = codec.encode(m, [good, good[:10]])
    # 130 events for history 0, then history 1
    ev = np.concatenate([batch.events[:128], batch.events[:2], batch.events[128:138]])
    hdr = batch.hdr.copy()
    hdr[0] = (0, 130, 2, 3, 0, 0)
    hdr[1] = (130, 10, 2, 3, 1, 0)
    ctx.set_table(m)
    st, nd, _, tot = ctx.check_arrays(3, hdr, ev, None, EXH, MAXN)
    ref = oracle("register", [good[:10]])[0]
    assert st[0] == codec.STATUS_ENCODE_ERROR and nd[0] == 0
    assert (codec.STATUS_NAMES[int(st[1])], int(nd[1])) == ref[:2]
    assert tot["encode_errors"] == 1


def spread_pids(hist, n_pids):
    """The same operations with operation k on pid k % n_pids."""
    out, cur, k = [], {}, 0
    for pid, (kind, x) in hist:
        if kind == "L":
            cur[pid] = k % n_pids
            k += 1
        out.append((cur[pid], (kind, x)))
    return out


@pytest.mark.parametrize("n_pids", [1, 8, 9, 64])
def test_pid_count_edges(ctx, n_pids):
    if n_pids == 64:        # 64 operations, one pid each
        hists = [spread_pids(seq_history("register", 128, s), 64) for s in range(8)]
    elif n_pids == 1:       # every client on one pid (quirk Q1: shared pids)
        hists = [[(0, e) for _, e in h] for h in tg.gen_batch(tg.REGISTER, "3x10", 200, seed=7)]
    else:                   # n_pids clients, overlapping
        rng = random.Random(f"pids/{n_pids}")
        hists = []
        while len(hists) < 16:
            h = tg.gen_history(tg.REGISTER, rng, n_pids, 2 * n_pids, 0.03)
            if len({p for p, _ in h}) == n_pids:
                hists.append(h)
    assert all(len({p for p, _ in h}) == n_pids for h in hists)
    check_both(ctx, "register", hists)


def test_100_pids_with_unanswered_invocations(ctx):
    """128 events: 28 complete operations and 72 invocations never answered,
    placed throughout, each on a pid of its own (100 pids)."""
    hists = []
    for s in range(8):
        rng = random.Random(f"lone/{s}")
        h = spread_pids(seq_history("register", 56, s, p_bug=0.02 * (s % 2)), 28)
        for k in range(72):
            h.insert(rng.randrange(len(h) + 1), (28 + k, ("L", rng.choice(tg.REG_INVS))))
        assert len(h) == 128 and len({p for p, _ in h}) == 100
        hists.append(h)
    check_both(ctx, "register", hists)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_size_edges(ctx, n):
    hists = tg.gen_batch(tg.REGISTER, "3x10", 4097, seed=99)[:n]
    ref = batch_size_reference()[:n]
    m = table("register")
    batch, st, nd, w, tot = run_host(ctx, m, hists)
    assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)
    if n in (65, 4097):
        st2, nd2, w2, tot2 = run_device(ctx, batch.hdr, batch.events)
        assert np.array_equal(st, st2) and np.array_equal(nd, nd2) and np.array_equal(w, w2) and tot == tot2


@functools.lru_cache(maxsize=None)
def batch_size_reference():
    return oracle("register", tg.gen_batch(tg.REGISTER, "3x10", 4097, seed=99))


def test_mixed_width_classes(ctx):
    hists = []
    for s in range(40):
        hists += [seq_history("lock", n, s, p_bug=0.05) for n in (8, 32, 40, 64, 70, 128, 0)]
    random.Random(5).shuffle(hists)
    st, _ = check_both(ctx, "lock", hists)
    assert {0, 1, 2} <= set(st.tolist())


# ---------------------------------------------------------------------- 5. errors

def rc_of(exc):
    return int(str(exc.value).split("failed (")[1].split(")")[0])


def good_batch_still_checks(ctx, name="register"):
    hists = tg.gen_batch(CLOSURES[name], "3x10", 64, seed=3)
    m = table(name)
    batch, st, nd, w, tot = run_host(ctx, m, hists)
    assert_results(m, hists, oracle(name, hists), st, nd, w, batch.hdr, None, tot)


def test_api_errors(ctx):
    m = table("register")
    ctx.set_table(m)
    hists = tg.gen_batch(tg.REGISTER, "3x10", 8, seed=3)
    batch = codec.encode(m, hists)
    lib, h = ctx._lib, ctx._h

    # qsmd_table_set: everything the kernel will index
    def struct(**kw):
        st = m.c_struct()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    bad_inv = m.on_inv.copy()
    bad_inv[3, 20] = 4
    bad_resp = m.on_resp.copy()
    bad_resp[0, 0] = 255
    cases = [struct(n_states=0), struct(n_states=257), struct(n_inv=0), struct(n_inv=33), struct(n_resp=0),
             struct(n_resp=33), struct(init_state=4), struct(on_inv=None), struct(on_resp=None),
             struct(post=None), struct(on_inv=bad_inv.ctypes.data), struct(on_resp=bad_resp.ctypes.data)]
    for st in cases:
        assert lib.qsmd_table_set(h, ctypes.byref(st)) == -1
        assert lib.qsmd_last_error(h)
    assert lib.qsmd_table_set(h, None) == -1
    good_batch_still_checks(ctx)        # the previous table is still set

    # check calls
    with pytest.raises(device.DeviceError) as e:
        ctx.check_arrays(3, batch.hdr, batch.events, ctypes.c_uint32(4), EXH, MAXN)
    assert rc_of(e) == -1
    good_batch_still_checks(ctx)
    with pytest.raises(device.DeviceError) as e:
        ctx.check_arrays(3, batch.hdr, batch.events, None, EXH | device.QSMD_FLAG_EARLY_EXIT_BATCH, MAXN)
    assert rc_of(e) == -4
    good_batch_still_checks(ctx)
    with pytest.raises(device.DeviceError) as e:
        ctx.split_frontier(3, batch.hdr[:1], batch.events)
    assert rc_of(e) == -4
    with pytest.raises(device.DeviceError) as e:
        ctx.check_tasks(3, batch.hdr[:1], batch.events, np.zeros(1, dtype=device.TASK_DTYPE))
    assert rc_of(e) == -4
    good_batch_still_checks(ctx)
    # QSMD_FLAG_MEMO is accepted and changes nothing
    a = ctx.check_arrays(3, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
    b = ctx.check_arrays(3, batch.hdr, batch.events, None, EXH | device.QSMD_FLAG_MEMO, MAXN, witness=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]

    fresh = device.Context(0, time_limit_ms=60000)
    try:
        with pytest.raises(device.DeviceError) as e:
            fresh.check_arrays(3, batch.hdr, batch.events, None, EXH, MAXN)
        assert rc_of(e) == -1
        good_batch_still_checks(fresh)
    finally:
        fresh.close()


def test_encode_errors_inside_a_batch(ctx):
    m = table("register")
    hists = tg.gen_batch(tg.REGISTER, "3x10", 70, seed=11)
    ref = oracle("register", hists)
    batch = codec.encode(m, hists)
    hdr, ev = batch.hdr.copy(), batch.events.copy()

    def event_of(i, resp):
        o, n = int(hdr[i]["ev_off"]), int(hdr[i]["n_ev"])
        return next(k for k in range(o, o + n) if bool(ev["kp"][k] & 0x80) == resp)

    bad = [3, 17, 40, 64, 69]
    hdr["model_id"][3] = 1
    ev["code"][event_of(17, False)] = len(m.invs)           # an invocation code >= n_inv
    ev["code"][event_of(40, True)] = len(m.resps)           # a response code >= n_resp
    hdr["n_ev"][64] = 129
    hdr["ev_off"][69] = len(ev) - int(hdr["n_ev"][69]) + 1   # ev_off + n_ev > n_events
    ctx.set_table(m)
    for entry in ("host", "device"):
        if entry == "host":
            st, nd, w, tot = ctx.check_arrays(3, hdr, ev, None, EXH, MAXN, witness=True)
        else:
            st, nd, w, tot = run_device(ctx, hdr, ev)
        for i in bad:
            assert st[i] == codec.STATUS_ENCODE_ERROR and nd[i] == 0, i
        keep = [i for i in range(len(hists)) if i not in bad]
        assert_results(m, [hists[i] for i in keep], [ref[i] for i in keep], st[keep], nd[keep], w, hdr[keep])
        assert tot["encode_errors"] == len(bad) and tot["nodes"] == int(nd.sum())
    # legal codes of a wider table are not legal here: every code is checked against this table
    assert len(m.resps) < len(table("counter").resps)


def test_replacing_the_table_between_calls(ctx):
    """The same arrays under two tables: each call is judged by its own."""
    reg = table("register")
    # a register whose Read answers are off by one: same shape, other verdicts
    odd = TableModel.from_closures(tg.reg_transition,
                                   lambda s, i, r: tg.reg_postcondition((s + 1) % 4 if i == "Read" else s, i, r),
                                   0, tg.REG_INVS, tg.REG_RESPS)
    hists = tg.gen_batch(tg.REGISTER, "3x10", 256, seed=21)
    batch = codec.encode(reg, hists)
    refs = {}
    for key, mod in (("reg", reg), ("odd", odd)):
        refs[key] = [oracle_linearisable(mod.transition, mod.postcondition, 0, h, MAXN) for h in hists]
    assert [r[:2] for r in refs["reg"]] != [r[:2] for r in refs["odd"]]
    for key, mod in (("reg", reg), ("odd", odd), ("reg", reg)):
        ctx.set_table(mod)
        st, nd, w, tot = ctx.check_arrays(3, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
        assert_results(mod, hists, refs[key], st, nd, w, batch.hdr, None, tot)
    # linearisable_batch sets the table the context does not hold
    assert ctx.table is reg
    res = linearisable_batch(odd, hists[:64], max_nodes=MAXN, witness=True, ctx=ctx)
    assert ctx.table is odd
    assert_results(odd, hists[:64], refs["odd"][:64], res.status, res.nodes, res.witness, res.batch.hdr)


# ---------------------------------------------------------------- 6. largest table

def test_largest_table(ctx):
    m = table("counter")
    assert (len(m.states), len(m.invs), len(m.resps)) == (256, 32, 32) and m.post_err is not None
    rng = random.Random("counter")
    hists = [tg.gen_history(CLOSURES["counter"], rng, 3, 10, 0.1) for _ in range(255)]
    # the raising postcondition: state 63, invocation 0
    hists.append([(0, ("L", 31)), (0, ("R", 31)), (0, ("L", 31)), (0, ("R", 30)), (0, ("L", 1)), (0, ("R", 31)),
                  (0, ("L", 0)), (0, ("R", 31))])
    st, _ = check_both(ctx, "counter", hists)
    assert st[255] == codec.STATUS_MODEL_ERROR and {0, 1} <= set(st.tolist())
    # from another initial state
    check_both(ctx, "counter", hists[:64], model0=200)


# ------------------------------------------------------------------- 7. time limit

def test_time_limit(ctx):
    """64 reads on 64 pids, fully overlapped, the last answer wrong: no order
    explains it and the search is far beyond any budget.  max_nodes is a
    second stop, so the run is bounded even if the limit were broken."""
    m = table("register")
    h = [(p, ("L", "Read")) for p in range(64)] + [(p, ("R", ("Val", 0))) for p in range(63)] + \
        [(63, ("R", ("Val", 1)))]
    max_nodes = 200_000_000
    ctx.set_table(m)
    batch = codec.encode(m, [h])
    try:
        ctx.set_time_limit_ms(5)
        st, nd, _, tot = ctx.check_arrays(3, batch.hdr, batch.events, None, EXH, max_nodes)
        assert st[0] == codec.STATUS_BUDGET and ctx.timed_out()
        assert 0 < int(nd[0]) < max_nodes
        assert tot["budget"] == 1 and tot["nodes"] == int(nd[0])
    finally:
        ctx.set_time_limit_ms(60000)
    good_batch_still_checks(ctx)
    assert not ctx.timed_out()
