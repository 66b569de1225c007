"""GPU parity of the keyed model's local mode (csrc/ksplit.hip, knob
"ktable_local"): status and node count of every history against the literal
restatement (tests/ktablelocal_ref.py: the split, the literal oracle with the
component's closures on every key's part, the combine rule); the histories the
restatement does not split against a knob-0 call on the same batch.  No history
is left out: the device runs with the restatement's max_nodes, and a `budget`
must match too."""

import functools
import random

import numpy as np
import pytest

import ktablegen as kg
import ktablelocal_ref as ref
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device
from qsmd.linearisability import linearisable, linearisable_batch
from qsmd.models import KeyedTableModel, ModelError, TableModel, WideTableModel

pytestmark = pytest.mark.gpu

EXH = device.QSMD_FLAG_EXHAUSTIVE
MAXN = tg.MAX_NODES
COMPONENTS = {"register": tg.REGISTER, "lock": tg.LOCK}
CODE = {"lin": 1, "nonlin": 0, "error": 2, "encode": 3, "budget": 4}


@pytest.fixture(scope="module")
def ctx():
    c = device.Context(0, time_limit_ms=60000)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def component(name):
    c = COMPONENTS[name]
    return TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                    raises=OracleModelError)


@functools.lru_cache(maxsize=None)
def keyed(name, K):
    return KeyedTableModel(component(name), K)


@functools.lru_cache(maxsize=None)
def prod(name, K):
    return kg.product(COMPONENTS[name], K)


@functools.lru_cache(maxsize=None)
def generated(name, K, clients, ops, p_bug, n, seed=tg.SEED):
    rng = random.Random(f"{seed}/local/{name}/{K}/{clients}x{ops}/{p_bug}")
    return tuple(tuple(tg.gen_history(prod(name, K), rng, clients, ops, p_bug)) for _ in range(n))


def encode(name, K, hists, model0=None):
    batch = codec.encode(keyed(name, K), [list(h) for h in hists], model0)
    assert not batch.encode_errors
    return batch.hdr, batch.events


def run_host(ctx, name, K, hdr, ev, local, max_nodes=MAXN, model0=None, flags=EXH, witness=False):
    m = keyed(name, K)
    if ctx.keyed_table is not m:
        ctx.set_keyed_table(m)
    ctx.set_param("ktable_local", local)
    try:
        st, nd, w, tot = ctx.check_arrays(5, hdr, ev, m.pack_model0(model0, {}), flags, max_nodes, witness=witness)
        split = ctx.ktable_local_last()
    finally:
        ctx.set_param("ktable_local", 0)
    return st, nd, w, tot, split


class DeviceCall:
    """One qsmd_check_batch_device call on a stream, its buffers kept until
    read()."""

    def __init__(self, ctx, name, K, hdr, ev, local, stream, max_nodes=MAXN, model0=None):
        import torch
        m = keyed(name, K)
        if ctx.keyed_table is not m:
            ctx.set_keyed_table(m)
        dev = torch.device("cuda:0")
        self.n, self.torch = len(hdr), torch
        with torch.cuda.stream(stream):
            self.hdr = torch.from_numpy(hdr.view(np.uint8).copy()).to(dev)
            self.ev = torch.from_numpy(ev.view(np.uint8).copy()).to(dev) if len(ev) else \
                torch.zeros(8, dtype=torch.uint8, device=dev)
            self.st = torch.full((max(self.n, 1),), 0xEE, dtype=torch.uint8, device=dev)
            self.nd = torch.full((max(self.n, 1),), -1, dtype=torch.int64, device=dev)
            self.tot = torch.full((8,), -1, dtype=torch.int64, device=dev)
        ctx.set_param("ktable_local", local)
        try:
            ctx.check_device(5, self.hdr.data_ptr(), self.n, self.ev.data_ptr(), len(ev), self.st.data_ptr(),
                             self.nd.data_ptr(), None, self.tot.data_ptr(), model0=m.pack_model0(model0, {}),
                             flags=EXH, max_nodes=max_nodes, stream=stream.cuda_stream)
        finally:
            ctx.set_param("ktable_local", 0)

    def read(self):
        self.torch.cuda.synchronize()
        tot = dict(zip((n for n, _ in device.Totals._fields_), (int(x) for x in self.tot.cpu().numpy())))
        return self.st.cpu().numpy()[:self.n], self.nd.cpu().numpy().astype(np.uint64)[:self.n], tot


def run_device(ctx, name, K, hdr, ev, local, **kw):
    torch = pytest.importorskip("torch")
    call = DeviceCall(ctx, name, K, hdr, ev, local, torch.cuda.Stream(), **kw)
    st, nd, tot = call.read()
    return st, nd, tot, ctx.ktable_local_last()


def expected(ctx, name, K, hdr, ev, max_nodes=MAXN, model0=None):
    """[(status code, nodes)] per header and the number of split histories:
    the restatement's result, and for a history it does not split the knob-0
    call's."""
    want = ref.check_arrays(COMPONENTS[name], K, hdr, ev, max_nodes, model0)
    n_split = sum(w is not None for w in want)
    if n_split < len(want):
        st0, nd0, _, _, split0 = run_host(ctx, name, K, hdr, ev, 0, max_nodes, model0)
        assert split0 == 0
    return [(CODE[w[0]], w[1]) if w is not None else (int(st0[i]), int(nd0[i])) for i, w in enumerate(want)], n_split


def assert_equal(want, n_split, st, nd, tot, split):
    got = [(int(s), int(n)) for s, n in zip(st, nd)]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad and len(got) == len(want), bad[:5]
    count = lambda c: sum(1 for s, _ in want if s == c)     # noqa: E731
    assert tot == dict(checked=count(0) + count(1) + count(2), linearisable=count(1), nonlinearisable=count(0),
                       model_errors=count(2), encode_errors=count(3), budget=count(4), skipped=0,
                       nodes=sum(n for _, n in want))
    assert split == n_split


def check_local(ctx, name, K, hdr, ev, max_nodes=MAXN, model0=None, dev=True):
    """Knob 1 through the host entry (and the device entry) against the expectation."""
    want, n_split = expected(ctx, name, K, hdr, ev, max_nodes, model0)
    st, nd, _, tot, split = run_host(ctx, name, K, hdr, ev, 1, max_nodes, model0)
    assert_equal(want, n_split, st, nd, tot, split)
    if dev:
        assert_equal(want, n_split, *run_device(ctx, name, K, hdr, ev, 1, max_nodes=max_nodes, model0=model0))
    return want


# ---------------------------------------------------------- 1. parity batches

PARITY = [("register", 2, 4, 16, 0.03), ("register", 4, 4, 16, 0.05), ("lock", 4, 4, 16, 0.05),
          ("register", 8, 6, 24, 0.03)]


@pytest.mark.parametrize("name,K,clients,ops,p_bug", PARITY)
def test_parity_with_the_restatement(ctx, name, K, clients, ops, p_bug):
    hists = generated(name, K, clients, ops, p_bug, 300)
    hdr, ev = encode(name, K, hists)
    want = check_local(ctx, name, K, hdr, ev)
    assert not ctx.timed_out()
    seen = {s for s, _ in want}
    assert {0, 1} <= seen and (name != "lock" or 2 in seen)
    # the restatement on the arrays is the restatement on the histories
    assert want == [(CODE[s], n) for s, n in (ref.check(COMPONENTS[name], K, list(h), MAXN) for h in hists)]


# ------------------------------------------------- 2. what the mode is for

def test_decides_what_the_product_search_leaves_budget(ctx):
    p = prod("register", 8)
    hists = generated("register", 8, 6, 24, 0.03, 150)
    product = [oracle_linearisable(p["transition"], p["postcondition"], p["init"], list(h), MAXN)[0] for h in hists]
    hard = [h for h, s in zip(hists, product) if s == "budget"]
    assert hard
    hdr, ev = encode("register", 8, hard)
    st, nd, _, tot, split = run_host(ctx, "register", 8, hdr, ev, 0)
    assert split == 0 and set(st.tolist()) == {CODE["budget"]} and set(nd.tolist()) == {MAXN}
    assert tot["budget"] == len(hard)
    want = check_local(ctx, "register", 8, hdr, ev)
    assert all(s in (0, 1) for s, _ in want)


# ------------------------------------------- 3. the fallback in a mixed batch

def test_fallback_in_a_mixed_batch(ctx):
    name, K = "register", 4
    good = [list(h) for h in generated(name, K, 4, 16, 0.05, 40)]
    W = lambda p, k: (p, ("L", (k, ("Write", 1))))      # noqa: E731
    ok = lambda p: (p, ("R", "Ok"))                     # noqa: E731
    shared = [W(0, 1), W(0, 2), ok(0), ok(0), W(1, 1), ok(1)]       # a shared pid, operations overlapping
    cut = good[3][:-1]                                  # cut before its last response
    assert good[3][-1][1][0] == "R"
    starts_resp = [ok(0)] + good[4]
    hists = []
    for i, h in enumerate(good):
        hists.append(h)
        if i == 5:
            hists += [shared, cut, starts_resp]
    hists += [good[7], good[8], good[9], good[10], good[11], []]
    hdr, ev = encode(name, K, hists)
    hdr, ev = hdr.copy(), ev.copy()
    n = len(hists)

    def first(i, resp):
        o = int(hdr[i]["ev_off"])
        return o + next(k for k in range(int(hdr[i]["n_ev"])) if bool(ev["kp"][o + k] & 0x80) == resp)

    ev["a"][first(n - 6, False)] = K                    # a key >= n_keys
    ev["code"][first(n - 5, False)] = len(tg.REG_INVS)  # an invocation code >= n_inv
    ev["code"][first(n - 4, True)] = len(tg.REG_RESPS)  # a response code >= n_resp
    hdr["model_id"][n - 3] = 3
    # ev_off + n_ev > n_events: the last non-empty slot, one event longer
    hdr["n_ev"][n - 2] += 1
    assert int(hdr[n - 2]["ev_off"]) + int(hdr[n - 2]["n_ev"]) == len(ev) + 1 and hdr[n - 1]["n_ev"] == 0
    want, n_split = expected(ctx, name, K, hdr, ev)
    fallback = [6, 7, 8, n - 6, n - 5, n - 4, n - 3, n - 2]
    assert n_split == n - len(fallback)                 # (the empty history is split: into no part)
    assert [want[i][0] for i in fallback[3:]] == [CODE["encode"]] * 5 and want[n - 1] == (1, 0)
    st, nd, _, tot, split = run_host(ctx, name, K, hdr, ev, 1)
    assert_equal(want, n_split, st, nd, tot, split)
    assert_equal(want, n_split, *run_device(ctx, name, K, hdr, ev, 1))
    # the shared-pid and the cut history were searched (on the product), not refused
    assert want[6][1] > 0 and want[7][1] > 0


# ------------------------------------- 4. shapes at which the kernels can go wrong

@pytest.mark.parametrize("n_hist", [1, 63, 64, 65, 129])
def test_batch_sizes(ctx, n_hist):
    hists = generated("register", 4, 4, 16, 0.05, 300)[:n_hist]
    check_local(ctx, "register", 4, *encode("register", 4, hists))


def long_history(K, keys, clients, n_ops, seed, p_bug=0.0):
    """n_ops operations on the keys `keys` of register^K."""
    p = dict(prod("register", K))
    p["invs"] = [(k, i) for k in keys for i in tg.REG_INVS]
    return tg.gen_history(p, random.Random(f"local/long/{K}/{keys}/{seed}"), clients, n_ops, p_bug)


def test_two_event_histories(ctx):
    hists = [[(p, ("L", (k, inv))), (p, ("R", resp))] for p, k in ((0, 0), (5, 7), (127, 3))
             for inv, resp in (("Read", ("Val", 0)), ("Read", ("Val", 2)), (("Write", 3), "Ok"))]
    hdr, ev = encode("register", 8, hists)
    ev = ev.copy()
    for i, h in enumerate(hists):                       # the pids as written (the codec makes them dense)
        o = int(hdr[i]["ev_off"])
        ev["kp"][o:o + 2] = (ev["kp"][o:o + 2] & 0x80) | h[0][0]
    want = check_local(ctx, "register", 8, hdr, ev)
    assert [s for s, _ in want] == [1, 0, 1] * 3


@pytest.mark.parametrize("K,keys,clients", [(8, tuple(range(8)), 6), (8, (3,), 3), (1, (0,), 3)])
def test_128_event_histories(ctx, K, keys, clients):
    """On 8 keys the parts are in the 32-event class; on one key the part is
    the whole history."""
    hists = [long_history(K, keys, clients, 64, s, p_bug=0.02 * (s % 2)) for s in range(12)]
    assert all(len(h) == 128 for h in hists)
    hdr, ev = encode("register", K, hists)
    parts = ref.split_arrays(hdr[0], ev, len(ev), K, len(tg.REG_INVS), len(tg.REG_RESPS))
    assert [k for k, _ in parts] == list(keys)
    assert (max(len(idx) for _, idx in parts) <= 32) == (len(keys) == 8)
    check_local(ctx, "register", K, hdr, ev)


def test_128_events_on_64_pids(ctx):
    inv = lambda p, k, i: (p, ("L", (k, i)))            # noqa: E731
    hists = []
    for wrong in (None, 10, 62):
        h = []
        for p in range(0, 64, 2):                       # pairs of overlapping writes, then reads
            k = (p // 2) % 8
            if p % 4 == 0:
                h += [inv(p, k, ("Write", 1)), inv(p + 1, k, ("Write", 2)), (p, ("R", "Ok")), (p + 1, ("R", "Ok"))]
            else:
                v = 2 if p == wrong else 1
                h += [inv(p, k - 1, "Read"), inv(p + 1, k - 1, "Read"), (p, ("R", ("Val", 1))),
                      (p + 1, ("R", ("Val", v)))]
        hists.append(h)
    assert all(len(h) == 128 and len({p for p, _ in h}) == 64 for h in hists)
    hdr, ev = encode("register", 8, hists)
    ev = ev.copy()
    ev["kp"] = (ev["kp"] & 0x80) | (127 - (ev["kp"] & 0x7F))       # pids 64..127
    want = check_local(ctx, "register", 8, hdr, ev)
    assert len({s for s, _ in want}) == 2


def test_slots_out_of_order_with_gaps_and_at_the_end(ctx):
    hists = [list(h) for h in generated("register", 8, 6, 24, 0.03, 150)[:70]]
    hdr0, ev0 = encode("register", 8, hists)
    order = list(range(len(hists)))
    random.Random(11).shuffle(order)
    junk = np.zeros(1, dtype=codec.EV_DTYPE)
    junk["kp"], junk["code"], junk["a"] = 0xFF, 0xFF, 0xFF
    chunks, hdr, off = [], hdr0.copy(), 0
    for n, i in enumerate(order):                       # slot n holds history order[n], after a gap of n % 3 events
        gap = n % 3
        chunks += [junk] * gap
        off += gap
        o, k = int(hdr0[i]["ev_off"]), int(hdr0[i]["n_ev"])
        chunks.append(ev0[o:o + k])
        hdr["ev_off"][i] = off
        off += k
    ev = np.concatenate(chunks)
    last = order[-1]
    assert int(hdr[last]["ev_off"]) + int(hdr[last]["n_ev"]) == len(ev)     # a slot at the very end
    assert list(hdr["ev_off"]) != sorted(hdr["ev_off"])
    want = check_local(ctx, "register", 8, hdr, ev)
    assert want == check_local(ctx, "register", 8, hdr0, ev0, dev=False)
    # ev_off == n_events with no event
    hdr2 = np.concatenate([hdr, hdr[:1]])
    hdr2[-1] = (len(ev), 0, 0, 5, 0, 0)
    assert check_local(ctx, "register", 8, hdr2, ev, dev=False)[-1] == (1, 0)


# ------------------------------------------------------------------ 5. model0

def test_model0(ctx):
    start = (3, 0, 2, 1)
    p = dict(prod("register", 4), init=start)
    rng = random.Random("local/model0")
    hists = [tg.gen_history(p, rng, 3, 10, 0.05) for _ in range(300)]
    hdr, ev = encode("register", 4, hists, model0=start)
    want = check_local(ctx, "register", 4, hdr, ev, model0=start)
    plain = ref.check_arrays(tg.REGISTER, 4, hdr, ev, MAXN)
    lin_only_from_start = [i for i, (w, q) in enumerate(zip(want, plain)) if w[0] == 1 and q[0] != "lin"]
    assert len(lin_only_from_start) > 100


# --------------------------------------------------------------- 6. max_nodes

def test_max_nodes_applies_to_every_part(ctx):
    hists = generated("register", 4, 4, 16, 0.05, 300)
    hdr, ev = encode("register", 4, hists)
    want = check_local(ctx, "register", 4, hdr, ev, max_nodes=8)
    budget = [w for w in want if w[0] == CODE["budget"]]
    assert 0 < len(budget) < len(want)
    assert max(n for _, n in want) > 8                  # a sum over parts, each within the limit
    # a part that stopped is not the lowest failing one everywhere
    parts = [[ref.oracle_linearisable(tg.reg_transition, tg.reg_postcondition, 0, ref.unkeyed(sub), 8)[0]
              for _, sub in ref.split(tg.REGISTER, 4, list(h))] for h in hists]
    assert any("budget" in p and next(s for s in p if s != "lin") == "nonlin" for p in parts)


# --------------------------------------------------------- 7. knobs together

def test_with_the_memo_and_with_a_single_pass(ctx):
    hists = generated("register", 8, 6, 24, 0.03, 150)
    hdr, ev = encode("register", 8, hists)
    want = check_local(ctx, "register", 8, hdr, ev, dev=False)
    default = ctx.get_param("table_budget")
    try:
        ctx.set_param("table_budget", 8)
        ctx.set_param("ktable_memo", 64)
        check_local(ctx, "register", 8, hdr, ev, dev=False)
        assert ctx.table_pass2() > 0
        ctx.set_param("ktable_memo", 0)
        ctx.set_param("table_budget", 0)
        assert check_local(ctx, "register", 8, hdr, ev) == want
        assert ctx.table_pass2() == 0
    finally:
        ctx.set_param("ktable_memo", 0)
        ctx.set_param("table_budget", default)


def test_a_witness_call_takes_the_product_route(ctx):
    hists = generated("register", 4, 4, 16, 0.05, 300)[:100]
    hdr, ev = encode("register", 4, hists)
    a = run_host(ctx, "register", 4, hdr, ev, 0, witness=True)
    b = run_host(ctx, "register", 4, hdr, ev, 1, witness=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert a[4] == b[4] == 0
    local = run_host(ctx, "register", 4, hdr, ev, 1)
    assert local[4] == 100 and not np.array_equal(local[1], a[1])


def test_the_knob_itself(ctx):
    assert ctx.get_param("ktable_local") == 0
    ctx.set_param("ktable_local", 1)
    try:
        for bad in (2, 3, 1 << 40):
            with pytest.raises(device.DeviceError) as e:
                ctx.set_param("ktable_local", bad)
            assert int(str(e.value).split("failed (")[1].split(")")[0]) == -1
            assert ctx.get_param("ktable_local") == 1
    finally:
        ctx.set_param("ktable_local", 0)
    assert ctx.get_param("ktable_local") == 0


def test_no_effect_on_models_3_and_4(ctx):
    reg = component("register")
    p2 = prod("lock", 2)
    flat = WideTableModel.from_closures(p2["transition"], p2["postcondition"], p2["init"], p2["invs"], p2["resps"],
                                        raises=OracleModelError)
    ctx.set_table(reg)
    ctx.set_wide_table(flat)
    b3 = codec.encode(reg, tg.gen_batch(tg.REGISTER, "3x10", 100, seed=3))
    b4 = codec.encode(flat, tg.gen_batch(p2, "3x10", 100, seed=3))
    results = {}
    try:
        for local in (0, 1):
            ctx.set_param("ktable_local", local)
            results[local] = [ctx.check_arrays(mid, b.hdr, b.events, None, EXH, MAXN, witness=True)
                              for mid, b in ((3, b3), (4, b4))]
    finally:
        ctx.set_param("ktable_local", 0)
    for x, y in zip(results[0], results[1]):
        assert all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]
        assert {0, 1} <= set(x[0].tolist())


# -------------------------------------------------- 8. ordering and workspace

def test_workspace_regrown_between_calls():
    hists = generated("register", 4, 4, 16, 0.05, 300)
    c = device.Context(0, time_limit_ms=60000)
    try:
        for local, n in ((1, 64), (0, 300), (1, 300), (1, 10), (0, 10), (1, 129)):
            hdr, ev = encode("register", 4, hists[:n])
            if local:
                check_local(c, "register", 4, hdr, ev)
            else:
                st, nd, _, _, split = run_host(c, "register", 4, hdr, ev, 0)
                p = prod("register", 4)
                assert split == 0 and [(int(s), int(x)) for s, x in zip(st, nd)] == [
                    (CODE[r[0]], r[1]) for r in (oracle_linearisable(p["transition"], p["postcondition"], p["init"],
                                                                     list(h), MAXN) for h in hists[:n])]
    finally:
        c.close()


def test_two_calls_back_to_back_on_two_streams(ctx):
    torch = pytest.importorskip("torch")
    a = encode("register", 8, generated("register", 8, 6, 24, 0.03, 150))
    b = encode("register", 8, generated("register", 8, 4, 16, 0.05, 40))
    want_a, split_a = expected(ctx, "register", 8, *a)
    want_b, split_b = expected(ctx, "register", 8, *b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for second_local in (1, 0):                         # the second call reuses (knob 1) or leaves the workspace
        first = DeviceCall(ctx, "register", 8, *a, 1, s1)
        second = DeviceCall(ctx, "register", 8, *b, second_local, s2)
        st, nd, tot = first.read()
        assert_equal(want_a, split_a, st, nd, tot, split_a)
        st2, nd2, tot2 = second.read()
        if second_local:
            assert_equal(want_b, split_b, st2, nd2, tot2, ctx.ktable_local_last())
        else:
            st0, nd0, _, tot0, _ = run_host(ctx, "register", 8, *b, 0)
            assert np.array_equal(st2, st0) and np.array_equal(nd2, nd0) and tot2 == tot0


# ------------------------------------------------------ 9. the Python entries

def test_through_linearisable_batch_and_linearisable(ctx):
    m = keyed("lock", 4)
    hists = [list(h) for h in generated("lock", 4, 4, 16, 0.05, 300)[:60]]
    want = [ref.check(tg.LOCK, 4, h, MAXN) for h in hists]
    res = linearisable_batch(m, hists, max_nodes=MAXN, ctx=ctx, ktable_local=True)
    assert [(res.verdict(i), int(res.nodes[i])) for i in range(60)] == want
    assert ctx.ktable_local_last() == 60 and ctx.get_param("ktable_local") == 0
    res0 = linearisable_batch(m, hists, max_nodes=MAXN, ctx=ctx, ktable_local=False)
    assert ctx.ktable_local_last() == 0 and not np.array_equal(res0.nodes, res.nodes)
    ctx.set_param("ktable_local", 1)
    try:                                                # None leaves the context's knob alone
        res1 = linearisable_batch(m, hists, max_nodes=MAXN, ctx=ctx)
        assert np.array_equal(res1.nodes, res.nodes) and ctx.get_param("ktable_local") == 1
    finally:
        ctx.set_param("ktable_local", 0)
    assert {"lin", "nonlin", "error"} <= {w[0] for w in want}
    for h, (st, _) in list(zip(hists, want))[:30]:
        if st == "error":
            with pytest.raises(ModelError):
                linearisable(m.transition, m.postcondition, None, h, ctx=ctx, max_nodes=MAXN, ktable_local=True)
        else:
            assert linearisable(m.transition, m.postcondition, None, h, ctx=ctx, max_nodes=MAXN,
                                ktable_local=True) == (st == "lin")
        assert ctx.ktable_local_last() == 1
