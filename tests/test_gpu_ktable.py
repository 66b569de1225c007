"""GPU parity of the keyed table model (csrc/ktable.hip, QSMD_MODEL_KTABLE):
status, node count and witness of every history against the literal oracle run
on the product closures (tests/ktablegen.py), against model 3 at one key and
against model 4 on the flat product.  No history is left out of a comparison:
the device runs with the oracle's max_nodes, and a `budget` verdict must match
too (nodes == max_nodes)."""

import ctypes
import functools
import random

import numpy as np
import pytest

import ktablegen as kg
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device
from qsmd.linearisability import linearisable, linearisable_batch
from qsmd.models import KeyedTableModel, ModelError, TableModel, WideTableModel
from test_gpu_table import assert_results, counter_closures, rc_of, run_device

pytestmark = pytest.mark.gpu

EXH = device.QSMD_FLAG_EXHAUSTIVE
MAXN = tg.MAX_NODES
COMPONENTS = {"register": tg.REGISTER, "lock": tg.LOCK, "counter": counter_closures()}


@pytest.fixture(scope="module")
def ctx():
    """This module's own context.  The session's context must stay without a
    keyed table: tests/test_gpu_wtable.py expects a model-5 call on it to be
    refused, and a keyed table, once set, cannot be taken away."""
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


def oracle(name, K, hists, max_nodes=MAXN, model0=None):
    p = prod(name, K)
    init = p["init"] if model0 is None else model0
    return [oracle_linearisable(p["transition"], p["postcondition"], init, h, max_nodes) for h in hists]


@functools.lru_cache(maxsize=None)
def parity_case(name, K, setting):
    """The histories of one generator setting and the oracle's results
    (computed once, shared)."""
    hists = tg.gen_batch(prod(name, K), setting)
    return hists, oracle(name, K, hists)


def run_host(ctx, m, hists, model0=None, max_nodes=MAXN, flags=EXH):
    if ctx.keyed_table is not m:
        ctx.set_keyed_table(m)
    batch = codec.encode(m, hists, model0)
    assert not batch.encode_errors
    st, nd, w, tot = ctx.check_arrays(5, batch.hdr, batch.events, m.pack_model0(model0, {}), flags, max_nodes,
                                      witness=True)
    return batch, st, nd, w, tot


def check(ctx, name, K, hists, model0=None, ref=None, both=False):
    """The host entry (and the device entry) against the oracle."""
    m = keyed(name, K)
    ref = ref or oracle(name, K, hists, model0=model0)
    batch, st, nd, w, tot = run_host(ctx, m, hists, model0)
    assert_results(m, hists, ref, st, nd, w, batch.hdr, model0, tot)
    if both:
        st2, nd2, w2, tot2 = run_device(ctx, batch.hdr, batch.events, m.pack_model0(model0, {}), model_id=5)
        assert np.array_equal(st, st2) and np.array_equal(nd, nd2) and np.array_equal(w, w2) and tot == tot2
    return st, nd


# --------------------------------------------------- 1. parity with the oracle

PARITY = [("register", 4, "3x10"), ("register", 4, "4x16"), ("register", 4, "6x24"), ("lock", 8, "3x10"),
          ("lock", 8, "4x16"), ("register", 8, "4x16")]


@pytest.mark.parametrize("name,K,setting", PARITY)
def test_parity_with_the_oracle(ctx, name, K, setting):
    hists, ref = parity_case(name, K, setting)
    check(ctx, name, K, hists, ref=ref, both=setting == "4x16")
    assert not ctx.timed_out()
    if name == "register" and K == 8:       # the second state register is in use
        assert any(k >= 4 for h in hists for _, (kind, x) in h if kind == "L" for k in [x[0]])


def test_parity_inputs_reach_every_status():
    seen = {name: set() for name, _, _ in PARITY}
    for name, K, setting in PARITY:
        seen[name] |= {r[0] for r in parity_case(name, K, setting)[1]}
    assert {"lin", "nonlin", "budget"} <= seen["register"]
    assert {"lin", "nonlin", "error"} <= seen["lock"]


def test_drop_in_call(ctx):
    m = keyed("lock", 8)
    hists, ref = parity_case("lock", 8, "3x10")
    for h, (st, _, _) in list(zip(hists, ref))[:40]:
        if st == "error":
            with pytest.raises(ModelError):
                linearisable(m.transition, m.postcondition, None, h, ctx=ctx, max_nodes=MAXN)
        elif st != "budget":
            assert linearisable(m.transition, m.postcondition, None, h, ctx=ctx, max_nodes=MAXN) == (st == "lin")
    res = linearisable_batch(m, hists[:40], max_nodes=MAXN, ctx=ctx)
    assert [res.verdict(i) for i in range(40)] == [r[0] for r in ref[:40]]


# ------------------------------------------------------ 2. one key is model 3

def test_one_key_equals_model_3(ctx):
    reg = component("register")
    hists = tg.gen_batch(tg.REGISTER, "4x16")
    ctx.set_table(reg)
    b3 = codec.encode(reg, hists)
    r3 = ctx.check_arrays(3, b3.hdr, b3.events, None, EXH, MAXN, witness=True)
    m = keyed("register", 1)
    _, st, nd, w, tot = run_host(ctx, m, [[(p, (k, (0, x)) if k == "L" else (k, x)) for p, (k, x) in h] for h in hists])
    assert np.array_equal(st, r3[0]) and np.array_equal(nd, r3[1]) and np.array_equal(w, r3[2]) and tot == r3[3]
    assert {0, 1} <= set(st.tolist())


# ------------------------------------- 3. the flat product through model 4

@pytest.mark.parametrize("name,K,states", [("register", 2, 16), ("register", 4, 256), ("lock", 8, 256)])
def test_equals_the_flat_product(ctx, name, K, states):
    p = prod(name, K)
    flat = WideTableModel.from_closures(p["transition"], p["postcondition"], p["init"], p["invs"], p["resps"],
                                        raises=OracleModelError)
    assert len(flat.states) == states and len(flat.invs) == K * len(COMPONENTS[name]["invs"])
    hists = tg.gen_batch(p, "4x16", 600, seed=77)
    _, st, nd, w, tot = run_host(ctx, keyed(name, K), hists)
    ctx.set_wide_table(flat)
    b4 = codec.encode(flat, hists)
    assert not b4.encode_errors
    r4 = ctx.check_arrays(4, b4.hdr, b4.events, None, EXH, MAXN, witness=True)
    assert np.array_equal(st, r4[0]) and np.array_equal(nd, r4[1]) and np.array_equal(w, r4[2]) and tot == r4[3]
    assert {0, 1} <= set(st.tolist())


# ----------------------------------------------------- 4. the state's byte edges

def wrap_history(keys, last_ok=True):
    """Every key of `keys` takes 9 sequential operations of symbol 31 (0 ->
    ... -> 248 -> 23: through 255 -> 0), one pid per key, interleaved; then
    each key is read back with symbol 1."""
    h, s = [], {k: 0 for k in keys}
    for _ in range(9):
        for p, k in enumerate(keys):
            h += [(p, ("L", (k, 31))), (p, ("R", (s[k] + 31) % 32))]
            s[k] = (s[k] + 31) % 256
    assert all(v == 23 for v in s.values())
    for p, k in enumerate(keys):
        right = (s[k] + 1) % 32
        h += [(p, ("L", (k, 1))), (p, ("R", right if last_ok or p + 1 < len(keys) else (right + 1) % 32))]
    return h


def test_state_byte_edges(ctx):
    p = prod("counter", 8)
    hists = tg.gen_batch(p, "3x10", 500)
    hand = [wrap_history(keys, ok) for keys in ([7], [3], [7, 3], [0, 3, 4, 7]) for ok in (True, False)]
    # all eight keys at 255 (every byte of both registers full), stepped to 0 one by one
    full = [(0, e) for k in range(8) for e in (("L", (k, 1)), ("R", 0))]
    # key 5 to 63, where symbol 0 raises (post_err), after key 2 moved
    hand.append([(0, e) for e in (("L", (2, 7)), ("R", 7), ("L", (5, 31)), ("R", 31), ("L", (5, 31)), ("R", 30),
                                  ("L", (5, 1)), ("R", 31), ("L", (5, 0)), ("R", 31))])
    ref = oracle("counter", 8, hists + hand)
    assert [r[0] for r in ref[500:]] == ["lin", "nonlin"] * 4 + ["error"]
    st, _ = check(ctx, "counter", 8, hists + hand, ref=ref, both=True)
    assert {0, 1, 2} <= set(st.tolist())
    st, _ = check(ctx, "counter", 8, [full, full[:-1] + [(0, ("R", 1))]], model0=(255,) * 8)
    assert st.tolist() == [1, 0]


# ------------------------------------------------------- 5. undo across keys

def overlapped(keys, n_ops, shared_pids):
    """n_ops register operations, every invocation before every response,
    operation n on key keys[n % len(keys)]: writes and compare-and-swaps whose
    answers fit some orders, and last a read no order explains.  shared_pids:
    operations 2q and 2q + 1 are two clients on pid q (quirk Q1)."""
    ops = []
    for n in range(n_ops - 1):
        k = keys[n % len(keys)]
        ops.append(((k, ("Write", 1 + n % 2)), "Ok") if n % 3 else ((k, ("Cas", 0, 2)), "CasOk"))
    ops.append(((keys[0], "Read"), ("Val", 3)))
    pid = (lambda n: n // 2) if shared_pids else (lambda n: n)
    return [(pid(n), ("L", inv)) for n, (inv, _) in enumerate(ops)] + \
           [(pid(n), ("R", resp)) for n, (_, resp) in enumerate(ops)]


@pytest.mark.parametrize("shared_pids", [False, True])
def test_undo_across_keys(ctx, shared_pids):
    hists = [overlapped(keys, n, shared_pids) for keys in ([0, 7], [3, 4], list(range(8))) for n in (3, 4, 5, 6)]
    ref = oracle("register", 8, hists)
    assert all(r[0] == "nonlin" for r in ref) and max(r[1] for r in ref) > 150
    check(ctx, "register", 8, hists, ref=ref, both=True)


# ------------------------------------------------- 6. width classes and pids

def long_history(n_events, seed):
    rng = random.Random(f"ktable/long/{n_events}/{seed}")
    return tg.gen_history(prod("lock", 8), rng, 3, n_events // 2, 0.0)


def relabel_pids(batch):
    """Every history's dense pids spread over 0..127 (a bijection per
    history; pid 0 becomes 127): the reference only compares pids."""
    ev = batch.events.copy()
    for i, h in enumerate(batch.hdr):
        sl = slice(int(h["ev_off"]), int(h["ev_off"]) + int(h["n_ev"]))
        pid = ev["kp"][sl] & 0x7F
        ev["kp"][sl] = (ev["kp"][sl] & 0x80) | ((127 - 37 * pid.astype(np.int64) - 5 * i) % 128).astype(np.uint8)
    return ev


@functools.lru_cache(maxsize=None)
def long_case(n_events):
    hists = [long_history(n_events, s) for s in range(24)]
    assert all(len(h) == n_events for h in hists)
    return hists, oracle("lock", 8, hists)


@pytest.mark.parametrize("n_events", [30, 62, 126, 0])
def test_width_classes_and_pids(ctx, n_events):
    if n_events:
        hists, ref = long_case(n_events)
    else:                   # one batch that mixes all three classes
        hists, ref = [], []
        for n in (30, 62, 126):
            hists, ref = hists + long_case(n)[0], ref + long_case(n)[1]
        order = list(range(len(hists)))
        random.Random(5).shuffle(order)
        hists, ref = [hists[k] for k in order], [ref[k] for k in order]
    m = keyed("lock", 8)
    ctx.set_keyed_table(m)
    batch = codec.encode(m, hists)
    ev = relabel_pids(batch)
    assert 127 in (ev["kp"] & 0x7F)
    st, nd, w, tot = ctx.check_arrays(5, batch.hdr, ev, None, EXH, MAXN, witness=True)
    assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)
    st2, nd2, w2, tot2 = run_device(ctx, batch.hdr, ev, model_id=5)
    assert np.array_equal(st, st2) and np.array_equal(nd, nd2) and np.array_equal(w, w2) and tot == tot2


def test_more_than_128_events(ctx):
    m = keyed("lock", 8)
    good = long_history(128, 0)
    batch = codec.encode(m, [good, good[:10]])
    ev = np.concatenate([batch.events[:128], batch.events[:1], batch.events[128:138]])
    hdr = batch.hdr.copy()
    hdr[0] = (0, 129, 3, 5, 0, 0)
    hdr[1] = (129, 10, 3, 5, 1, 0)
    ctx.set_keyed_table(m)
    st, nd, _, tot = ctx.check_arrays(5, hdr, ev, None, EXH, MAXN)
    ref = oracle("lock", 8, [good[:10]])[0]
    assert st[0] == codec.STATUS_ENCODE_ERROR and nd[0] == 0
    assert (codec.STATUS_NAMES[int(st[1])], int(nd[1])) == ref[:2]
    assert tot["encode_errors"] == 1


# ------------------------------------------------------------- 7. two passes

def test_two_passes(ctx):
    m = keyed("register", 4)
    hists, ref = parity_case("register", 4, "4x16")
    default = ctx.get_param("table_budget")
    assert default > 8
    try:
        results = {}
        for budget in (0, 8, default):
            ctx.set_param("table_budget", budget)
            batch, st, nd, w, tot = run_host(ctx, m, hists)
            results[budget] = (st, nd, w, tot)
            pass2 = ctx.table_pass2()
            if budget == 0:
                assert pass2 == 0
            else:
                assert pass2 == sum(1 for r in ref if r[1] > budget or (r[0] == "budget" and r[1] >= budget)) > 0
        for budget in (8, default):
            assert all(np.array_equal(x, y) for x, y in zip(results[0][:3], results[budget][:3]))
            assert results[0][3] == results[budget][3]
        assert_results(m, hists, ref, *results[8][:3], batch.hdr, None, results[8][3])
        # the caller's budget, below and above pass 1's
        ref50 = oracle("register", 4, hists, max_nodes=50)
        assert 0 < sum(r[0] == "budget" for r in ref50) < len(hists)
        for budget in (8, default):
            ctx.set_param("table_budget", budget)
            _, st, nd, _, _ = run_host(ctx, m, hists, max_nodes=50)
            assert [(codec.STATUS_NAMES[int(s)], int(n)) for s, n in zip(st, nd)] == [r[:2] for r in ref50]
            assert all(int(n) == 50 for s, n in zip(st, nd) if s == codec.STATUS_BUDGET)
        # the state memo is not served: the knob changes nothing
        ctx.set_param("table_memo", 64)
        _, st, nd, w, tot = run_host(ctx, m, hists)
        assert all(np.array_equal(x, y) for x, y in zip((st, nd, w), results[0][:3])) and tot == results[0][3]
        assert ctx.table_pass2() > 0 and ctx.table_memo_hits() == 0
    finally:
        ctx.set_param("table_memo", 0)
        ctx.set_param("table_budget", default)


# ----------------------------------------------------------------- 8. model0

def test_model0(ctx):
    start = (3, 0, 2, 1)
    hists = tg.gen_batch(dict(prod("register", 4), init=start), "3x10", 400, seed=8)
    ref = oracle("register", 4, hists, model0=start)
    assert [r[:2] for r in ref] != [r[:2] for r in oracle("register", 4, hists)]
    st, _ = check(ctx, "register", 4, hists, model0=start, ref=ref, both=True)
    assert {0, 1} <= set(st.tolist())


# ----------------------------------------------------------------- 9. errors

def good_batch_still_checks(ctx, name="register", K=4):
    check(ctx, name, K, parity_case(name, K, "3x10")[0][:64], ref=parity_case(name, K, "3x10")[1][:64])


def test_table_set_errors(ctx):
    reg = component("register")
    ctx.set_keyed_table(keyed("register", 4))
    lib, h = ctx._lib, ctx._h

    def struct(**kw):
        st = reg.c_struct()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    bad_inv = reg.on_inv.copy()
    bad_inv[3, 20] = 4
    for st, n_keys in [(struct(), 0), (struct(), 9), (struct(on_inv=bad_inv.ctypes.data), 4),
                       (struct(n_states=257), 4), (struct(n_inv=33), 4), (struct(post=None), 4),
                       (struct(init_state=4), 4)]:
        assert lib.qsmd_ktable_set(h, ctypes.byref(st), n_keys) == -1
        assert lib.qsmd_last_error(h)
    assert lib.qsmd_ktable_set(h, None, 4) == -1
    good_batch_still_checks(ctx)        # the previous keyed table is still set


def test_call_errors(ctx):
    m = keyed("register", 4)
    ctx.set_keyed_table(m)
    batch = codec.encode(m, parity_case("register", 4, "3x10")[0][:8])
    with pytest.raises(device.DeviceError) as e:
        ctx.check_arrays(5, batch.hdr, batch.events, (ctypes.c_uint32 * 4)(0, 0, 4, 0), EXH, MAXN)
    assert rc_of(e) == -1
    with pytest.raises(device.DeviceError) as e:
        ctx.check_arrays(5, batch.hdr, batch.events, None, EXH | device.QSMD_FLAG_EARLY_EXIT_BATCH, MAXN)
    assert rc_of(e) == -4
    with pytest.raises(device.DeviceError) as e:
        ctx.split_frontier(5, batch.hdr[:1], batch.events)
    assert rc_of(e) == -4
    with pytest.raises(device.DeviceError) as e:
        ctx.check_tasks(5, batch.hdr[:1], batch.events, np.zeros(1, dtype=device.TASK_DTYPE))
    assert rc_of(e) == -4
    good_batch_still_checks(ctx)
    # QSMD_FLAG_MEMO is accepted and changes nothing
    a = ctx.check_arrays(5, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
    b = ctx.check_arrays(5, batch.hdr, batch.events, None, EXH | device.QSMD_FLAG_MEMO, MAXN, witness=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    fresh = device.Context(0, time_limit_ms=60000)
    try:
        fresh.set_table(component("register"))      # a narrow table is no keyed table
        with pytest.raises(device.DeviceError) as e:
            fresh.check_arrays(5, batch.hdr, batch.events, None, EXH, MAXN)
        assert rc_of(e) == -1
    finally:
        fresh.close()


def test_per_history_encode_errors(ctx):
    m = keyed("register", 4)
    ctx.set_keyed_table(m)
    hists, ref = parity_case("register", 4, "3x10")
    hists, ref = hists[:96], ref[:96]
    batch = codec.encode(m, hists)
    good = ctx.check_arrays(5, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
    assert_results(m, hists, ref, good[0], good[1], good[2], batch.hdr, None, good[3])

    def first_inv(i):
        o = int(batch.hdr[i]["ev_off"])
        return o + next(k for k in range(int(batch.hdr[i]["n_ev"])) if not batch.events["kp"][o + k] & 0x80)

    hdr, ev = batch.hdr.copy(), batch.events.copy()
    ev["a"][first_inv(5)] = 4                   # a key >= n_keys
    ev["a"][first_inv(6)] = 255
    ev["code"][first_inv(40)] = 21              # an invocation code >= n_inv
    resp70 = int(hdr[70]["ev_off"]) + int(hdr[70]["n_ev"]) - 1
    assert ev["kp"][resp70] & 0x80
    ev["code"][resp70] = 7                      # a response code >= n_resp
    hdr["model_id"][90] = 3
    broken = {5, 6, 40, 70, 90}
    st, nd, w, tot = ctx.check_arrays(5, hdr, ev, None, EXH, MAXN, witness=True)
    for i in range(96):
        if i in broken:
            assert st[i] == codec.STATUS_ENCODE_ERROR and nd[i] == 0, i
        else:
            assert (st[i], nd[i]) == (good[0][i], good[1][i]), i
            sl = slice(int(hdr[i]["ev_off"]), int(hdr[i]["ev_off"]) + int(hdr[i]["n_ev"]))
            assert np.array_equal(w[sl], good[2][sl])
    assert tot["encode_errors"] == 5
    assert tot["checked"] + tot["budget"] == 96 - 5
    # a response's `a`, and b / val anywhere, are ignored
    ev2 = batch.events.copy()
    ev2["a"][(ev2["kp"] & 0x80) != 0] = 200
    ev2["b"] = 9
    ev2["val"] = -1
    again = ctx.check_arrays(5, batch.hdr, ev2, None, EXH, MAXN, witness=True)
    assert all(np.array_equal(x, y) for x, y in zip(good[:3], again[:3])) and good[3] == again[3]


def test_three_tables_in_one_context(ctx):
    reg = component("register")
    p2 = prod("lock", 2)
    flat = WideTableModel.from_closures(p2["transition"], p2["postcondition"], p2["init"], p2["invs"], p2["resps"],
                                        raises=OracleModelError)
    km = keyed("register", 4)
    ctx.set_table(reg)
    ctx.set_wide_table(flat)
    ctx.set_keyed_table(km)
    h3 = tg.gen_batch(tg.REGISTER, "3x10", 64, seed=3)
    h4 = tg.gen_batch(p2, "3x10", 64, seed=3)
    h5, ref5 = parity_case("register", 4, "3x10")
    b3, b4, b5 = codec.encode(reg, h3), codec.encode(flat, h4), codec.encode(km, h5[:64])
    ref3 = [oracle_linearisable(tg.reg_transition, tg.reg_postcondition, 0, h, MAXN) for h in h3]
    ref4 = oracle("lock", 2, h4)
    for _ in range(2):
        for model_id, m, b, hists, ref in ((5, km, b5, h5[:64], ref5[:64]), (3, reg, b3, h3, ref3),
                                           (4, flat, b4, h4, ref4), (5, km, b5, h5[:64], ref5[:64])):
            st, nd, w, tot = ctx.check_arrays(model_id, b.hdr, b.events, None, EXH, MAXN, witness=True)
            assert_results(m, hists, ref, st, nd, w, b.hdr, None, tot)


# ------------------------------------------------------------ 10. time limit

def test_time_limit(ctx):
    """64 reads on 64 pids over the 8 keys, fully overlapped, the last answer
    wrong: no order explains it and the search is far beyond any budget.
    max_nodes is a second stop, so the run is bounded even if the limit were
    broken."""
    m = keyed("register", 8)
    h = [(p, ("L", (p % 8, "Read"))) for p in range(64)] + [(p, ("R", ("Val", 0))) for p in range(63)] + \
        [(63, ("R", ("Val", 1)))]
    max_nodes = 200_000_000
    ctx.set_keyed_table(m)
    batch = codec.encode(m, [h])
    try:
        ctx.set_time_limit_ms(5)
        st, nd, _, tot = ctx.check_arrays(5, batch.hdr, batch.events, None, EXH, max_nodes)
        assert st[0] == codec.STATUS_BUDGET and ctx.timed_out()
        assert 0 < int(nd[0]) < max_nodes
        assert tot["budget"] == 1 and tot["nodes"] == int(nd[0])
    finally:
        ctx.set_time_limit_ms(60000)
    good_batch_still_checks(ctx, "register", 4)
    assert not ctx.timed_out()
