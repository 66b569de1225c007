"""The keyed-table-model generator on the host (qsmd_gen_ktable_batch,
include/qsmd_gen.h; qsmd.gen.generate_ktable): byte parity with the Python
restatement of the header's definition (ktablegen_ref.py), equality with the
model-4 generator on the flat product and with the model-3 generator at one
key, shard and thread independence, the linearisability promise against the
literal oracle on the product closures, the weights' statistics, and
parameter validation.  No GPU."""

import collections
import ctypes
import functools
import math

import numpy as np
import pytest

import ktablegen_ref as ref
import ktgen_cases as kc
import tgen_cases as tc
from linearise_lists import ModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, gen
from qsmd.models import WideTableModel

N_PARITY = 200


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ------------------------------------------------------ 1. host = restatement

@functools.lru_cache(maxsize=None)
def restated(cid):
    """The restatement's batch of a case and the counters it moved (computed
    once, shared by the parity and the coverage test)."""
    _, name, keys, kw, first, ev_base, w, kwt = kc.case(cid)
    before = collections.Counter(ref.COUNTERS)
    out = ref.generate(kc.model(name, keys), first, N_PARITY, ev_base=ev_base, inv_weight=w, key_weight=kwt, **kw)
    moved = collections.Counter(ref.COUNTERS)
    moved.subtract(before)
    return out, moved


@pytest.mark.parametrize("cid", kc.CASE_IDS)
def test_host_equals_restatement(cid):
    c = kc.case(cid)
    hdr, ev, fl = kc.host(c, N_PARITY)
    (hdr_r, ev_r, fl_r), _ = restated(cid)
    assert hdr.tobytes() == hdr_r.tobytes()
    assert ev.tobytes() == ev_r.tobytes()
    assert fl.tobytes() == fl_r.tobytes()
    assert int(fl.max()) <= 3
    assert np.all(hdr["model_id"] == 5)
    resp = (ev["kp"] & 0x80) != 0
    assert np.all(ev["a"][resp] == 0) and np.all(ev["a"] < c[2])
    assert np.all(ev["b"] == 0) and np.all(ev["val"] == 0)


# ------------------------------------------------- 2. what the cases reach

def test_cases_reach_every_branch():
    total = collections.Counter()
    per_case = {}
    for cid in kc.CASE_IDS:
        per_case[cid] = restated(cid)[1]
        total.update(per_case[cid])
    for what in ("unit_pick", "general_scan", "fallback", "stuck", "bug_change", "bug_swap", "bug_noop"):
        assert total[what] > 0, what
    assert all(total["key", k] > 0 for k in range(8))
    # the fallback on the unit-weight pick and in the general scan, each followed by stuck steps
    for cid, path in (("lock2_fallback", "unit_pick"), ("lock3_fallback_w", "general_scan")):
        m = per_case[cid]
        assert m[path] > 0 and m["fallback"] > 0 and m["stuck"] > 0, cid
    # (on eight keys some key of the random component always accepts: no fallback there, stuck in-window)
    assert per_case["rand8_5x64"]["stuck"] > 0 and per_case["rand8_3x7_w"]["general_scan"] > 0
    m = per_case["full32_8_4x16"]
    assert m["w256"] == m["unit_pick"] > 0 and all(m["key", k] > 0 for k in range(8))
    for cid in ("reg1_4x16_bugs", "lock1_zero_inv", "lock1_fallback", "rand1_5x64"):      # the one-key pick
        assert per_case[cid]["unit_pick"] > 0 and per_case[cid]["general_scan"] == 0, cid
    assert per_case["lock1_fallback"]["fallback"] > 0 and per_case["rand1_5x64"]["stuck"] > 0
    assert per_case["one_resp2_single"]["bug_noop"] == N_PARITY
    assert per_case["one_resp2_swap"]["bug_swap"] == N_PARITY
    # a key or an invocation of weight 0 is never requested
    assert per_case["reg8_hot_key"]["key", 7] == 0 and per_case["reg4_zero_key"]["key", 1] == 0
    assert per_case["lock3_fallback_w"]["key", 1] == 0


# ------------------------------------------- 3. the flat product, by model 4

@functools.lru_cache(maxsize=None)
def flat(name, keys):
    p = kc.product(name, keys)
    return WideTableModel.from_closures(p["transition"], p["postcondition"], p["init"], p["invs"], p["resps"],
                                        raises=ModelError)


FLAT_WEIGHTS = {"register": (tuple(1 + i % 3 for i in range(21)), (0, 2, 5, 1, 1, 3, 1, 4)),
                "lock": ((6, 1, 6), (8, 1, 1, 1, 1, 1, 1, 0))}


@pytest.mark.parametrize("policy", [tc.AT_INVOKE, tc.IN_WINDOW])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name,keys", [("register", 2), ("register", 4), ("lock", 8)])
def test_equals_the_model_4_generator_on_the_flat_product(name, keys, weighted, policy):
    """One draw per request over the pairs key-major: the keyed stream is the
    model-4 stream on the tabulated product with symbol k * n_inv + i and
    weight key_weight[k] * inv_weight[i]."""
    m, f = kc.model(name, keys), flat(name, keys)
    n_inv = len(m.component.invs)
    assert len(f.invs) == keys * n_inv and list(f.invs) == list(m.invs)
    iw, kw = FLAT_WEIGHTS[name] if weighted else (None, None)
    kw = None if kw is None else kw[:keys]
    sched = dict(n_clients=4, n_ops=16, prefix_ops=3, lin_policy=policy, pid_mode=tc.PER_CLIENT, overlap=3,
                 p_bug=0.5, seed=0xF1A7 + keys)
    n, first, ev_base = 1500, kc.LATER, 64
    tiled = None if not weighted else [kw[k] * iw[i] for k in range(keys) for i in range(n_inv)]
    hdr4, ev4, fl4 = gen.generate_table(gen.table_params(inv_weight=tiled, **sched), f, first, n, ev_base=ev_base)
    hdr5, ev5, fl5 = gen.generate_ktable(gen.ktable_params(inv_weight=iw, key_weight=kw, **sched), m, first, n,
                                         ev_base=ev_base)
    inv = (ev4["kp"] & 0x80) == 0
    ev4 = ev4.copy()
    ev4["a"][inv] = ev4["code"][inv] // n_inv
    ev4["code"][inv] = ev4["code"][inv] % n_inv
    hdr4 = hdr4.copy()
    assert np.all(hdr4["model_id"] == 4)
    hdr4["model_id"] = 5
    assert hdr5.tobytes() == hdr4.tobytes()
    assert ev5.tobytes() == ev4.tobytes()
    assert fl5.tobytes() == fl4.tobytes()
    assert np.any(fl5 & 1) and len(np.unique(ev5["a"][inv])) == (keys if not weighted else np.count_nonzero(kw))


# ------------------------------------------------- 4. one key is model 3

@pytest.mark.parametrize("name,w", [("register", None), ("lock", (6, 1, 6)), ("rand_narrow", None)])
def test_one_key_equals_the_model_3_generator(name, w):
    sched = dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT, p_bug=0.5,
                 seed=0x0E1)
    hdr3, ev3, fl3 = gen.generate_table(gen.table_params(inv_weight=w, **sched), tc.model(name), 7, 1500)
    hdr5, ev5, fl5 = gen.generate_ktable(gen.ktable_params(inv_weight=w, **sched), kc.model(name, 1), 7, 1500)
    assert np.all(hdr3["model_id"] == 3) and np.all(hdr5["model_id"] == 5)
    hdr3 = hdr3.copy()
    hdr3["model_id"] = 5
    assert hdr5.tobytes() == hdr3.tobytes() and ev5.tobytes() == ev3.tobytes() and fl5.tobytes() == fl3.tobytes()


# ---------------------------------------------------------------- 5. shards

@pytest.mark.parametrize("cid", ["reg4_4x16_bugs", "lock8_w", "reg4_later_shard"])
def test_shards_and_threads(cid):
    c = kc.case(cid)
    first, ev_base, per = c[4], c[5], 2 * c[3]["n_ops"]
    whole = kc.host(c, 100, threads=8)
    a, b = kc.host(c, 37, first=first), kc.host(c, 63, first=first + 37)
    assert np.concatenate([a[1], b[1]]).tobytes() == whole[1].tobytes()
    assert np.concatenate([a[2], b[2]]).tobytes() == whole[2].tobytes()
    h = whole[0][37:].copy()
    h["ev_off"] -= 37 * per                   # a shard's headers: its own ev_off, the global tag
    assert a[0].tobytes() == whole[0][:37].tobytes() and b[0].tobytes() == h.tobytes()
    assert int(whole[0]["ev_off"][0]) == ev_base
    assert np.array_equal(whole[0]["tag"], (first + np.arange(100)) & 0xFFFFFFFF)
    big = kc.host(c, 5000, threads=1)         # past the size below which one thread does the work
    assert same(big, kc.host(c, 5000, threads=3)) and same(big, kc.host(c, 5000, threads=8))
    assert same(whole, [x[:100 * k] for x, k in zip(big, (1, per, 1))])


# ------------------------------------------------------------ 6. the promise

PROMISE_MAX_NODES = 20000


def _never_raises(post):
    def quiet(m, inv, resp):
        try:
            return post(m, inv, resp)
        except ModelError:
            return False
    return quiet


@pytest.mark.parametrize("policy", [tc.AT_INVOKE, tc.IN_WINDOW])
@pytest.mark.parametrize("name,keys,shape", [("register", 4, (4, 16)), ("register", 8, (3, 10)),
                                             ("lock", 8, (4, 16)), ("lock", 2, (3, 10))])
def test_unflagged_histories_are_linearisable(name, keys, shape, policy):
    """Every per-client history with flag byte 0 is "lin" for the literal
    oracle on the product closures.  The register's are asserted with no
    exception.  The lock raises (post_err): in-window the reference's search
    may raise on a branch it tries before the witness (the header's caveat,
    test_table_gen_host.py's account of it); those are counted, held to 1 in
    20, and their witness is checked with the raising step made a failing
    one."""
    p, m = kc.product(name, keys), kc.model(name, keys)
    q = gen.ktable_params(n_clients=shape[0], n_ops=shape[1], prefix_ops=2, lin_policy=policy,
                          pid_mode=tc.PER_CLIENT, p_bug=0.0, seed=0xA11CE + keys,
                          inv_weight=tc.CLOSURES[name].get("weights"))
    n = 300
    hdr, ev, fl = gen.generate_ktable(q, m, 0, n)
    assert not np.any(fl & 1)
    if policy == tc.AT_INVOKE:
        assert not np.any(fl)       # the state cannot move between a request and its execution
    may_raise_first = name == "lock" and policy == tc.IN_WINDOW
    checked = dropped = raised_first = 0
    for i in np.flatnonzero(fl == 0):
        h = kc.history(m, hdr, ev, i)
        st, _, _ = oracle_linearisable(p["transition"], p["postcondition"], p["init"], h, PROMISE_MAX_NODES)
        if st == "error" and may_raise_first:
            raised_first += 1
            st, _, _ = oracle_linearisable(p["transition"], _never_raises(p["postcondition"]), p["init"], h,
                                           PROMISE_MAX_NODES)
        if st == "budget":
            dropped += 1
            continue
        assert st == "lin", (i, st)
        checked += 1
    print(f"{name}^{keys} {shape} policy {policy}: checked {checked}, budget {dropped}, raised first {raised_first}")
    if name == "register":
        assert dropped == 0 and checked == np.count_nonzero(fl == 0)
    assert (dropped + raised_first) * 20 <= n, (dropped, raised_first, checked)
    assert checked > n // 2


# --------------------------------------------------------------- 7. weights

def test_zero_weights_never_appear_and_a_hot_key_gets_its_share():
    """Register: every state accepts a response for every invocation, so a
    request picks pair (k, i) with probability weight(k, i) / W exactly (up to
    below()'s 2^-32 granularity) and independently of every other request.
    Key 0's count over n requests is Binomial(n, p), p = key_weight[0] /
    sum(key_weight); the bound is six standard deviations."""
    kw, iw = (8, 1, 1, 1, 1, 1, 1, 0), [1] * 21
    iw[4] = iw[20] = 0
    m = kc.model("register", 8)
    q = gen.ktable_params(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT,
                          seed=78, inv_weight=iw, key_weight=kw)
    n_hist = 5000
    _, ev, _ = gen.generate_ktable(q, m, 0, n_hist)
    inv = ev[(ev["kp"] & 0x80) == 0]
    n = len(inv)
    assert n == n_hist * 16
    keys, codes = np.bincount(inv["a"], minlength=8), np.bincount(inv["code"], minlength=21)
    assert keys[7] == 0 and np.all(keys[:7] > 0)
    assert codes[4] == 0 and codes[20] == 0 and np.all(np.delete(codes, [4, 20]) > 0)
    p = kw[0] / sum(kw)
    bound = 6.0 * math.sqrt(n * p * (1.0 - p))
    assert abs(int(keys[0]) - n * p) <= bound, (int(keys[0]), n * p, bound)
    p1 = kw[1] / sum(kw)
    assert abs(int(keys[1]) - n * p1) <= 6.0 * math.sqrt(n * p1 * (1.0 - p1))


# ------------------------------------------------------------ 8. validation

def _call(p, comp_struct, n=8, first=0, ev_base=0):
    lib = gen._load()
    per = 2 * max(int(p.n_ops), 1)
    hdr = np.full(n, 0xA5, dtype=np.uint8).repeat(16).view(codec.HDR_DTYPE)
    ev = np.full(n * min(per, 128) * 8, 0xA5, dtype=np.uint8).view(codec.EV_DTYPE)
    fl = np.full(n, 0xA5, dtype=np.uint8)
    rc = lib.qsmd_gen_ktable_batch(ctypes.byref(p), ctypes.addressof(comp_struct) if comp_struct else None,
                                   first, n, ev_base, hdr.ctypes.data, ev.ctypes.data, fl.ctypes.data, 2)
    untouched = all(np.all(x.view(np.uint8) == 0xA5) for x in (hdr, ev, fl))
    return rc, untouched


GOOD = dict(n_keys=4, n_clients=4, n_ops=16, prefix_ops=4, lin_policy=1, pid_mode=0, p_bug=0.5, seed=1)
BAD = [("n_keys", 0), ("n_keys", 9), ("n_clients", 0), ("n_clients", 33), ("n_ops", 0), ("n_ops", 65),
       ("lin_policy", 2), ("pid_mode", 2), ("p_bug", float("nan")), ("p_bug", -0.01), ("p_bug", 1.01)]


def test_good_parameters_are_accepted():
    st = tc.model("register").c_struct()
    rc, untouched = _call(gen.ktable_params(**GOOD), st)
    assert rc == 0 and not untouched


@pytest.mark.parametrize("field,value", BAD)
def test_bad_parameter_is_rejected(field, value):
    st = tc.model("register").c_struct()
    rc, untouched = _call(gen.ktable_params(**dict(GOOD, **{field: value})), st)
    assert rc == -1 and untouched


def test_bad_weights_and_components_are_rejected():
    m = tc.model("register")
    st = m.c_struct()
    P = gen.ktable_params
    assert _call(P(inv_weight=[0] * 21, **GOOD), st) == (-1, True)
    assert _call(P(key_weight=[0] * 4, **GOOD), st) == (-1, True)
    # every pairwise product zero although neither array is
    assert _call(P(inv_weight=[0] * 21, key_weight=[1, 2, 3, 4], **GOOD), st) == (-1, True)
    # a sum past 2^32 - 1: within one array, across keys, and in one product
    assert _call(P(inv_weight=[1 << 31, 1 << 31] + [0] * 19, key_weight=[1, 0, 0, 0], **GOOD), st) == (-1, True)
    assert _call(P(inv_weight=[1 << 31] + [0] * 20, key_weight=[1, 1, 0, 0], **GOOD), st) == (-1, True)
    assert _call(P(inv_weight=[1 << 16] + [0] * 20, key_weight=[1 << 16, 0, 0, 0], **GOOD), st) == (-1, True)
    assert _call(P(inv_weight=[(1 << 32) - 1] + [0] * 20, key_weight=[0, 0, 1, 0], **GOOD), st)[0] == 0
    assert _call(P(inv_weight=[(1 << 16) + 1] + [0] * 20, key_weight=[0, (1 << 16) - 1, 0, 0], **GOOD), st)[0] == 0
    assert _call(P(**GOOD), None) == (-1, True)                    # no component
    assert _call(P(**GOOD), st, ev_base=(1 << 32) - 100) == (-1, True)   # ev_off past u32
    # what qsmd_ktable_set rejects: a transition out of range, a missing table, init_state, a wide dimension
    bad = m.c_struct()
    on_inv = m.on_inv.copy()
    on_inv[2, 3] = len(m.states)
    bad.on_inv = on_inv.ctypes.data
    assert _call(P(**GOOD), bad) == (-1, True)
    bad = m.c_struct()
    on_resp = m.on_resp.copy()
    on_resp[1, 2] = len(m.states)
    bad.on_resp = on_resp.ctypes.data
    assert _call(P(**GOOD), bad) == (-1, True)
    bad = m.c_struct()
    bad.post = None
    assert _call(P(**GOOD), bad) == (-1, True)
    bad = m.c_struct()
    bad.init_state = len(m.states)
    assert _call(P(**GOOD), bad) == (-1, True)
    for field, value in (("n_inv", 33), ("n_resp", 33), ("n_states", 257), ("n_states", 0)):
        bad = m.c_struct()
        setattr(bad, field, value)
        assert _call(P(**GOOD), bad) == (-1, True)


def test_python_binding_checks_the_weights_lengths():
    m = kc.model("register", 4)
    kw = {k: v for k, v in GOOD.items() if k != "n_keys"}
    with pytest.raises(ValueError):
        gen.generate_ktable(gen.ktable_params(inv_weight=[1, 2], **kw), m, 0, 4)
    with pytest.raises(ValueError):
        gen.generate_ktable(gen.ktable_params(key_weight=[1, 2, 3], **kw), m, 0, 4)
    with pytest.raises(ValueError):
        gen.generate_ktable(gen.ktable_params(**dict(kw, n_clients=40)), m, 0, 4)


# ------------------------------------ 9. the table generator keeps to 3 and 4

def test_qsmd_gen_table_batch_still_rejects_model_5():
    reg = tc.model("register")
    p = gen.table_params(n_clients=4, n_ops=16, prefix_ops=4)
    p.model_id = 5
    st = reg.c_struct()
    hdr = np.zeros(4, dtype=codec.HDR_DTYPE)
    ev = np.zeros(4 * 32, dtype=codec.EV_DTYPE)
    rc = gen._load().qsmd_gen_table_batch(ctypes.byref(p), ctypes.addressof(st), 0, 4, 0, hdr.ctypes.data,
                                          ev.ctypes.data, None, 1)
    assert rc == -1 and not hdr.view(np.uint8).any() and not ev.view(np.uint8).any()
