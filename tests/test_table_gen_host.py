"""The table-model generator on the host (qsmd_gen_table_batch,
include/qsmd_gen.h; qsmd.gen.generate_table): byte parity with the Python
restatement of the header's definition (tablegen_ref.py), shard and thread
independence, the linearisability promise against the literal oracle, the
bug's and the weights' statistics, and parameter validation.  No GPU."""

import ctypes

import numpy as np
import pytest

import tablegen_ref as ref
import tgen_cases as tc
from linearise_lists import ModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, gen

N_PARITY = 2000


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ------------------------------------------------------ 1. host = restatement

@pytest.mark.parametrize("case", tc.CASES, ids=tc.CASE_IDS)
def test_host_equals_restatement(case):
    _, name, kw, first, ev_base, w = case
    hdr, ev, fl = tc.host(case, N_PARITY)
    hdr_r, ev_r, fl_r = ref.generate(tc.model(name), first, N_PARITY, ev_base=ev_base, inv_weight=w, **kw)
    assert hdr.tobytes() == hdr_r.tobytes()
    assert ev.tobytes() == ev_r.tobytes()
    assert fl.tobytes() == fl_r.tobytes()
    assert int(fl.max()) <= 3
    assert np.all(ev["a"] == 0) and np.all(ev["b"] == 0) and np.all(ev["val"] == 0)


def test_cases_reach_every_branch():
    """The settings above are only worth their time if they reach the stream's
    corners: stuck steps, the W = 0 fallback, both kinds of bug."""
    fl = tc.host(tc.CASES[tc.CASE_IDS.index("lock_fallback")], 500)[2]
    assert np.all(fl & 2)                                   # Unlock on an unlocked lock: always stuck
    fl = tc.host(tc.CASES[tc.CASE_IDS.index("rand_narrow_5x64")], 500)[2]
    assert 0 < np.count_nonzero(fl & 2) < 500
    fl = tc.host(tc.CASES[tc.CASE_IDS.index("one_resp_single")], 500)[2]
    assert not np.any(fl & 1)                               # one response symbol, one suffix response: no bug
    fl = tc.host(tc.CASES[tc.CASE_IDS.index("one_resp_swap")], 500)[2]
    assert np.all(fl & 1)


# ---------------------------------------------------------------- 2. shards

@pytest.mark.parametrize("cid", ["reg_4x16_bugs", "kv_3x10_w", "reg_32x64_shared"])
def test_shards_and_threads(cid):
    case = tc.CASES[tc.CASE_IDS.index(cid)]
    first, ev_base, per = case[3], case[4], 2 * case[2]["n_ops"]
    whole = tc.host(case, 5000, threads=8)
    assert same(whole, tc.host(case, 5000, threads=1))
    parts = [tc.host(case, hi - lo, first=first + lo) for lo, hi in ((0, 1), (1, 64), (64, 5000))]
    assert np.concatenate([p[1] for p in parts]).tobytes() == whole[1].tobytes()
    assert np.concatenate([p[2] for p in parts]).tobytes() == whole[2].tobytes()
    lo = 0
    for p in parts:                      # a shard's headers: its own ev_off, the global tag
        h = whole[0][lo:lo + len(p[0])].copy()
        h["ev_off"] -= lo * per
        assert h.tobytes() == p[0].tobytes()
        lo += len(p[0])
    assert int(whole[0]["ev_off"][0]) == ev_base
    assert np.array_equal(whole[0]["tag"], (first + np.arange(5000)) & 0xFFFFFFFF)


# ------------------------------------------------------------ 3. the promise

PROMISE_MAX_NODES = 20000


def _never_raises(post):
    def quiet(m, inv, resp):
        try:
            return post(m, inv, resp)
        except ModelError:
            return False
    return quiet


@pytest.mark.parametrize("policy", [tc.AT_INVOKE, tc.IN_WINDOW])
@pytest.mark.parametrize("shape", [(4, 16), (3, 10)])
@pytest.mark.parametrize("name", ["register", "lock", "kv"])
def test_unflagged_histories_are_linearisable(name, shape, policy):
    """Every history with flag byte 0 is "lin" for the literal oracle under the
    model's own closures, at most 1 in 20 left undecided by the node limit.

    One setting needs a second look.  The lock's postcondition raises
    (post_err), and with LIN_IN_WINDOW about 1 in 300 unflagged histories
    (measured: 1, 1, 1, 3, 1 of 300 at 4x16 over five seeds; 0, 0, 0, 1, 0 at
    3x10) come back "error", not "lin": two Unlocks overlap, a Lock lies
    between their linearisation points, and the reference search tries the
    two Unlocks back to back -- which raises -- before it reaches the witness.
    The history is linearisable, as the header promises; the reference's
    search raising first is the reference's semantics (the device checker
    reports MODEL_ERROR for it too).  For exactly that outcome the witness's
    existence is checked by the same oracle with the raising step made a
    failing one; any other verdict than "lin" fails the test.  With
    LIN_AT_INVOKE the history's invocation order is the witness and the
    search's first path, so "lin" is asserted with no exception."""
    c, m = tc.CLOSURES[name], tc.model(name)
    p = gen.table_params(n_clients=shape[0], n_ops=shape[1], prefix_ops=2, lin_policy=policy,
                         pid_mode=tc.PER_CLIENT, p_bug=0.0, seed=0xA11CE + shape[1],
                         inv_weight=c.get("weights"))
    n = 300
    hdr, ev, fl = gen.generate_table(p, m, 0, n)
    assert not np.any(fl & 1)
    if policy == tc.AT_INVOKE:
        # the state cannot move between a request and its execution: never stuck
        # (register and kv accept a response everywhere; lock's request avoids its raising pair)
        assert not np.any(fl)
    may_raise_first = m.post_err is not None and policy == tc.IN_WINDOW
    checked = dropped = raised_first = 0
    for i in np.flatnonzero(fl == 0):
        h = tc.history(m, hdr, ev, i)
        st, _, _ = oracle_linearisable(c["transition"], c["postcondition"], c["init"], h, PROMISE_MAX_NODES)
        if st == "error" and may_raise_first:
            raised_first += 1
            st, _, _ = oracle_linearisable(c["transition"], _never_raises(c["postcondition"]), c["init"], h,
                                           PROMISE_MAX_NODES)
        if st == "budget":
            dropped += 1
            continue
        assert st == "lin", (i, st)
        checked += 1
    assert (dropped + raised_first) * 20 <= n, (dropped, raised_first, checked)
    assert checked > n // 2


# ------------------------------------------------------------------ 4. bugs

def test_bug_rate_and_footprint():
    n, k, pre = 20000, 16, 4
    kw = dict(n_clients=4, n_ops=k, prefix_ops=pre, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT, seed=0xB06)
    m = tc.model("register")
    _, ev0, fl0 = gen.generate_table(gen.table_params(p_bug=0.0, **kw), m, 0, n)
    _, ev1, fl1 = gen.generate_table(gen.table_params(p_bug=0.5, **kw), m, 0, n)
    assert not np.any(fl0 & 1)
    share = np.count_nonzero(fl1 & 1) / n
    assert 0.48 <= share <= 0.52, share
    per = 2 * k
    e0, e1 = ev0.reshape(n, per), ev1.reshape(n, per)
    diff = e0.view(np.uint64) != e1.view(np.uint64)
    assert not np.any(diff[(fl1 & 1) == 0])                  # no bug: the p_bug = 0 twin
    assert not np.any(diff[:, :2 * pre])                     # never the prefix
    rows = np.flatnonzero(diff.any(axis=1))
    assert len(rows) > n // 4
    assert np.all(e0["kp"][diff] & 0x80) and np.array_equal(e0["kp"], e1["kp"])   # responses only,
    for f in ("a", "b", "val"):                                                   # and only their codes
        assert np.array_equal(e0[f], e1[f])
    assert int(diff.sum(axis=1).max()) <= 2
    # all prefix: no suffix response, no bug
    kw["prefix_ops"] = k
    _, _, fl = gen.generate_table(gen.table_params(p_bug=1.0, **kw), m, 0, 2000)
    assert not np.any(fl & 1)


# --------------------------------------------------------------- 5. weights

def _inv_counts(ev, n_inv):
    inv = ev[(ev["kp"] & 0x80) == 0]
    return np.bincount(inv["code"], minlength=n_inv)


def test_uniform_weights_are_uniform():
    m = tc.model("register")
    p = gen.table_params(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT,
                         seed=77)
    _, ev, _ = gen.generate_table(p, m, 0, 20000)
    cnt = _inv_counts(ev, 21)
    mean = cnt.sum() / 21
    assert cnt.sum() == 20000 * 16
    assert np.all(np.abs(cnt - mean) <= 0.05 * mean), cnt


def test_zero_weight_never_appears():
    m = tc.model("register")
    w = [1] * 21
    w[4] = w[20] = 0
    p = gen.table_params(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT,
                         seed=78, inv_weight=w)
    _, ev, _ = gen.generate_table(p, m, 0, 5000)
    cnt = _inv_counts(ev, 21)
    assert cnt[4] == 0 and cnt[20] == 0 and np.all(np.delete(cnt, [4, 20]) > 0)


def test_lock_weights_match_the_restatement():
    m = tc.model("lock")
    kw = dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT)
    _, ev, _ = gen.generate_table(gen.table_params(seed=79, inv_weight=(6, 1, 6), **kw), m, 0, 20000)
    share = _inv_counts(ev, 3) / (20000 * 16)
    _, ev_r, _ = ref.generate(m, 0, 3000, inv_weight=(6, 1, 6), seed=1079, **kw)
    share_r = _inv_counts(ev_r, 3) / (3000 * 16)
    assert np.all(np.abs(share - share_r) <= 0.05 * share_r), (share, share_r)


# ------------------------------------------------------------ 6. validation

def _call(p, model_struct, n=8, first=0, ev_base=0):
    lib = gen._load()
    per = 2 * max(int(p.n_ops), 1)
    hdr = np.full(n, 0xA5, dtype=np.uint8).repeat(16).view(codec.HDR_DTYPE)
    ev = np.full(n * min(per, 128) * 8, 0xA5, dtype=np.uint8).view(codec.EV_DTYPE)
    fl = np.full(n, 0xA5, dtype=np.uint8)
    rc = lib.qsmd_gen_table_batch(ctypes.byref(p), ctypes.addressof(model_struct) if model_struct else None,
                                  first, n, ev_base, hdr.ctypes.data, ev.ctypes.data, fl.ctypes.data, 2)
    untouched = all(np.all(x.view(np.uint8) == 0xA5) for x in (hdr, ev, fl))
    return rc, untouched


GOOD = dict(model_id=3, n_clients=4, n_ops=16, prefix_ops=4, lin_policy=1, pid_mode=0, p_bug=0.5, seed=1)
BAD = [("model_id", 2), ("model_id", 5), ("n_clients", 0), ("n_clients", 33), ("n_ops", 0), ("n_ops", 65),
       ("lin_policy", 2), ("pid_mode", 2), ("p_bug", float("nan")), ("p_bug", -0.01), ("p_bug", 1.01)]


def test_good_parameters_are_accepted():
    st = tc.model("register").c_struct()
    rc, untouched = _call(gen.table_params(**GOOD), st)
    assert rc == 0 and not untouched


@pytest.mark.parametrize("field,value", BAD)
def test_bad_parameter_is_rejected(field, value):
    st = tc.model("register").c_struct()
    rc, untouched = _call(gen.table_params(**dict(GOOD, **{field: value})), st)
    assert rc == -1 and untouched


def test_bad_weights_and_models_are_rejected():
    m = tc.model("register")
    st = m.c_struct()
    assert _call(gen.table_params(inv_weight=[0] * 21, **GOOD), st) == (-1, True)
    assert _call(gen.table_params(inv_weight=[1 << 31, 1 << 31] + [0] * 19, **GOOD), st) == (-1, True)
    assert _call(gen.table_params(inv_weight=[(1 << 32) - 1] + [0] * 20, **GOOD), st)[0] == 0
    assert _call(gen.table_params(**GOOD), None) == (-1, True)                    # no model
    assert _call(gen.table_params(**GOOD), st, ev_base=(1 << 32) - 100) == (-1, True)   # ev_off past u32
    # what qsmd_table_set rejects: a transition out of range, a missing table, init_state
    bad = m.c_struct()
    on_inv = m.on_inv.copy()
    on_inv[2, 3] = len(m.states)
    bad.on_inv = on_inv.ctypes.data
    assert _call(gen.table_params(**GOOD), bad) == (-1, True)
    bad = m.c_struct()
    bad.post = None
    assert _call(gen.table_params(**GOOD), bad) == (-1, True)
    bad = m.c_struct()
    bad.init_state = len(m.states)
    assert _call(gen.table_params(**GOOD), bad) == (-1, True)
    bad = m.c_struct()
    bad.n_inv = 33
    assert _call(gen.table_params(**GOOD), bad) == (-1, True)
    # the wide table's struct under model_id 4
    w = tc.model("kv")
    assert _call(gen.table_params(**dict(GOOD, model_id=4)), w.c_struct())[0] == 0
    bad = w.c_struct()
    bad.n_states = 65537
    assert _call(gen.table_params(**dict(GOOD, model_id=4)), bad) == (-1, True)


def test_python_binding_checks_the_weights_length():
    with pytest.raises(ValueError):
        gen.generate_table(gen.table_params(inv_weight=[1, 2], **GOOD), tc.model("register"), 0, 4)
    with pytest.raises(ValueError):
        gen.generate_table(gen.table_params(**dict(GOOD, n_clients=40)), tc.model("register"), 0, 4)


def test_qsmd_gen_batch_still_rejects_the_table_models():
    for mid in (3, 4):
        with pytest.raises(ValueError):
            gen.generate(gen.params(model_id=mid, n_clients=4, n_ops=16, prefix_ops=4), 0, 4)
