"""GPU parity of the three table searches (csrc/table.hip, csrc/wtable.hip,
csrc/ktable.hip) on histories of any shape (tests/anyshape.py): ill-formed
ones, several operations of one pid in flight, pending invocations, stray and
leading responses, in every width class, in both passes and under the state
memo.  These are the inputs on which the reference's four rules show --
takeInvocations stops at the first response, filter1 removes the pid's first
invocation (quirk Q1), findResponse => [] is no node, undo by Lemma L1 (and,
keyed, the one state byte of the chosen event's key).

The reference is the literal oracle (oracle/linearise_lists.py) on the models'
closures; for the memo's hit count, the literal mirrors of the kernels' steps
(tests/tablememo.py, tests/ktablememo.py).  No history is left out of a
comparison: the device runs with the oracle's max_nodes, and a `budget`
verdict must match too (nodes == max_nodes)."""

import functools
import random

import numpy as np
import pytest

import anyshape as an
import ktablememo as km
import tablegen as tg
import tablememo as tm
import wtablegen as wg
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device
from qsmd.linearisability import BudgetExceeded, linearisable, linearisable_batch
from qsmd.models import ModelError
from test_gpu_ktable import check, keyed, prod
from test_gpu_ktable import run_host as run_host5
from test_gpu_table import EXH, MAXN, assert_results, run_device, table
from test_gpu_table import run_host as run_host3
from test_gpu_wtable import run_host as run_host4

pytestmark = pytest.mark.gpu

# device model -> (model id, the closures its histories are generated and judged with)
MODELS = {"register": (3, "register"), "lock": (3, "lock"), "kv": (4, "kv"), "lock/wide": (4, "lock"),
          "register^4": (5, "register^4"), "lock^8": (5, "lock^8"), "register^8": (5, "register^8")}
KEYED = {"register^4": ("register", 4), "lock^8": ("lock", 8), "register^8": ("register", 8)}
PARITY = ["register", "lock", "kv", "lock/wide", "register^4", "lock^8"]
SETTINGS = list(an.ALL_SETTINGS)
BOTH_ENTRIES = ("6x16", "2x62")
RUN_HOST = {3: run_host3, 4: run_host4, 5: run_host5}
MEMO_KNOB = {3: "table_memo", 4: "table_memo", 5: "ktable_memo"}


@pytest.fixture(scope="module")
def ctx():
    """This module's own context (a keyed table, once set, cannot be taken
    away, and the session's context must stay without one: see
    test_gpu_ktable.py)."""
    c = device.Context(0, time_limit_ms=60000)
    yield c
    c.close()


def closures(name):
    if name in KEYED:
        return prod(*KEYED[name])
    return {"register": tg.REGISTER, "lock": tg.LOCK, "kv": wg.KV}[name]


def device_model(key):
    mid, name = MODELS[key]
    if mid == 3:
        return table(name)
    return wg.wide_table(name) if mid == 4 else keyed(*KEYED[key])


def oracle(name, hists):
    c = closures(name)
    return [oracle_linearisable(c["transition"], c["postcondition"], c["init"], h, MAXN) for h in hists]


@functools.lru_cache(maxsize=None)
def case(name, setting):
    """The histories of one setting for the closures `name` and the oracle's
    results (computed once, shared, never changed)."""
    hists = an.batch(closures(name), setting)
    return hists, oracle(name, hists)


@functools.lru_cache(maxsize=None)
def mirror_hits(name, setting, entries):
    """Per history of case(name, setting): the memo hits of the literal
    mirror of the kernel's step (0 for a search pass 2 can never take)."""
    hists, ref = case(name, setting)
    out = []
    for h, r in zip(hists, ref):
        info = {"hits": 0}
        if r[1] > 1:
            if name in KEYED:
                got = km.kmemo_dfs(*KEYED[name], h, entries, MAXN, info)
            else:
                got = tm.memo_dfs(closures(name), h, entries, MAXN, info)
            assert got == r
        out.append(info["hits"])
    return out


def set_model(ctx, key):
    mid, m = MODELS[key][0], device_model(key)
    if mid == 3 and ctx.table is not m:
        ctx.set_table(m)
    elif mid == 4 and ctx.wide_table is not m:
        ctx.set_wide_table(m)
    elif mid == 5 and ctx.keyed_table is not m:
        ctx.set_keyed_table(m)
    return mid, m


def run(ctx, key, hists):
    """The host entry: (batch, status, nodes, witness, totals)."""
    return RUN_HOST[MODELS[key][0]](ctx, device_model(key), hists)


def run_arrays(ctx, key, hdr, ev):
    """The host entry on arrays built by hand."""
    mid, _ = set_model(ctx, key)
    return ctx.check_arrays(mid, hdr, ev, None, EXH, MAXN, witness=True)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def pass2_expected(ref, budget):
    """The histories pass 2 takes (the formula of test_gpu_table.py's
    test_parity_with_the_oracle)."""
    if budget == 0:
        return []
    return [i for i, r in enumerate(ref) if r[1] > budget or (r[0] == "budget" and r[1] >= budget)]


class knobs:
    """Set table knobs; restore all of them on exit."""
    NAMES = ("table_budget", "table_memo", "ktable_memo", "table_memo_grid")

    def __init__(self, ctx, **params):
        self.ctx, self.params = ctx, params

    def __enter__(self):
        self.saved = {k: self.ctx.get_param(k) for k in self.NAMES}
        for k, v in self.params.items():
            self.ctx.set_param(k, v)
        return self.ctx

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.ctx.set_param(k, v)
        return False


# ------------------------------------------------------------ 1. parity matrix

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("key", PARITY)
def test_parity(ctx, key, setting):
    mid, name = MODELS[key]
    m = device_model(key)
    hists, ref = case(name, setting)
    default = ctx.get_param("table_budget")
    assert default == 256
    for budget in (default, 1, 0):
        with knobs(ctx, table_budget=budget):
            batch, st, nd, w, tot = run(ctx, key, hists)
            pass2 = ctx.table_pass2()
            assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)
            assert pass2 == len(pass2_expected(ref, budget))
            if setting in BOTH_ENTRIES:
                assert same((st, nd, w, tot), run_device(ctx, batch.hdr, batch.events, model_id=mid))
    assert not ctx.timed_out()
    if key == "lock^8":
        assert any(x[0] >= 4 for h in hists for _, (kind, x) in h if kind == "L")
    if key == "kv" and setting != an.RANDOM:     # state indices past one byte
        assert max(max(wg.state_indices_visited("kv", h), default=0) for h in hists) > 255


# ------------------------------------------------------------------ 2. memo on

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("key", PARITY)
def test_memo_on(ctx, key, setting):
    """Under the memo (2 entries: lossy; 1024) the results are still the
    oracle's.  The hits are the mirror's: a lane's gate map is reset per
    history and a hit compares the history index, so what other histories left
    in a lane slot never hits -- also with pass 2 on one workgroup
    ("table_memo_grid" 1), where every lane slot serves many histories."""
    mid, name = MODELS[key]
    m = device_model(key)
    hists, ref = case(name, setting)
    default = ctx.get_param("table_budget")
    for budget, grid in ((1, 0), (default, 0), (1, 1)):
        taken = pass2_expected(ref, budget)
        for entries in (2, 1024):
            with knobs(ctx, table_budget=budget, table_memo_grid=grid, **{MEMO_KNOB[mid]: entries}):
                batch, st, nd, w, tot = run(ctx, key, hists)
                hits, pass2 = ctx.table_memo_hits(), ctx.table_pass2()
                dev = run_device(ctx, batch.hdr, batch.events, model_id=mid) if setting in BOTH_ENTRIES else None
                hits_dev = ctx.table_memo_hits()
            assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)
            assert pass2 == len(taken)
            if dev is not None:
                assert same((st, nd, w, tot), dev) and hits_dev == hits
            print(key, setting, budget, grid, entries, "pass 2:", pass2, "hits:", hits)
            if mid != 4:        # (the wide step's slot hash has no mirror)
                per_history = mirror_hits(name, setting, entries)
                assert hits == sum(per_history[i] for i in taken), (budget, grid, entries)
            # the random family: few hits (lock^8's mirror counts none); at the default budget
            # pass 2 takes one of its histories or none
            if setting != an.RANDOM or (mid == 4 and budget == 1):
                assert hits > 0, (budget, grid, entries)
            elif not taken:
                assert hits == 0
    assert not ctx.timed_out()
    assert ctx.get_param("table_memo") == 0 and ctx.get_param("ktable_memo") == 0
    assert ctx.get_param("table_memo_grid") == 0 and ctx.get_param("table_budget") == default


@pytest.mark.parametrize("key", ["register", "kv", "lock^8"])
def test_one_history_many_times_in_a_lane_slot(ctx, key):
    """200 copies of one history through pass 2 on one workgroup: every lane
    slot meets the same (rem, state) keys again under another history index,
    in the same call.  What an earlier copy recorded must not hit, so the hits
    are 200 times those of the history alone."""
    mid, name = MODELS[key]
    m = device_model(key)
    hists, ref = case(name, "8x24")
    picked = [i for i, r in enumerate(ref) if 256 < r[1] < MAXN][:3]
    assert len(picked) == 3
    for i in picked:
        with knobs(ctx, **{MEMO_KNOB[mid]: 1024}):
            run(ctx, key, [hists[i]])
            alone = ctx.table_memo_hits()
        with knobs(ctx, table_memo_grid=1, **{MEMO_KNOB[mid]: 1024}):
            batch, st, nd, w, tot = run(ctx, key, [hists[i]] * 200)
            hits = ctx.table_memo_hits()
            assert ctx.table_pass2() == 200
        assert_results(m, [hists[i]] * 200, [ref[i]] * 200, st, nd, w, batch.hdr, None, tot)
        assert hits == 200 * alone > 0, i
        if mid != 4:
            assert alone == mirror_hits(name, "8x24", 1024)[i]


# ------------------------------------------------------------- 3. exact lengths

LENGTHS = [31, 32, 33, 63, 64, 65, 127, 128]


@functools.lru_cache(maxsize=None)
def length_case(name, n):
    """24 bent histories cut (or extended) to exactly n events: by turns 2
    clients on 2 pids with no wrong response (what is ill-formed there comes
    from the mutations and the cut; some stay linearisable at every length)
    and 3 clients on 2 pids."""
    rng = random.Random(f"anyshape/exactly/{name}/{n}")
    c = closures(name)
    hists = [an.exactly(an.bent(c, rng, 2 + k % 2, n // 2 + 4, 2, 0.02 * (k % 2)), n) for k in range(24)]
    assert all(len(h) == n for h in hists)
    return hists, oracle(name, hists)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("key", ["register", "register^8"])
def test_exact_lengths(ctx, key, n):
    mid, name = MODELS[key]
    m = device_model(key)
    hists, ref = length_case(name, n)
    assert {"lin", "nonlin"} <= {r[0] for r in ref}
    assert any(an.census(h) for h in hists)
    default = ctx.get_param("table_budget")
    for budget, entries in ((default, 0), (1, 0), (1, 16), (default, 16)):
        with knobs(ctx, table_budget=budget, **{MEMO_KNOB[mid]: entries}):
            batch, st, nd, w, tot = run(ctx, key, hists)
            assert_results(m, hists, ref, st, nd, w, batch.hdr, None, tot)
            assert same((st, nd, w, tot), run_device(ctx, batch.hdr, batch.events, model_id=mid))
    assert (batch.hdr["n_ev"] == n).all()


# ---------------------------------------------------------------- 4. pid planes

def relabelled(batch, seed):
    """The batch's events with every history's dense pids sent through an
    injection into 0..127 of its own."""
    ev = batch.events.copy()
    for i, h in enumerate(batch.hdr):
        o, n = int(h["ev_off"]), int(h["n_ev"])
        to = np.array(random.Random(f"{seed}/{i}").sample(range(128), max(int(h["n_pid"]), 1)), dtype=np.uint8)
        ev["kp"][o:o + n] = (ev["kp"][o:o + n] & 0x80) | to[ev["kp"][o:o + n] & 0x7F]
    return ev


@pytest.mark.parametrize("setting", BOTH_ENTRIES)
@pytest.mark.parametrize("key", ["register", "lock", "kv", "register^4", "lock^8"])
def test_pid_planes(ctx, key, setting):
    mid, name = MODELS[key]
    hists, ref = case(name, setting)
    batch, *plain = run(ctx, key, hists)
    assert_results(device_model(key), hists, ref, plain[0], plain[1], plain[2], batch.hdr, None, plain[3])
    ev = relabelled(batch, f"anyshape/planes/{key}/{setting}")
    for b in range(7):      # a history in which the plane tells pids apart
        assert any(len({(int(kp) >> b) & 1 for kp in ev["kp"][int(h["ev_off"]):int(h["ev_off"]) + int(h["n_ev"])]})
                   == 2 for h in batch.hdr), b
    assert int((ev["kp"] & 0x7F).max()) > 100
    # the event indices do not change: the very same arrays
    assert same(plain, run_arrays(ctx, key, batch.hdr, ev))
    assert same(plain, run_device(ctx, batch.hdr, ev, model_id=mid))
    with knobs(ctx, table_budget=1, **{MEMO_KNOB[mid]: 16}):
        assert same(plain, run_arrays(ctx, key, batch.hdr, ev))


# ------------------------------------------------------------ 5. key permutation

@pytest.mark.parametrize("setting", ["6x16", "8x24", an.RANDOM])
@pytest.mark.parametrize("key", ["register^4", "lock^8"])
def test_key_permutation(ctx, key, setting):
    """Every key starts in the same state, so renaming the keys changes
    nothing; a response's `a` is ignored."""
    comp, K = KEYED[key]
    hists, ref = case(MODELS[key][1], setting)
    check(ctx, comp, K, hists, ref=ref)
    batch, *plain = run(ctx, key, hists)
    perm, rng = list(range(K)), random.Random(f"anyshape/keys/{key}")
    while any(perm[k] == k for k in range(K)):      # (no key keeps its name)
        rng.shuffle(perm)
    ev = batch.events.copy()
    resp = (ev["kp"] & 0x80) != 0
    assert set(ev["a"][~resp].tolist()) == set(range(K)) and not ev["a"][resp].any()
    ev["a"] = np.where(resp, 0xFF, np.array(perm, dtype=np.uint8)[ev["a"]])
    for budget, entries in ((256, 0), (1, 0), (1, 16)):
        with knobs(ctx, table_budget=budget, ktable_memo=entries):
            assert same(plain, run_arrays(ctx, key, batch.hdr, ev)), (budget, entries)


# -------------------------------------------------------------------- 6. offsets

@pytest.mark.parametrize("key", ["register", "lock/wide", "kv", "register^4", "lock^8"])
def test_offsets(ctx, key):
    """1..7 junk events before the first history and between histories."""
    mid, name = MODELS[key]
    hists = case(name, "6x16")[0][:200] + case(name, "2x62")[0][:30]
    batch, *plain = run(ctx, key, hists)
    rng = random.Random(f"anyshape/offsets/{key}")
    gaps = [rng.randint(1, 7) for _ in hists]
    assert set(gaps) == set(range(1, 8))
    hdr = batch.hdr.copy()
    hdr["ev_off"] = batch.hdr["ev_off"] + np.cumsum(gaps)
    ev = np.zeros(len(batch.events) + sum(gaps), dtype=codec.EV_DTYPE)
    ev.view(np.uint8)[:] = np.frombuffer(rng.randbytes(ev.nbytes), dtype=np.uint8)     # junk everywhere ...
    inside = np.zeros(len(ev), dtype=bool)
    for h0, h1 in zip(batch.hdr, hdr):
        n = int(h0["n_ev"])
        ev[int(h1["ev_off"]):int(h1["ev_off"]) + n] = batch.events[int(h0["ev_off"]):int(h0["ev_off"]) + n]
        inside[int(h1["ev_off"]):int(h1["ev_off"]) + n] = True                          # ... but in the histories
    assert int(hdr["ev_off"][0]) == gaps[0] and not inside[:gaps[0]].any()
    for entry in ("host", "device"):
        st, nd, w, tot = run_arrays(ctx, key, hdr, ev) if entry == "host" else run_device(ctx, hdr, ev, model_id=mid)
        assert np.array_equal(st, plain[0]) and np.array_equal(nd, plain[1]) and tot == plain[3]
        assert np.array_equal(w[inside], plain[2])
        assert (w[~inside] == 0xFF).all()           # as it was given
    assert {0, 1} <= set(plain[0].tolist())


# ------------------------------------------------------------------- 7. drop-in

@pytest.mark.parametrize("key", ["lock", "kv", "lock^8"])
def test_drop_in_call(ctx, key):
    name = MODELS[key][1]
    m = device_model(key)
    hists, ref = [], []
    for setting in SETTINGS:
        hists += case(name, setting)[0][:8]
        ref += case(name, setting)[1][:8]
    assert len(hists) == 40
    for h, (st, _, _) in zip(hists, ref):
        call = functools.partial(linearisable, m.transition, m.postcondition, None, h, ctx=ctx, max_nodes=MAXN)
        if st == "error":
            with pytest.raises(ModelError):
                call()
        elif st == "budget":
            with pytest.raises(BudgetExceeded):
                call()
        else:
            assert call() == (st == "lin")
    res = linearisable_batch(m, hists, max_nodes=MAXN, witness=True, ctx=ctx)
    assert_results(m, hists, ref, res.status, res.nodes, res.witness, res.batch.hdr, None, res.totals)
    assert {"lin", "nonlin"} <= {r[0] for r in ref}
