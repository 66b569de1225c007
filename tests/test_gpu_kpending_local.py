"""GPU parity of the keyed pending call's local mode (csrc/ksplit.hip's pending
form, knob "kpending_local"): status, node count and totals of every history
against the literal restatement (tests/kpendinglocal_ref.py: the split, the
pending rule of tests/pending_ref.py with the component's closures on every
key's part, the combine rule); the histories the restatement does not split
against a knob-0 call on the same batch; "kpending_local_last" against the
restatement's count of splittable histories (an empty history is splittable:
into no part, as for "ktable_local").  No history is left out: the device runs
with the restatement's max_nodes, and a `budget` must match too.  Through the
host and the device entry, at `table_budget` default, 0 and 4."""

import functools
import random

import numpy as np
import pytest

import kpendinglocal_ref as klr
import ktablelocal_ref as lref
import pending_ref as pr
import tablegen as tg
from qsmd import codec, device
from qsmd.linearisability import linearisable, linearisable_batch
from qsmd.models import KeyedTableModel, ModelError
from test_gpu_ktable import COMPONENTS, component, keyed, prod
from test_gpu_table_pending import budget_knob
from test_kpending_local_host import KAT_RULE2, KATS, Rd, Val, W

pytestmark = pytest.mark.gpu

L, R = tg.L, tg.R
EXH = device.QSMD_FLAG_EXHAUSTIVE
MAXN = tg.MAX_NODES
CODE = {"lin": 1, "nonlin": 0, "error": 2, "encode": 3, "budget": 4}
BUDGETS = (256, 0, 4)
CRASH = 0.3


@pytest.fixture(scope="module")
def ctx():
    """This module's own context (a keyed table, once set, cannot be taken
    away: see test_gpu_ktable.py)."""
    c = device.Context(0, time_limit_ms=60000)
    assert c.get_param("table_budget") == BUDGETS[0]
    yield c
    c.close()


def model_of(name, K):
    """The keyed model of a COMPONENTS name and K; a KeyedTableModel given as
    ``name`` is itself (K is then not looked at: the raw-table modules pass
    their own models, and the restatement's closures as ``closures=``)."""
    return name if isinstance(name, KeyedTableModel) else keyed(name, K)


def encode(name, K, hists, model0=None):
    batch = codec.encode(model_of(name, K), [list(h) for h in hists], model0)
    assert not batch.encode_errors
    return batch.hdr, batch.events


class knobs:
    """Context knobs set for a block and put back to 0."""

    def __init__(self, ctx, **values):
        self.ctx, self.values = ctx, values

    def __enter__(self):
        for k, v in self.values.items():
            self.ctx.set_param(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.ctx.set_param(k, 0)
        return False


def set_table(ctx, name, K):
    m = model_of(name, K)
    if ctx.keyed_table is not m:
        ctx.set_keyed_table(m)
    return m


def run_host(ctx, name, K, hdr, ev, local, max_nodes=MAXN, model0=None, witness=False):
    """(status, nodes, witness, assumed, totals, kpending_local_last)"""
    m = set_table(ctx, name, K)
    with knobs(ctx, kpending_local=local):
        out = ctx.check_kpending_arrays(hdr, ev, m.pack_model0(model0, {}), EXH, max_nodes, witness=witness)
        return out + (ctx.kpending_local_last(),)


class DeviceCall:
    """One qsmd_check_kpending_batch_device call on a stream, its buffers kept
    until read()."""

    def __init__(self, ctx, name, K, hdr, ev, local, stream, max_nodes=MAXN, model0=None, witness=False):
        import torch
        m = set_table(ctx, name, K)
        dev = torch.device("cuda:0")
        self.n, self.n_ev, self.torch, self.witness = len(hdr), len(ev), torch, witness
        with torch.cuda.stream(stream):
            self.hdr = torch.from_numpy(hdr.view(np.uint8).copy()).to(dev) if len(hdr) else \
                torch.zeros(16, dtype=torch.uint8, device=dev)
            self.ev = torch.from_numpy(ev.view(np.uint8).copy()).to(dev) if len(ev) else \
                torch.zeros(8, dtype=torch.uint8, device=dev)
            self.st = torch.full((max(self.n, 1),), 0xEE, dtype=torch.uint8, device=dev)
            self.nd = torch.full((max(self.n, 1),), -1, dtype=torch.int64, device=dev)
            self.tot = torch.full((8,), -1, dtype=torch.int64, device=dev)
            self.w = torch.full((max(self.n_ev, 1),), 0xFF, dtype=torch.uint8, device=dev)
            self.a = torch.full((max(self.n_ev, 1),), 0xFF, dtype=torch.uint8, device=dev)
        with knobs(ctx, kpending_local=local):
            ctx.check_kpending_device(self.hdr.data_ptr(), self.n, self.ev.data_ptr(), self.n_ev, self.st.data_ptr(),
                                      self.nd.data_ptr(), self.w.data_ptr() if witness else None,
                                      self.tot.data_ptr(), model0=m.pack_model0(model0, {}),
                                      flags=EXH | (device.QSMD_FLAG_WITNESS if witness else 0),
                                      max_nodes=max_nodes, stream=stream.cuda_stream,
                                      assumed_ptr=self.a.data_ptr() if witness else None)

    def read(self):
        self.torch.cuda.synchronize()
        tot = dict(zip((n for n, _ in device.Totals._fields_), (int(x) for x in self.tot.cpu().numpy())))
        return (self.st.cpu().numpy()[:self.n], self.nd.cpu().numpy().astype(np.uint64)[:self.n],
                self.w.cpu().numpy()[:self.n_ev], self.a.cpu().numpy()[:self.n_ev], tot)


def run_device(ctx, name, K, hdr, ev, local, **kw):
    torch = pytest.importorskip("torch")
    call = DeviceCall(ctx, name, K, hdr, ev, local, torch.cuda.Stream(), **kw)
    return call.read() + (ctx.kpending_local_last(),)


def expected(ctx, name, K, hdr, ev, max_nodes=MAXN, model0=None, closures=None):
    """[(status code, nodes)] per header and the number of split histories:
    the restatement's result, and for a history it does not split the knob-0
    call's (at the default `table_budget`: the product route's results do not
    depend on it).  ``closures``: the component's, when ``name`` is a model."""
    want = klr.check_arrays(closures or COMPONENTS[name], model_of(name, K).n_keys, hdr, ev, max_nodes, model0)
    n_split = sum(w is not None for w in want)
    if n_split < len(want):
        st0, nd0, _, _, _, split0 = run_host(ctx, name, K, hdr, ev, 0, max_nodes, model0)
        assert split0 == 0
    return [(CODE[w[0]], w[1]) if w is not None else (int(st0[i]), int(nd0[i])) for i, w in enumerate(want)], n_split


def assert_equal(want, n_split, st, nd, tot, split, max_nodes=MAXN):
    got = [(int(s), int(n)) for s, n in zip(st, nd)]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad and len(got) == len(want), bad[:5]
    count = lambda c: sum(1 for s, _ in want if s == c)     # noqa: E731
    assert tot == dict(checked=count(0) + count(1) + count(2), linearisable=count(1), nonlinearisable=count(0),
                       model_errors=count(2), encode_errors=count(3), budget=count(4), skipped=0,
                       nodes=sum(n for _, n in want))
    assert split == n_split


def check_local(ctx, name, K, hdr, ev, max_nodes=MAXN, model0=None, budgets=BUDGETS, want=None, closures=None):
    """Knob 1 through the host and the device entry, at every budget, against
    the expectation."""
    want, n_split = want or expected(ctx, name, K, hdr, ev, max_nodes, model0, closures)
    for budget in budgets:
        with budget_knob(ctx, budget):
            st, nd, w, asm, tot, split = run_host(ctx, name, K, hdr, ev, 1, max_nodes, model0)
            assert w is None and asm is None
            assert_equal(want, n_split, st, nd, tot, split)
            st, nd, _, _, tot, split = run_device(ctx, name, K, hdr, ev, 1, max_nodes=max_nodes, model0=model0)
            assert_equal(want, n_split, st, nd, tot, split)
    return want, n_split


@functools.lru_cache(maxsize=None)
def crashed(name, K, setting, n, p_crash=CRASH):
    p = prod(name, K)
    rng = random.Random(f"kpending-local/{name}/{K}/{setting}")
    return tuple(tuple(pr.crash(h, rng, p_crash)) for h in tg.gen_batch(p, setting, n))


# ------------------------------------------------------------------ 1. KATs

def test_kats(ctx):
    for K in (4, 8):
        kats = [(h, st, nd) for h, k, st, nd in KATS if k == K]
        hdr, ev = encode("register", K, [h for h, _, _ in kats])
        want, n_split = check_local(ctx, "register", K, hdr, ev)
        assert want == [(CODE[st], nd) for _, st, nd in kats] and n_split == len(kats)
    hdr, ev = encode("lock", 4, [KAT_RULE2, KAT_RULE2[:1]])
    assert check_local(ctx, "lock", 4, hdr, ev)[0] == [(CODE["nonlin"], 1), (CODE["lin"], 0)]
    # the drop-in
    m = keyed("register", 4)
    h, _, st, nd = KATS[1]
    assert not linearisable(m.transition, m.postcondition, None, h, ctx=ctx, pending="complete", kpending_local=True)
    assert ctx.kpending_local_last() == 1 and ctx.get_param("kpending_local") == 0
    res = linearisable_batch(m, [h], ctx=ctx, pending="complete", kpending_local=True)
    assert (res.verdict(0), int(res.nodes[0])) == (st, nd) == ("nonlin", 2)
    res = linearisable_batch(m, [h], ctx=ctx, pending="complete")
    assert (res.verdict(0), int(res.nodes[0])) == ("nonlin", 3) and ctx.kpending_local_last() == 0


# ---------------------------------------------------------- 2. crashed batches

CRASH_BATCHES = [("register", 4, "3x10", 300, {"lin", "nonlin"}),
                 ("register", 4, "4x16", 300, {"lin", "nonlin"}),
                 ("register", 8, "6x24", 60, {"lin", "nonlin"}),
                 ("lock", 8, "4x16", 300, {"lin", "nonlin", "error"}),
                 ("counter", 2, "4x16", 200, {"lin", "nonlin"})]


@pytest.mark.parametrize("name,K,setting,n,statuses", CRASH_BATCHES)
def test_crashed_batches(ctx, name, K, setting, n, statuses):
    hists = crashed(name, K, setting, n)
    assert sum(1 for h in hists if pr.pending_invocations(list(h))) > n // 3
    hdr, ev = encode(name, K, hists)
    want, n_split = check_local(ctx, name, K, hdr, ev)
    assert not ctx.timed_out()
    assert n_split == n and statuses <= {s for s in CODE if CODE[s] in {c for c, _ in want}}
    # the restatement on the arrays is the restatement on the histories
    assert want == [(CODE[s], nd) for s, nd in (klr.check(COMPONENTS[name], K, list(h), MAXN) for h in hists)]
    # several parts per history, and parts without a response
    parts = [klr.split(COMPONENTS[name], K, list(h)) for h in hists]
    assert sum(1 for p in parts if len(p) > 1) > n // 2
    assert any(all(e[1][0] == "L" for e in sub) for p in parts for _, sub in p)
    st0, nd0, _, _, tot0, split0 = run_host(ctx, name, K, hdr, ev, 0)
    assert split0 == 0
    if name == "register":
        # verdicts are the product's wherever the product decides
        assert all(int(s) == w[0] for s, w in zip(st0, want) if int(s) != CODE["budget"])
    if (name, K) == ("register", 8):
        decided = sum(1 for s, w in zip(st0, want) if int(s) == CODE["budget"] and w[0] in (0, 1))
        assert decided >= 1 and tot0["budget"] >= decided
        assert any(x[0] >= 4 for h in hists for _, (kind, x) in h if kind == "L")
    if name == "counter":                   # the largest table: 80 KB, with post_err
        c = component("counter")
        assert c.post_err is not None and len(c.states) == 256


# --------------------------------------------------------- 3. complete batches

@pytest.mark.parametrize("name,K", [("register", 4), ("lock", 8)])
def test_complete_batches_equal_the_local_check_call(ctx, name, K):
    hists = tg.gen_batch(prod(name, K), "4x16", 300)
    assert not any(pr.pending_invocations(h) for h in hists)
    hdr, ev = encode(name, K, hists)
    m = set_table(ctx, name, K)
    for budget in BUDGETS:
        with budget_knob(ctx, budget):
            with knobs(ctx, ktable_local=1):
                st0, nd0, _, tot0 = ctx.check_arrays(5, hdr, ev, None, EXH, MAXN)
                split0 = ctx.ktable_local_last()
            st, nd, _, _, tot, split = run_host(ctx, name, K, hdr, ev, 1)
            assert np.array_equal(st, st0) and np.array_equal(nd, nd0) and tot == tot0 and split == split0 == 300
            std, ndd, _, _, totd, splitd = run_device(ctx, name, K, hdr, ev, 1)
            assert np.array_equal(std, st0) and np.array_equal(ndd, nd0) and totd == tot0 and splitd == 300
    assert {0, 1} <= set(st.tolist())
    assert [(int(s), int(x)) for s, x in zip(st, nd)] == [
        (CODE[r[0]], r[1]) for r in (lref.check(COMPONENTS[name], K, h, MAXN) for h in hists)]
    assert m is ctx.keyed_table


# ------------------------------------------------------------------ 4. fallbacks

def fallback_batch():
    """(hdr, events, the rows that must take the product route) of a batch of
    splittable crashed histories with every kind of fallback mixed in."""
    name, K = "register", 4
    good = [list(h) for h in crashed(name, K, "4x16", 300)[:80]]
    ok = lambda p: (p, R("Ok"))                         # noqa: E731
    lone = good[4][:1] + [ok(9)] + good[4][1:]          # a lone response (after the first invocation)
    in_flight = [(0, W(1, 1)), (0, W(2, 2)), ok(0), ok(0), (1, W(1, 1)), ok(1)]     # two operations of one pid
    after_pending = good[5] + [(9, W(0, 1)), (9, Rd(0))]                    # an invocation after a pending one
    hists = good[:6] + [lone, in_flight, after_pending] + good[6:70]
    tail = [good[70 + i] for i in range(5)]
    assert all(len(h) > 2 for h in tail)
    hists += tail + [[]]
    hdr, ev = encode(name, K, hists)
    hdr, ev = hdr.copy(), ev.copy()
    n = len(hists)

    def first(i, resp):
        o = int(hdr[i]["ev_off"])
        return o + next(k for k in range(int(hdr[i]["n_ev"])) if bool(ev["kp"][o + k] & 0x80) == resp)

    ev["a"][first(n - 6, False)] = K                    # a key >= n_keys
    ev["code"][first(n - 5, False)] = len(tg.REG_INVS)  # an invocation code >= n_inv
    ev["code"][first(n - 4, True)] = len(tg.REG_RESPS)  # a response code >= n_resp
    hdr["model_id"][n - 3] = 3                          # a wrong model id
    hdr["n_ev"][n - 2] += 1                             # a slot past n_events (the last non-empty one)
    assert int(hdr[n - 2]["ev_off"]) + int(hdr[n - 2]["n_ev"]) == len(ev) + 1 and hdr[n - 1]["n_ev"] == 0
    return hdr, ev, [6, 7, 8, n - 6, n - 5, n - 4, n - 3, n - 2]


def test_fallbacks_in_a_mixed_batch(ctx):
    hdr, ev, fallback = fallback_batch()
    n = len(hdr)
    want, n_split = expected(ctx, "register", 4, hdr, ev)
    assert n_split == n - len(fallback)                 # (the empty history is split: into no part)
    assert [want[i][0] for i in fallback[3:]] == [CODE["encode"]] * 5 and want[n - 1] == (1, 0)
    assert all(want[i][1] > 0 for i in fallback[:3])    # searched (on the product), not refused
    check_local(ctx, "register", 4, hdr, ev, want=(want, n_split))
    # the fallback rows are the knob-0 call's, bit for bit, at every budget
    for budget in BUDGETS:
        with budget_knob(ctx, budget):
            st0, nd0, _, _, _, _ = run_host(ctx, "register", 4, hdr, ev, 0)
            st1, nd1, _, _, _, _ = run_host(ctx, "register", 4, hdr, ev, 1)
            assert [(int(st0[i]), int(nd0[i])) for i in fallback] == [(int(st1[i]), int(nd1[i])) for i in fallback]


def test_every_fallback_alone(ctx):
    hdr, ev, fallback = fallback_batch()
    n = len(hdr)
    for i in fallback + [n - 1]:
        h1 = hdr[i:i + 1].copy()
        n_events = len(ev)
        if i == n - 2:                                  # the slot past n_events: one event short
            n_events = int(h1[0]["ev_off"]) + int(h1[0]["n_ev"]) - 1
        e1 = ev[:n_events]
        a = run_host(ctx, "register", 4, h1, e1, 0)
        b = run_host(ctx, "register", 4, h1, e1, 1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[4] == b[4], i
        assert (a[5], b[5]) == (0, 1 if i == n - 1 else 0), i
        d = run_device(ctx, "register", 4, h1, e1, 1)
        assert np.array_equal(a[0], d[0]) and np.array_equal(a[1], d[1]) and a[4] == d[4] and d[5] == b[5], i


# ---------------------------------------------------------------- 5. witness call

def test_a_witness_call_takes_the_product_route(ctx):
    hists = crashed("register", 4, "4x16", 300)[:100]
    hdr, ev = encode("register", 4, hists)
    a = run_host(ctx, "register", 4, hdr, ev, 0, witness=True)
    b = run_host(ctx, "register", 4, hdr, ev, 1, witness=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    assert a[5] == b[5] == 0
    assert np.any(a[3] != device.QSMD_ASSUMED_NONE)     # `assumed` included
    d0 = run_device(ctx, "register", 4, hdr, ev, 0, witness=True)
    d1 = run_device(ctx, "register", 4, hdr, ev, 1, witness=True)
    assert all(np.array_equal(x, y) for x, y in zip(d0[:4], d1[:4])) and d0[4] == d1[4] and d1[5] == 0
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], d1[:4]))
    local = run_host(ctx, "register", 4, hdr, ev, 1)
    assert local[5] == 100 and not np.array_equal(local[1], a[1])


# ------------------------------------------------------------ 6. split kernel edges

def long_history(K, keys, clients, n_ops, seed, p_bug=0.0):
    """n_ops complete operations on the keys `keys` of register^K."""
    p = dict(prod("register", K))
    p["invs"] = [(k, i) for k in keys for i in tg.REG_INVS]
    return tg.gen_history(p, random.Random(f"kpending-local/long/{K}/{keys}/{seed}"), clients, n_ops, p_bug)


def edge_histories():
    all8 = tuple(range(8))
    out = {}
    g = lambda n_ops, s, keys=all8: long_history(8, keys, 6, n_ops, s)      # noqa: E731  (pids 0..5)
    out["64 exactly"] = g(31, 1)[:40] + [(10, W(3, 1))] + g(31, 1)[40:] + [(11, Rd(3))]
    out["65, a one-event pid in the second round"] = g(32, 2) + [(10, W(7, 2))]
    out["127"] = g(63, 3) + [(10, Rd(0))]
    out["128, a pending invocation as event 127"] = g(63, 4)[:70] + [(10, W(5, 3))] + g(63, 4)[70:] + [(11, Rd(5))]
    for v in range(4):
        # pid 7 pending at 62; pid 8: invocation at 63, response at 64, then pending in the second round
        out[f"straddle {v}"] = g(31, 5) + [(7, W(2, 1)), (8, Rd(6)), (8, Val(v)), (9, Rd(2)), (8, W(6, 2))]
    h = g(60, 6)
    last = {pid: kind for pid, (kind, _) in h}
    first_round = {pid for pid, _ in h[:64]}
    assert all(k == "R" for k in last.values()) and first_round == set(range(6))
    out["every pid ends pending in the second round"] = h + [(pid, W(pid, 1)) for pid in range(6)]
    out["all events on the highest key"] = g(40, 7, (7,))[:-3] + [(10, L((7, "Read")))]
    out["all events on the highest key, 128"] = g(63, 8, (7,)) + [(10, W(7, 1)), (11, Rd(7))]
    return out


def test_split_kernel_edges(ctx):
    edges = edge_histories()
    assert len(edges["64 exactly"]) == 64 and len(edges["127"]) == 127
    assert len(edges["65, a one-event pid in the second round"]) == 65
    h128 = edges["128, a pending invocation as event 127"]
    assert len(h128) == 128 and h128[127][1][0] == "L"
    s = edges["straddle 0"]
    assert s[63] == (8, Rd(6)) and s[64][0] == 8 and s[64][1][0] == "R" and s[-1] == (8, W(6, 2)) and len(s) == 67
    assert len(edges["all events on the highest key, 128"]) == 128
    hists = list(edges.values())
    # random crashed long histories beside them: 33..128 events
    rng = random.Random("kpending-local/edges")
    for s in range(60):
        h = pr.crash(long_history(8, tuple(range(8)), 6, 40 + (s % 25), 100 + s, p_bug=0.02 * (s % 2)), rng, 0.5)
        hists.append(h)
    assert sum(1 for h in hists if len(h) > 64) > 30 and all(len(h) <= 128 for h in hists)
    hdr, ev = encode("register", 8, hists)
    want, n_split = check_local(ctx, "register", 8, hdr, ev)
    assert n_split == len(hists) and {0, 1} <= {c for c, _ in want}
    # all 8 keys present; parts in a narrower width class than their history
    parts = klr.split_arrays(hdr[3], ev, len(ev), 8, len(tg.REG_INVS), len(tg.REG_RESPS))
    assert [k for k, _ in parts] == list(range(8)) and max(len(idx) for _, idx in parts) <= 32
    parts = klr.split_arrays(hdr[len(edges) - 1], ev, len(ev), 8, len(tg.REG_INVS), len(tg.REG_RESPS))
    assert [(k, len(idx)) for k, idx in parts] == [(7, 128)]
    # one key of one: the part is the whole history, pending invocations and all
    h1 = [long_history(1, (0,), 4, 63, s) + [(10, W(0, 1)), (11, Rd(0))] for s in range(4)]
    h1 += [long_history(1, (0,), 4, 31, s) + [(10, W(0, 1)), (11, Rd(0))] for s in range(4)]
    hdr1, ev1 = encode("register", 1, h1)
    want1, _ = check_local(ctx, "register", 1, hdr1, ev1, budgets=(256, 0))
    st0, nd0, _, _, _, _ = run_host(ctx, "register", 1, hdr1, ev1, 0)
    assert want1 == [(int(s), int(x)) for s, x in zip(st0, nd0)]


@pytest.mark.parametrize("n_hist", [1, 63, 64, 65, 129])
def test_batch_sizes(ctx, n_hist):
    hists = crashed("register", 4, "4x16", 300)[:n_hist]
    check_local(ctx, "register", 4, *encode("register", 4, hists), budgets=(256,))


# ------------------------------------------------------------------ 7. model0

def test_model0_per_key(ctx):
    start = (3, 0, 2, 1)
    p = dict(prod("register", 4), init=start)
    rng = random.Random("kpending-local/model0")
    hists = [pr.crash(tg.gen_history(p, rng, 3, 10, 0.05), rng, CRASH) for _ in range(200)]
    hists += [[(0, W(1, 3)), (1, Rd(2)), (1, Val(2))], [(0, W(1, 3)), (1, Rd(2)), (1, Val(0))]]
    hdr, ev = encode("register", 4, hists, model0=start)
    want, _ = check_local(ctx, "register", 4, hdr, ev, model0=start)
    assert want[-2:] == [(1, 2), (0, 2)]
    plain = klr.check_arrays(tg.REGISTER, 4, hdr, ev, MAXN)
    assert sum(1 for w, q in zip(want, plain) if w[0] == 1 and q[0] != "lin") > 50


# ------------------------------------------------------------ 8. independence

def test_the_check_calls_knob_does_not_reach_this_call(ctx):
    hists = crashed("register", 4, "4x16", 300)[:100]
    hdr, ev = encode("register", 4, hists)
    plain = run_host(ctx, "register", 4, hdr, ev, 0)
    with knobs(ctx, ktable_local=1):
        got = run_host(ctx, "register", 4, hdr, ev, 0)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]) and plain[4] == got[4]
    assert got[5] == 0


def test_this_knob_does_not_reach_the_check_call(ctx):
    m = set_table(ctx, "register", 4)
    complete = encode("register", 4, tg.gen_batch(prod("register", 4), "4x16", 100))
    crashed_ = encode("register", 4, crashed("register", 4, "4x16", 300)[:70])
    results = {}
    for klocal in (0, 1):
        with knobs(ctx, ktable_local=klocal):
            a = ctx.check_arrays(5, *complete, None, EXH, MAXN)
            last = ctx.ktable_local_last()
            with knobs(ctx, kpending_local=1):
                b = ctx.check_arrays(5, *complete, None, EXH, MAXN)
                assert ctx.ktable_local_last() == last == 100 * klocal
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
            results[klocal] = a
            # a local pending call in between moves its own counter only
            assert run_host(ctx, "register", 4, *crashed_, 1)[5] == 70
            assert ctx.ktable_local_last() == last
            ctx.check_arrays(5, *complete, None, EXH, MAXN)
            assert ctx.kpending_local_last() == 70 and ctx.ktable_local_last() == last
    assert not np.array_equal(results[0][1], results[1][1]) and m is ctx.keyed_table


def test_check_calls_and_pending_calls_alternate_on_one_workspace():
    hists = crashed("register", 4, "4x16", 300)
    complete = tg.gen_batch(prod("register", 4), "4x16", 300)
    c = device.Context(0, time_limit_ms=60000)
    try:
        set_table(c, "register", 4)
        for pending, n in ((True, 64), (False, 300), (True, 300), (False, 10), (True, 10), (True, 129),
                           (False, 129), (True, 1), (False, 300), (True, 200)):
            if pending:
                check_local(c, "register", 4, *encode("register", 4, hists[:n]), budgets=(256,))
            else:
                hdr, ev = encode("register", 4, complete[:n])
                with knobs(c, ktable_local=1):
                    st, nd, _, _ = c.check_arrays(5, hdr, ev, None, EXH, MAXN)
                    assert c.ktable_local_last() == n
                assert [(int(s), int(x)) for s, x in zip(st, nd)] == [
                    (CODE[r[0]], r[1]) for r in (lref.check(tg.REGISTER, 4, h, MAXN) for h in complete[:n])]
    finally:
        c.close()


def test_the_memo_knobs_are_inert(ctx):
    hists = crashed("register", 8, "6x24", 60)
    hdr, ev = encode("register", 8, hists)
    plain = run_host(ctx, "register", 8, hdr, ev, 1)
    with knobs(ctx, ktable_memo=64, table_memo=64, pending_memo=64):
        for budget in (256, 4):
            with budget_knob(ctx, budget):
                got = run_host(ctx, "register", 8, hdr, ev, 1)
                assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]) and plain[4:] == got[4:]
                dev = run_device(ctx, "register", 8, hdr, ev, 1)
                assert np.array_equal(plain[0], dev[0]) and np.array_equal(plain[1], dev[1]) and plain[4:] == dev[4:]
    assert plain[5] == 60


# ------------------------------------------------------------------ 9. refusals

def test_refusals(ctx):
    m = set_table(ctx, "register", 4)
    assert ctx.get_param("kpending_local") == 0
    ctx.set_param("kpending_local", 1)
    try:
        for bad in (2, 3, 1 << 40):
            with pytest.raises(device.DeviceError) as e:
                ctx.set_param("kpending_local", bad)
            assert int(str(e.value).split("failed (")[1].split(")")[0]) == -1
            assert ctx.get_param("kpending_local") == 1
    finally:
        ctx.set_param("kpending_local", 0)
    h = KATS[1][0]
    reg = component("register")
    with pytest.raises(ValueError):
        linearisable_batch(reg, [[(0, L(("Write", 1)))]], ctx=ctx, pending="complete", kpending_local=True)
    with pytest.raises(ValueError):
        linearisable_batch(m, [h], ctx=ctx, kpending_local=True)
    with pytest.raises(ValueError):
        linearisable(m.transition, m.postcondition, None, h, ctx=ctx, kpending_local=False)
    assert ctx.get_param("kpending_local") == 0
    # ktable_local= keeps its meaning and stays inert for a pending call
    res = linearisable_batch(m, [h], ctx=ctx, pending="complete", ktable_local=True)
    assert (res.verdict(0), int(res.nodes[0])) == ("nonlin", 3) and ctx.kpending_local_last() == 0
    # the context serves a call afterwards
    hdr, ev = encode("register", 4, [h, KATS[0][0]])
    st, nd, _, _, _, split = run_host(ctx, "register", 4, hdr, ev, 1)
    assert [(int(s), int(x)) for s, x in zip(st, nd)] == [(0, 2), (1, 2)] and split == 2


# ------------------------------------------------------ 10. the Python entries

def test_through_linearisable_batch_and_linearisable(ctx):
    m = keyed("lock", 4)
    hists = [list(h) for h in crashed("lock", 4, "4x16", 300)[:60]]
    want = [klr.check(tg.LOCK, 4, h, MAXN) for h in hists]
    res = linearisable_batch(m, hists, max_nodes=MAXN, ctx=ctx, pending="complete", kpending_local=True)
    assert [(res.verdict(i), int(res.nodes[i])) for i in range(60)] == want
    assert ctx.kpending_local_last() == 60 and ctx.get_param("kpending_local") == 0
    res0 = linearisable_batch(m, hists, max_nodes=MAXN, ctx=ctx, pending="complete", kpending_local=False)
    assert ctx.kpending_local_last() == 0 and not np.array_equal(res0.nodes, res.nodes)
    ctx.set_param("kpending_local", 1)
    try:                                                # None leaves the context's knob alone
        res1 = linearisable_batch(m, hists, max_nodes=MAXN, ctx=ctx, pending="complete")
        assert np.array_equal(res1.nodes, res.nodes) and ctx.get_param("kpending_local") == 1
        # a witness call: the product route whole
        resw = linearisable_batch(m, hists, max_nodes=MAXN, ctx=ctx, pending="complete", witness=True)
        assert np.array_equal(resw.nodes, res0.nodes) and ctx.kpending_local_last() == 0
    finally:
        ctx.set_param("kpending_local", 0)
    assert {"lin", "nonlin", "error"} <= {w[0] for w in want}
    for h, (st, _) in list(zip(hists, want))[:30]:
        if st == "error":
            with pytest.raises(ModelError):
                linearisable(m.transition, m.postcondition, None, h, ctx=ctx, max_nodes=MAXN, pending="complete",
                             kpending_local=True)
        else:
            assert linearisable(m.transition, m.postcondition, None, h, ctx=ctx, max_nodes=MAXN, pending="complete",
                                kpending_local=True) == (st == "lin")
        assert ctx.kpending_local_last() == 1
