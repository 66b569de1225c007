"""GPU parity of the explain calls (include/qsmd.h qsmd_explain_batch; the
EXPLAIN instantiations of csrc/table.hip, csrc/wtable.hip, csrc/ktable.hip)
with the literal restatement of their rule (tests/explain_ref.py): status,
nodes, the reported path's operations, its depth and the model state at its
end, for every history -- `budget` ones too, at the same max_nodes on both
sides -- in every width class and in both passes."""

import functools

import numpy as np
import pytest

import explain_ref as xr
import tablegen as tg
import wtablegen as wg
from qsmd import codec, device
from qsmd.linearisability import ExplainResult, decode_state, explain, explain_batch
from qsmd.models import EncodeError
from test_gpu_ktable import keyed, prod
from test_gpu_table import EXH, MAXN, rc_of, table, witness_path

pytestmark = pytest.mark.gpu

# device model -> (model id, its closures)
MODELS = {"register": 3, "lock": 3, "kv": 4, "register^4": 5}
SHAPES = list(xr.SHAPES) + [xr.ANYSHAPE]
CLASS_OF = {"3x10": 32, "4x16": 32, "3x24": 64, "2x40": 128, "3x40": 128}
SENTINEL = 0xEE
NAMES = codec.STATUS_NAMES


@pytest.fixture(scope="module")
def ctx():
    """This module's own context (it sets a keyed table: see test_gpu_ktable.py)."""
    c = device.Context(0, time_limit_ms=60000)
    yield c
    c.close()


def closures(key):
    if key == "register^4":
        return prod("register", 4)
    return {"register": tg.REGISTER, "lock": tg.LOCK, "kv": wg.KV}[key]


def device_model(key):
    if MODELS[key] == 3:
        return table(key)
    return wg.wide_table(key) if MODELS[key] == 4 else keyed("register", 4)


@functools.lru_cache(maxsize=None)
def case(key, shape):
    """The histories of one shape and the restatement's results (computed
    once, shared, never changed)."""
    hists = xr.histories(closures(key), shape)
    return hists, xr.explain_all(closures(key), hists, MAXN)


def set_model(ctx, key):
    mid, m = MODELS[key], device_model(key)
    if mid == 3 and ctx.table is not m:
        ctx.set_table(m)
    elif mid == 4 and ctx.wide_table is not m:
        ctx.set_wide_table(m)
    elif mid == 5 and ctx.keyed_table is not m:
        ctx.set_keyed_table(m)
    return mid, m


@functools.lru_cache(maxsize=None)
def encoded(key, shape):
    batch = codec.encode(device_model(key), case(key, shape)[0])
    assert not batch.encode_errors
    return batch


def run(ctx, key, shape, fill=0xFF, flags=EXH):
    """The host entry: (status, nodes, path, records, totals)."""
    mid, _ = set_model(ctx, key)
    batch = encoded(key, shape)
    return ctx.explain_arrays(mid, batch.hdr, batch.events, None, flags, MAXN,
                              path=np.full(len(batch.events), fill, dtype=np.uint8))


def path_of(hdr, path, i):
    o, n = int(hdr[i]["ev_off"]), int(hdr[i]["n_ev"])
    out = []
    for x in path[o:o + n]:
        if x == codec.WITNESS_END:
            break
        out.append(int(x))
    return out


def assert_parity(key, shape, got):
    m = device_model(key)
    hists, ref = case(key, shape)
    hdr = encoded(key, shape).hdr
    st, nd, path, rec, tot = got
    assert len(st) == len(hists)
    for i, (h, (st_r, nd_r, ops_r, model_r)) in enumerate(zip(hists, ref)):
        p = path_of(hdr, path, i)
        state = decode_state(m, int(rec["state"][i]))
        got_i = (NAMES[int(st[i])], int(nd[i]), witness_path(h, p), int(rec["depth"][i]), state)
        assert got_i == (st_r, nd_r, ops_r, len(ops_r), tuple(model_r) if isinstance(model_r, tuple) else model_r), i
        assert int(rec["reserved"][i]) == 0 and int(rec["reserved2"][i]) == 0
    names = [NAMES[int(s)] for s in st]
    assert tot["linearisable"] == names.count("lin") and tot["nonlinearisable"] == names.count("nonlin")
    assert tot["model_errors"] == names.count("error") and tot["budget"] == names.count("budget")
    assert tot["encode_errors"] == 0 and tot["nodes"] == int(np.sum(nd.astype(np.uint64)))


class knobs:
    """Set table knobs; restore them on exit."""
    NAMES = ("table_budget", "table_memo", "ktable_memo", "ktable_local")

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


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


# ----------------------------------------------------- 1. parity, both passes

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("key", list(MODELS))
def test_parity_with_the_restatement(ctx, key, shape):
    """At the default "table_budget", with a single pass (0) and with nearly
    every search sent through pass 2 and its rewrite of the path (4)."""
    ref = case(key, shape)[1]
    default = ctx.get_param("table_budget")
    assert default == 256
    for budget in (default, 0, 4):
        with knobs(ctx, table_budget=budget):
            got = run(ctx, key, shape)
            pass2 = ctx.table_pass2()
        assert_parity(key, shape, got)
        taken = 0 if budget == 0 else sum(r[1] > budget or (r[0] == "budget" and r[1] >= budget) for r in ref)
        assert pass2 == taken, budget
    assert not ctx.timed_out()
    if shape in CLASS_OF:
        n_ev = encoded(key, shape).hdr["n_ev"]
        lo = {32: 0, 64: 32, 128: 64}[CLASS_OF[shape]]
        assert ((n_ev > lo) & (n_ev <= CLASS_OF[shape])).all()


def test_inputs_reach_every_status_and_depth_0():
    for key in MODELS:
        seen = set()
        for shape in SHAPES:
            seen |= {(r[0], len(r[2]) == 0) for r in case(key, shape)[1]}
        assert {("lin", False), ("nonlin", False), ("nonlin", True)} <= seen, key
        assert ("error", False) in seen or key != "lock", key
    # a deepest path that is not the last one searched: the record, not the stack
    assert any(r[0] == "nonlin" and r[1] > 2 * len(r[2]) > 0 for r in case("register", "4x16")[1])


SMALL = 40      # a max_nodes many searches of these shapes pass


@functools.lru_cache(maxsize=None)
def small_case(key, shape):
    return xr.explain_all(closures(key), case(key, shape)[0], SMALL)


@pytest.mark.parametrize("key", list(MODELS))
def test_budget_from_max_nodes(ctx, key):
    """A search that passes max_nodes reads BUDGET with the first deepest path
    among the max_nodes nodes counted, in one pass and through pass 2."""
    mid, m = set_model(ctx, key)
    for shape in ("4x16", "3x24", "3x40", xr.ANYSHAPE):
        hists, ref = case(key, shape)[0], small_case(key, shape)
        assert sum(r[0] == "budget" for r in ref) >= 3, shape
        batch = encoded(key, shape)
        for budget in (256, 0, 4):
            with knobs(ctx, table_budget=budget):
                st, nd, path, rec, _ = ctx.explain_arrays(mid, batch.hdr, batch.events, None, EXH, SMALL)
            for i, (h, (st_r, nd_r, ops_r, model_r)) in enumerate(zip(hists, ref)):
                got = (NAMES[int(st[i])], int(nd[i]), witness_path(h, path_of(batch.hdr, path, i)),
                       int(rec["depth"][i]), decode_state(m, int(rec["state"][i])))
                assert got == (st_r, nd_r, ops_r, len(ops_r), tuple_or(model_r)), (shape, budget, i)
                assert st_r != "budget" or nd_r == SMALL


# ------------------------------------- 2. the check call's results, the witness

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("key", list(MODELS))
def test_equals_the_check_call(ctx, key, shape):
    mid, _ = set_model(ctx, key)
    batch = encoded(key, shape)
    st, nd, path, rec, tot = run(ctx, key, shape)
    st_c, nd_c, wit, tot_c = ctx.check_arrays(mid, batch.hdr, batch.events, None, EXH, MAXN, witness=True)
    assert np.array_equal(st, st_c) and np.array_equal(nd, nd_c) and tot == tot_c
    lin = [i for i in range(len(st)) if st[i] == codec.STATUS_LIN]
    assert lin
    for i in lin:
        o, n = int(batch.hdr[i]["ev_off"]), int(batch.hdr[i]["n_ev"])
        d = int(rec["depth"][i])
        assert np.array_equal(path[o:o + min(d + 1, n)], wit[o:o + min(d + 1, n)]), i
        assert d == n or path[o + d] == codec.WITNESS_END


# ------------------------------------------------------- 3. the knobs it ignores

@pytest.mark.parametrize("key", list(MODELS))
def test_memo_and_local_knobs_change_nothing(ctx, key):
    for shape in ("4x16", "3x40", xr.ANYSHAPE):
        plain = run(ctx, key, shape, fill=SENTINEL)
        with knobs(ctx, table_memo=4096, ktable_memo=4096, ktable_local=1):
            assert same(plain, run(ctx, key, shape, fill=SENTINEL)), shape
            assert ctx.ktable_local_last() == 0 and ctx.table_memo_hits() == 0
        with knobs(ctx, table_budget=4, table_memo=4096, ktable_memo=4096, ktable_local=1):
            got = run(ctx, key, shape, fill=SENTINEL)
            assert ctx.table_memo_hits() == 0
        assert_parity(key, shape, got)
        # QSMD_FLAG_WITNESS and QSMD_FLAG_MEMO are accepted and change nothing
        flags = EXH | device.QSMD_FLAG_WITNESS | device.QSMD_FLAG_MEMO
        assert same(plain, run(ctx, key, shape, fill=SENTINEL, flags=flags)), shape


# ------------------------------------------------------------ 4. the device entry

@pytest.mark.parametrize("key", list(MODELS))
def test_device_entry_on_another_stream(ctx, key):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    mid, _ = set_model(ctx, key)
    for shape in ("3x10", "3x24", "3x40", xr.ANYSHAPE):
        batch = encoded(key, shape)
        host = run(ctx, key, shape, fill=SENTINEL)
        n, n_ev = len(batch.hdr), len(batch.events)
        d_hdr = torch.from_numpy(batch.hdr.view(np.uint8).copy()).to(dev)
        d_ev = torch.from_numpy(batch.events.view(np.uint8).copy()).to(dev)
        d_st = torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)
        d_nd = torch.full((n,), -1, dtype=torch.int64, device=dev)
        d_path = torch.full((n_ev,), SENTINEL, dtype=torch.uint8, device=dev)
        d_rec = torch.full((n * 16,), SENTINEL, dtype=torch.uint8, device=dev)
        d_tot = torch.full((8,), -1, dtype=torch.int64, device=dev)
        stream = torch.cuda.Stream()
        assert stream.cuda_stream != torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ctx.explain_device(mid, d_hdr.data_ptr(), n, d_ev.data_ptr(), n_ev, d_st.data_ptr(), d_path.data_ptr(),
                               d_rec.data_ptr(), d_nd.data_ptr(), d_tot.data_ptr(), max_nodes=MAXN,
                               stream=stream.cuda_stream)
        stream.synchronize()
        tot = dict(zip((f for f, _ in device.Totals._fields_), (int(x) for x in d_tot.cpu().numpy())))
        got = (d_st.cpu().numpy(), d_nd.cpu().numpy().astype(np.uint64), d_path.cpu().numpy(),
               d_rec.cpu().numpy().view(device.EXPLAIN_DTYPE), tot)
        assert same(host, got), shape
        assert_parity(key, shape, got)
        # nodes_dev and totals_dev may be NULL
        d_st.fill_(SENTINEL)
        ctx.explain_device(mid, d_hdr.data_ptr(), n, d_ev.data_ptr(), n_ev, d_st.data_ptr(), d_path.data_ptr(),
                           d_rec.data_ptr(), max_nodes=MAXN, stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(d_st.cpu().numpy(), host[0])


# ------------------------------------------------- 5. encode errors, empty histories

@pytest.mark.parametrize("key", list(MODELS))
def test_encode_errors_and_empty_histories(ctx, key):
    mid, m = set_model(ctx, key)
    hists = case(key, "3x10")[0][:6]
    ref = case(key, "3x10")[1][:6]
    batch = codec.encode(m, hists[:3] + [[]] + hists[3:])
    n0 = len(batch.events)
    pad = 8
    ev = np.concatenate([batch.events, np.zeros(pad, dtype=codec.EV_DTYPE)])
    hdr = np.concatenate([batch.hdr, np.zeros(4, dtype=codec.HDR_DTYPE)])
    hdr[7:] = batch.hdr[0]
    hdr["ev_off"][7], hdr["n_ev"][7] = n0 + 1, pad              # past the end of the events: slot starts inside
    hdr["ev_off"][8], hdr["n_ev"][8] = n0 + pad, 4              # starts outside
    hdr["ev_off"][9], hdr["n_ev"][9], hdr["model_id"][9] = n0 + 4, 2, 1     # another model's header
    hdr["ev_off"][10], hdr["n_ev"][10] = n0 + 6, 0              # empty, inside
    bad = 5                                                     # a symbol the table does not have
    o5 = int(hdr["ev_off"][bad])
    ev["code"][o5 + 1] = 0xFF
    st, nd, path, rec, tot = ctx.explain_arrays(mid, hdr, ev, None, EXH, MAXN,
                                                path=np.full(len(ev), SENTINEL, dtype=np.uint8))
    good = [0, 1, 2, 4, 6]
    for i, r in zip(good, ref[:3] + ref[3:4] + ref[5:6]):
        h = (hists[:3] + [[]] + hists[3:])[i]
        assert (NAMES[int(st[i])], int(nd[i]), witness_path(h, path_of(hdr, path, i))) == r[:3], i
    enc = [bad, 7, 8, 9]
    assert [int(st[i]) for i in enc] == [codec.STATUS_ENCODE_ERROR] * 4 and not nd[enc].any()
    assert not rec[enc].view(np.uint8).any()
    # the slot: its first byte the terminator, the rest as given
    n5 = int(hdr["n_ev"][bad])
    assert path[o5] == codec.WITNESS_END and (path[o5 + 1:o5 + n5] == SENTINEL).all()
    tail = path[n0:]
    expect = np.full(pad, SENTINEL, dtype=np.uint8)
    expect[1] = expect[4] = codec.WITNESS_END
    assert np.array_equal(tail, expect)
    # empty histories: LINEARISABLE, depth 0, the initial state, no byte written
    for i in (3, 10):
        assert int(st[i]) == codec.STATUS_LIN and int(nd[i]) == 0 and int(rec["depth"][i]) == 0
        assert decode_state(m, int(rec["state"][i])) == tuple_or(closures(key)["init"])
    assert tot["encode_errors"] == 4 and tot["linearisable"] == 2 + [r[0] for r in ref[:4] + ref[5:6]].count("lin")


def tuple_or(x):
    return tuple(x) if isinstance(x, tuple) else x


def test_empty_batch_and_model0(ctx):
    mid, m = set_model(ctx, "register")
    st, nd, path, rec, tot = ctx.explain_arrays(3, np.zeros(0, dtype=codec.HDR_DTYPE),
                                                np.zeros(0, dtype=codec.EV_DTYPE))
    assert len(st) == len(rec) == len(path) == 0 and tot["checked"] == 0
    # another initial state: an empty history and a depth-0 failure report it
    L, R = tg.L, tg.R
    res = explain_batch(m, [[], [(0, L("Read")), (0, R(("Val", 0)))], [(0, L("Read")), (0, R(("Val", 2)))]], 2, ctx=ctx)
    assert [res.verdict(i) for i in range(3)] == ["lin", "nonlin", "lin"]
    assert [res.state_of(i) for i in range(3)] == [2, 2, 2] and list(res.depth) == [0, 0, 1]


# -------------------------------------------------------------- 6. argument errors

def good_batch_still_explains(ctx, key="register"):
    got = run(ctx, key, "3x10")
    assert_parity(key, "3x10", got)


def test_argument_errors(ctx):
    set_model(ctx, "register")
    batch = encoded("register", "3x10")
    for mid in (1, 2):
        with pytest.raises(device.DeviceError) as e:
            ctx.explain_arrays(mid, batch.hdr, batch.events, None, EXH, MAXN)
        assert rc_of(e) == -4
    good_batch_still_explains(ctx)
    with pytest.raises(device.DeviceError) as e:
        ctx.explain_arrays(3, batch.hdr, batch.events, None, EXH | device.QSMD_FLAG_EARLY_EXIT_BATCH, MAXN)
    assert rc_of(e) == -4
    with pytest.raises(device.DeviceError) as e:
        ctx.explain_arrays(9, batch.hdr, batch.events, None, EXH, MAXN)
    assert rc_of(e) == -1
    import ctypes
    with pytest.raises(device.DeviceError) as e:     # model0: a state the table does not have
        ctx.explain_arrays(3, batch.hdr, batch.events, ctypes.c_uint32(200), EXH, MAXN)
    assert rc_of(e) == -1
    good_batch_still_explains(ctx)
    # NULL path / explain outputs
    lib, n, st = ctx._lib, len(batch.hdr), np.empty(len(batch.hdr), dtype=np.uint8)
    rec = np.zeros(n, dtype=device.EXPLAIN_DTYPE)
    pth = np.zeros(len(batch.events), dtype=np.uint8)
    for p, x in ((None, rec.ctypes.data), (pth.ctypes.data, None)):
        assert lib.qsmd_explain_batch(ctx._h, 3, batch.hdr.ctypes.data, n, batch.events.ctypes.data,
                                      len(batch.events), None, EXH, MAXN, st.ctypes.data, None, p, x, None) == -1
        assert lib.qsmd_explain_batch_device(ctx._h, 3, batch.hdr.ctypes.data, n, batch.events.ctypes.data,
                                             len(batch.events), None, EXH, MAXN, st.ctypes.data, None, p, x, None,
                                             None) == -1
    good_batch_still_explains(ctx)
    # no table set: a fresh context
    fresh = device.Context(0)
    try:
        for mid in (3, 4, 5):
            with pytest.raises(device.DeviceError) as e:
                fresh.explain_arrays(mid, batch.hdr, batch.events, None, EXH, MAXN)
            assert rc_of(e) == -1
    finally:
        fresh.close()


# -------------------------------------------------------------- 7. the Python API

@pytest.mark.parametrize("key", list(MODELS))
def test_explanations_print(ctx, key):
    m = device_model(key)
    hists, ref = [], []
    for shape in ("3x10", "4x16", xr.ANYSHAPE):
        hists += case(key, shape)[0]
        ref += case(key, shape)[1]
    res = explain_batch(m, hists, max_nodes=MAXN, ctx=ctx)
    assert isinstance(res, ExplainResult)
    seen = {}
    for i, r in enumerate(ref):
        if seen.setdefault(r[0], 0) >= 3:
            continue
        seen[r[0]] += 1
        e = res.explanation(i)          # (checks that the path replays to the device's depth and state)
        assert (e.status, e.prefix) == (r[0], r[2]) and tuple_or(e.model) == tuple_or(r[3])
        text = e.pretty()
        assert text.count("=/=>") == len(e.stuck) and text.count("==>") >= len(e.prefix)
        outcomes = {s[3] for s in e.stuck}
        if r[0] == "nonlin":
            assert outcomes <= {"no response", "postcondition false"}
        if r[0] == "error":
            assert "raises" in outcomes
        if r[0] == "lin":
            assert res.witness_of(i) == res.path_of(i) and outcomes <= {"no response"}
    assert {"lin", "nonlin"} <= set(seen)
    # one history, the reference's signature
    i = next(i for i, r in enumerate(ref) if r[0] == "nonlin" and r[2])
    e = explain(m.transition, m.postcondition, None, hists[i], max_nodes=MAXN, ctx=ctx)
    assert (e.status, e.prefix) == ("nonlin", ref[i][2])
    with pytest.raises(EncodeError):
        explain(m.transition, m.postcondition, None, [(0, tg.L("no such symbol")), (0, tg.R("Ok"))], ctx=ctx)
