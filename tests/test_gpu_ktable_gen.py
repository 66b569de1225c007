"""The keyed-table-model generator on the device (csrc/ktgen.hip,
qsmd_gen_ktable_batch_device; Context.gen_ktable_device): byte parity with
the host generator over ktgen_cases.CASES, no store past a partial group, the
grid-stride loop under the blob-size grid cap, generate-and-check as model 5
without leaving the device, the entry point's errors, and the narrow and wide
tables beside the keyed one."""

import ctypes

import numpy as np
import pytest

import ktgen_cases as kc
import tgen_cases as tc
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device, gen

gpu = pytest.mark.gpu

FILL = 0xA5
N_CASE = 64 * 3 + 7       # three full groups and a partial one


@pytest.fixture(scope="module")
def ctx():
    """This module's own context: the session's must stay without a keyed
    table (tests/test_gpu_wtable.py)."""
    c = device.Context(0, time_limit_ms=60000)
    yield c
    c.close()


def _hold(ctx, m):
    if ctx.keyed_table is not m:
        ctx.set_keyed_table(m)


def device_generate(ctx, m, p, first, n, ev_base=0, pad=64, flags=True):
    """(hdr, events, flags, tail_ok): the batch as the device wrote it, and
    whether the `pad` histories' worth of bytes past it still hold FILL."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    _hold(ctx, m)
    per = 2 * p.n_ops
    d_hdr = torch.full(((n + pad) * 16,), FILL, dtype=torch.uint8, device=dev)
    d_ev = torch.full(((n + pad) * per * 8,), FILL, dtype=torch.uint8, device=dev)
    d_fl = torch.full((n + pad,), FILL, dtype=torch.uint8, device=dev)
    ctx.gen_ktable_device(p, first, n, d_hdr.data_ptr(), d_ev.data_ptr(), d_fl.data_ptr() if flags else None,
                          ev_base=ev_base, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    hdr, ev, fl = d_hdr.cpu().numpy(), d_ev.cpu().numpy(), d_fl.cpu().numpy()
    tail_ok = bool(np.all(hdr[n * 16:] == FILL) and np.all(ev[n * per * 8:] == FILL) and
                   np.all(fl[n if flags else 0:] == FILL))
    return (hdr[:n * 16].view(codec.HDR_DTYPE), ev[:n * per * 8].view(codec.EV_DTYPE), fl[:n], tail_ok)


# ------------------------------------------------------------ 1. device = host

@gpu
@pytest.mark.parametrize("cid", kc.CASE_IDS)
def test_device_equals_host(ctx, cid):
    c = kc.case(cid)
    m, p = kc.model(c[1], c[2]), kc.params(c)
    hdr_h, ev_h, fl_h = kc.host(c, N_CASE)
    hdr, ev, fl, tail_ok = device_generate(ctx, m, p, c[4], N_CASE, c[5])
    assert hdr.tobytes() == hdr_h.tobytes()
    assert ev.tobytes() == ev_h.tobytes()
    assert fl.tobytes() == fl_h.tobytes()
    assert tail_ok
    # bug_dev = NULL: the same headers and events, no flag byte written
    hdr, ev, _, tail_ok = device_generate(ctx, m, kc.params(c), c[4], N_CASE, c[5], flags=False)
    assert hdr.tobytes() == hdr_h.tobytes() and ev.tobytes() == ev_h.tobytes() and tail_ok


# ------------------------------------------------------------ 2. grid-stride

@gpu
def test_grid_stride_under_the_blob_size_cap(ctx):
    """The 80 KB component caps the grid at 8 workgroups per CU, so 8 x CUs x
    64 + 70 histories make the stride loop run twice in some workgroups."""
    torch = pytest.importorskip("torch")
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 64 + 70
    m = kc.model("rand_narrow", 8)
    kw = dict(n_clients=2, n_ops=2, prefix_ops=0, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT, p_bug=0.5,
              seed=0x6121D)
    hdr_h, ev_h, fl_h = gen.generate_ktable(gen.ktable_params(**kw), m, 11, n)
    hdr, ev, fl, tail_ok = device_generate(ctx, m, gen.ktable_params(**kw), 11, n)
    assert hdr.tobytes() == hdr_h.tobytes()
    assert ev.tobytes() == ev_h.tobytes()
    assert fl.tobytes() == fl_h.tobytes()
    assert tail_ok


# ------------------------------------- 3. generate and check on the device

N_CHECK = 4096


def _generate_and_check(ctx, p_bug, max_nodes=0):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    m = kc.model("register", 4)
    _hold(ctx, m)
    p = gen.ktable_params(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT,
                          p_bug=p_bug, seed=0xC0DE)
    n, per = N_CHECK, 32
    d_hdr = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_ev = torch.zeros(n * per * 8, dtype=torch.uint8, device=dev)
    d_fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    d_nd = torch.zeros(n, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ctx.gen_ktable_device(p, 0, n, d_hdr.data_ptr(), d_ev.data_ptr(), d_fl.data_ptr(), stream=s)
    ctx.check_device(5, d_hdr.data_ptr(), n, d_ev.data_ptr(), n * per, d_st.data_ptr(), d_nd.data_ptr(),
                     flags=device.QSMD_FLAG_EXHAUSTIVE, max_nodes=max_nodes, stream=s)
    torch.cuda.synchronize()
    return (m, d_hdr.cpu().numpy().view(codec.HDR_DTYPE), d_ev.cpu().numpy().view(codec.EV_DTYPE),
            d_fl.cpu().numpy(), d_st.cpu().numpy(), d_nd.cpu().numpy().astype(np.uint64))


@pytest.fixture()
def memo_off(ctx):
    yield
    ctx.set_param("ktable_memo", 0)


@gpu
def test_generated_on_device_checks_linearisable(ctx, memo_off):
    for memo in (0, 64):
        ctx.set_param("ktable_memo", memo)
        _, _, _, fl, st, _ = _generate_and_check(ctx, 0.0)
        assert not np.any(fl)
        assert np.all(st == codec.STATUS_LIN), memo


@gpu
def test_generated_bugs_check_as_the_oracle_says(ctx, memo_off):
    m, hdr, ev, fl, st, nd = _generate_and_check(ctx, 0.5, max_nodes=20000)
    # Binomial(4096, 1/2): six standard deviations
    assert abs(np.count_nonzero(fl & 1) - N_CHECK / 2) <= 6 * np.sqrt(N_CHECK / 4)
    p = kc.product("register", 4)
    seen = set()
    for i in range(300):
        st_o, nd_o, _ = oracle_linearisable(p["transition"], p["postcondition"], p["init"],
                                            kc.history(m, hdr, ev, i), 20000)
        assert (codec.STATUS_NAMES[int(st[i])], int(nd[i])) == (st_o, nd_o), i
        seen.add(st_o)
    assert {"lin", "nonlin"} <= seen
    ctx.set_param("ktable_memo", 64)
    _, hdr2, ev2, fl2, st2, nd2 = _generate_and_check(ctx, 0.5, max_nodes=20000)
    assert ev2.tobytes() == ev.tobytes() and fl2.tobytes() == fl.tobytes()
    assert np.array_equal(st2, st) and np.array_equal(nd2, nd)


# ------------------------------------------------------------------ 4. errors

GOOD = dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=1, pid_mode=0, p_bug=0.5, seed=1)


def _try(c, p, n=64, ev_base=0):
    torch = pytest.importorskip("torch")
    per = 2 * max(1, min(int(p.n_ops), 64))
    d_hdr = torch.full((n * 16,), FILL, dtype=torch.uint8, device="cuda:0")
    d_ev = torch.full((n * per * 8,), FILL, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(device.DeviceError, match=r"\(-1\)"):
        c.gen_ktable_device(p, 0, n, d_hdr.data_ptr(), d_ev.data_ptr(), None, ev_base=ev_base)
    torch.cuda.synchronize()
    assert bool((d_hdr == FILL).all()) and bool((d_ev == FILL).all())


@gpu
def test_no_keyed_table_and_other_key_counts_are_argument_errors():
    with device.Context(0) as c:
        _try(c, gen.ktable_params(n_keys=4, **GOOD))
        c.set_table(tc.model("register"))                   # the narrow table does not serve the keyed generator
        _try(c, gen.ktable_params(n_keys=1, **GOOD))
        c.set_keyed_table(kc.model("register", 4))
        for keys in (1, 3, 5, 8, 9):
            _try(c, gen.ktable_params(n_keys=keys, **GOOD))
        lib = device.load_library()
        p = gen.ktable_params(n_keys=0, **GOOD)             # (the binding fills a 0 in; the C entry refuses it)
        assert lib.qsmd_gen_ktable_batch_device(c._h, ctypes.byref(p), 0, 0, 0, None, None, None, None) == -1
        p.n_keys = 4
        assert lib.qsmd_gen_ktable_batch_device(c._h, ctypes.byref(p), 0, 0, 0, None, None, None, None) == 0


@gpu
@pytest.mark.parametrize("field,value", [("n_clients", 0), ("n_clients", 33), ("n_ops", 0), ("n_ops", 65),
                                         ("lin_policy", 2), ("pid_mode", 2), ("p_bug", float("nan")),
                                         ("p_bug", -0.5), ("p_bug", 1.5)])
def test_bad_parameters_are_argument_errors(ctx, field, value):
    _hold(ctx, kc.model("register", 4))
    _try(ctx, gen.ktable_params(**dict(GOOD, **{field: value})))


@gpu
def test_bad_weights_and_offsets_are_argument_errors(ctx):
    _hold(ctx, kc.model("register", 4))
    P = gen.ktable_params
    _try(ctx, P(inv_weight=[0] * 21, **GOOD))
    _try(ctx, P(key_weight=[0] * 4, **GOOD))
    _try(ctx, P(inv_weight=[1 << 31, 1 << 31] + [0] * 19, key_weight=[1, 0, 0, 0], **GOOD))
    _try(ctx, P(inv_weight=[1 << 31] + [0] * 20, key_weight=[1, 1, 0, 0], **GOOD))
    _try(ctx, P(inv_weight=[1 << 16] + [0] * 20, key_weight=[1 << 16, 0, 0, 0], **GOOD))
    _try(ctx, P(**GOOD), ev_base=(1 << 32) - 100)
    with pytest.raises(ValueError):
        ctx.gen_ktable_device(P(key_weight=[1, 2], **GOOD), 0, 0, None, None)


# ----------------------------------------------- 5. a replaced keyed table

@gpu
def test_a_replaced_keyed_table_is_the_one_generated_from():
    """qsmd_ktable_set right after a generate call waits for it before it
    frees the component, and the next generate call reads the new one (with
    its own number of keys)."""
    torch = pytest.importorskip("torch")
    n, per = 20000, 32
    reg, lock = kc.model("register", 4), kc.model("lock", 8)
    p = gen.ktable_params(**GOOD)
    pl = gen.ktable_params(inv_weight=(6, 1, 6), **GOOD)
    with device.Context(0) as c:
        bufs = [[torch.zeros(n * k, dtype=torch.uint8, device="cuda:0") for k in (16, per * 8, 1)] for _ in (0, 1)]
        s = torch.cuda.current_stream().cuda_stream
        c.set_keyed_table(reg)
        c.gen_ktable_device(p, 0, n, *(b.data_ptr() for b in bufs[0]), stream=s)
        c.set_keyed_table(lock)                             # no synchronisation of ours in between
        c.gen_ktable_device(pl, 0, n, *(b.data_ptr() for b in bufs[1]), stream=s)
        torch.cuda.synchronize()
        assert pl.n_keys == 8
        for got, (m, q) in zip(bufs, ((reg, p), (lock, pl))):
            want = gen.generate_ktable(q, m, 0, n)
            assert all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(got, want))


# ------------------------------------- 6. the narrow and wide tables beside it

@gpu
def test_narrow_and_wide_tables_are_not_disturbed():
    torch = pytest.importorskip("torch")
    n, per = 2000, 32
    reg, kv = tc.model("register"), tc.model("kv")
    sched = dict(GOOD, seed=0xBE51DE)

    def table_gen(c, wide):
        bufs = [torch.zeros(n * k, dtype=torch.uint8, device="cuda:0") for k in (16, per * 8, 1)]
        c.gen_table_device(gen.table_params(**sched), 5, n, *(b.data_ptr() for b in bufs),
                           stream=torch.cuda.current_stream().cuda_stream, wide=wide)
        torch.cuda.synchronize()
        return [b.cpu().numpy().tobytes() for b in bufs]

    with device.Context(0) as c:
        c.set_table(reg)
        c.set_wide_table(kv)
        before = [table_gen(c, False), table_gen(c, True)]
        m = kc.model("lock", 8)
        got = device_generate(c, m, gen.ktable_params(inv_weight=(6, 1, 6), **sched), 5, n)
        want = gen.generate_ktable(gen.ktable_params(inv_weight=(6, 1, 6), **sched), m, 5, n)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:3], want)) and got[3]
        assert [table_gen(c, False), table_gen(c, True)] == before
        want3 = gen.generate_table(gen.table_params(**sched), reg, 5, n)
        assert before[0] == [x.tobytes() for x in want3]
