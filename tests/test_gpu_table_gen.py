"""The table-model generator on the device (csrc/tgen.hip,
qsmd_gen_table_batch_device; Context.gen_table_device): byte parity with the
host generator over tgen_cases.CASES, no store past a partial group,
generate-and-check without leaving the device, and the entry point's
errors."""

import ctypes

import numpy as np
import pytest

import tgen_cases as tc
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, device, gen

gpu = pytest.mark.gpu

FILL = 0xA5
N_BIG = 20000           # 312 full groups and one half group
N_SMALL = (1, 63, 64, 65)


def _hold(ctx, m):
    """Make m the context's (narrow or wide) table; True when it is wide."""
    wide = m.model_id == 4
    if wide:
        if ctx.wide_table is not m:
            ctx.set_wide_table(m)
    elif ctx.table is not m:
        ctx.set_table(m)
    return wide


def device_generate(ctx, m, p, first, n, ev_base=0, pad=64):
    """(hdr, events, flags, tail_ok): the batch as the device wrote it, and
    whether the `pad` histories' worth of bytes past it still hold FILL."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    wide = _hold(ctx, m)
    per = 2 * p.n_ops
    d_hdr = torch.full(((n + pad) * 16,), FILL, dtype=torch.uint8, device=dev)
    d_ev = torch.full(((n + pad) * per * 8,), FILL, dtype=torch.uint8, device=dev)
    d_fl = torch.full((n + pad,), FILL, dtype=torch.uint8, device=dev)
    ctx.gen_table_device(p, first, n, d_hdr.data_ptr(), d_ev.data_ptr(), d_fl.data_ptr(), ev_base=ev_base,
                         stream=torch.cuda.current_stream().cuda_stream, wide=wide)
    torch.cuda.synchronize()
    hdr, ev, fl = d_hdr.cpu().numpy(), d_ev.cpu().numpy(), d_fl.cpu().numpy()
    tail_ok = bool(np.all(hdr[n * 16:] == FILL) and np.all(ev[n * per * 8:] == FILL) and np.all(fl[n:] == FILL))
    return (hdr[:n * 16].view(codec.HDR_DTYPE), ev[:n * per * 8].view(codec.EV_DTYPE), fl[:n], tail_ok)


# ------------------------------------------------------------ 1. device = host

@gpu
@pytest.mark.parametrize("case", tc.CASES, ids=tc.CASE_IDS)
def test_device_equals_host(ctx, case):
    _, name, kw, first, ev_base, w = case
    m = tc.model(name)
    p = gen.table_params(inv_weight=w, **kw)
    hdr_h, ev_h, fl_h = tc.host(case, N_BIG)
    per = 2 * kw["n_ops"]
    for n in (N_BIG,) + N_SMALL:
        hdr, ev, fl, tail_ok = device_generate(ctx, m, p, first, n, ev_base)
        assert hdr.tobytes() == hdr_h[:n].tobytes(), n
        assert ev.tobytes() == ev_h[:n * per].tobytes(), n
        assert fl.tobytes() == fl_h[:n].tobytes(), n
        assert tail_ok, n


@gpu
def test_device_without_flag_buffer_and_on_a_later_shard(ctx):
    """bug_dev is nullable, and a shard generated on its own is the whole
    stream's slice (the grid restarts at group 0, the RNG does not)."""
    torch = pytest.importorskip("torch")
    case = tc.CASES[tc.CASE_IDS.index("reg_4x16_bugs")]
    m = tc.model("register")
    p = gen.table_params(**case[2])
    _, ev_h, _ = tc.host(case, 300)
    _hold(ctx, m)
    d_hdr = torch.zeros(200 * 16, dtype=torch.uint8, device="cuda:0")
    d_ev = torch.zeros(200 * 32 * 8, dtype=torch.uint8, device="cuda:0")
    ctx.gen_table_device(p, 100, 200, d_hdr.data_ptr(), d_ev.data_ptr(), None,
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d_ev.cpu().numpy().tobytes() == ev_h[100 * 32:].tobytes()
    hdr = d_hdr.cpu().numpy().view(codec.HDR_DTYPE)
    assert np.array_equal(hdr["tag"], np.arange(100, 300)) and int(hdr["ev_off"][1]) == 32


# ------------------------------------- 2. generate and check on the device

def _generate_and_check(ctx, name, p_bug, n, max_nodes=0):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    m = tc.model(name)
    wide = _hold(ctx, m)
    p = gen.table_params(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=tc.IN_WINDOW, pid_mode=tc.PER_CLIENT,
                         p_bug=p_bug, seed=0xC0DE)
    per = 32
    d_hdr = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_ev = torch.zeros(n * per * 8, dtype=torch.uint8, device=dev)
    d_fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    d_nd = torch.zeros(n, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ctx.gen_table_device(p, 0, n, d_hdr.data_ptr(), d_ev.data_ptr(), d_fl.data_ptr(), stream=s, wide=wide)
    ctx.check_device(m.model_id, d_hdr.data_ptr(), n, d_ev.data_ptr(), n * per, d_st.data_ptr(), d_nd.data_ptr(),
                     flags=device.QSMD_FLAG_EXHAUSTIVE, max_nodes=max_nodes, stream=s)
    torch.cuda.synchronize()
    return (m, d_hdr.cpu().numpy().view(codec.HDR_DTYPE), d_ev.cpu().numpy().view(codec.EV_DTYPE),
            d_fl.cpu().numpy(), d_st.cpu().numpy(), d_nd.cpu().numpy().astype(np.uint64))


@gpu
@pytest.mark.parametrize("name", ["register", "kv"])
def test_generated_on_device_checks_linearisable(ctx, name):
    _, _, _, fl, st, _ = _generate_and_check(ctx, name, 0.0, N_BIG)
    assert not np.any(fl)
    assert np.all(st == codec.STATUS_LIN)


@gpu
@pytest.mark.parametrize("name", ["register", "kv"])
def test_generated_bugs_check_as_the_oracle_says(ctx, name):
    m, hdr, ev, fl, st, nd = _generate_and_check(ctx, name, 0.5, N_BIG, max_nodes=20000)
    assert 0.48 <= np.count_nonzero(fl & 1) / N_BIG <= 0.52
    c = tc.CLOSURES[name]
    seen = set()
    for i in range(300):
        st_o, nd_o, _ = oracle_linearisable(c["transition"], c["postcondition"], c["init"],
                                            tc.history(m, hdr, ev, i), 20000)
        assert (codec.STATUS_NAMES[int(st[i])], int(nd[i])) == (st_o, nd_o), i
        seen.add(st_o)
    assert {"lin", "nonlin"} <= seen


# ------------------------------------------------------------------ 3. errors

def _try(ctx, p, n=64, wide=False, ev_base=0):
    torch = pytest.importorskip("torch")
    per = 2 * max(1, min(int(p.n_ops), 64))
    d_hdr = torch.full((n * 16,), FILL, dtype=torch.uint8, device="cuda:0")
    d_ev = torch.full((n * per * 8,), FILL, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(device.DeviceError, match=r"\(-1\)"):
        ctx.gen_table_device(p, 0, n, d_hdr.data_ptr(), d_ev.data_ptr(), None, ev_base=ev_base, wide=wide)
    torch.cuda.synchronize()
    assert bool((d_hdr == FILL).all()) and bool((d_ev == FILL).all())


GOOD = dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=1, pid_mode=0, p_bug=0.5, seed=1)


@gpu
def test_no_table_set_is_an_argument_error():
    with device.Context(0) as c:
        _try(c, gen.table_params(**GOOD))
        _try(c, gen.table_params(**GOOD), wide=True)
        c.set_table(tc.model("register"))
        _try(c, gen.table_params(**GOOD), wide=True)       # the narrow table does not serve model 4


@gpu
@pytest.mark.parametrize("field,value", [("n_clients", 0), ("n_clients", 33), ("n_ops", 0), ("n_ops", 65),
                                         ("lin_policy", 2), ("pid_mode", 2), ("p_bug", float("nan")),
                                         ("p_bug", -0.5), ("p_bug", 1.5)])
def test_bad_parameters_are_argument_errors(ctx, field, value):
    _hold(ctx, tc.model("register"))
    _try(ctx, gen.table_params(**dict(GOOD, **{field: value})))


@gpu
def test_bad_weights_model_id_and_offsets_are_argument_errors(ctx):
    _hold(ctx, tc.model("register"))
    _try(ctx, gen.table_params(inv_weight=[0] * 21, **GOOD))
    _try(ctx, gen.table_params(inv_weight=[1 << 31, 1 << 31] + [0] * 19, **GOOD))
    _try(ctx, gen.table_params(**GOOD), ev_base=(1 << 32) - 100)
    lib = device.load_library()
    p = gen.table_params(**GOOD)
    for mid in (0, 1, 2, 5):
        p.model_id = mid
        assert lib.qsmd_gen_table_batch_device(ctx._h, ctypes.byref(p), 0, 0, 0, None, None, None,
                                               None) == -1
    # qsmd_gen_batch_device still knows Bank and TicketDispenser only
    q = gen.params(model_id=3, n_clients=4, n_ops=16, prefix_ops=4)
    with pytest.raises(device.DeviceError, match=r"\(-1\)"):
        ctx.gen_device(q, 0, 0, None, None)


@gpu
def test_a_replaced_table_is_the_one_generated_from():
    """qsmd_table_set right after a generate call waits for it before it frees
    the table, and the next generate call reads the new one."""
    torch = pytest.importorskip("torch")
    n, per = N_BIG, 32
    reg, lock = tc.model("register"), tc.model("lock")
    p = gen.table_params(**GOOD)
    pl = gen.table_params(inv_weight=(6, 1, 6), **GOOD)
    with device.Context(0) as c:
        bufs = [[torch.zeros(n * k, dtype=torch.uint8, device="cuda:0") for k in (16, per * 8, 1)] for _ in (0, 1)]
        s = torch.cuda.current_stream().cuda_stream
        c.set_table(reg)
        c.gen_table_device(p, 0, n, *(b.data_ptr() for b in bufs[0]), stream=s)
        c.set_table(lock)                                   # no synchronisation of ours in between
        c.gen_table_device(pl, 0, n, *(b.data_ptr() for b in bufs[1]), stream=s)
        torch.cuda.synchronize()
        for got, (m, q) in zip(bufs, ((reg, p), (lock, pl))):
            want = gen.generate_table(q, m, 0, n)
            assert all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(got, want))
