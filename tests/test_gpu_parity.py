"""GPU parity: the HIP search (through the C ABI) against the oracle.

Bar: bit-exact verdicts, node counts and witness paths for every history
(integer search, no tolerance).  Oracles: the C restatement (oracle/ref_cpu.c),
itself pinned to the literal list transliteration and the KATs
(tests/test_oracle.py).
"""

import ctypes
import random

import numpy as np
import pytest

import histgen
import oracle_c
from kats import KATS
from qsmd import codec, device, gen, models
from qsmd.linearisability import linearisable, linearisable_batch, replay_witness

pytestmark = pytest.mark.gpu


def _compare(ctx, model_id, hdr, events, model0=None, max_nodes=0, threads=8, witness=True):
    st_d, nd_d, w_d, tot = ctx.check_arrays(model_id, hdr, events, model0, max_nodes=max_nodes,
                                            witness=witness)
    st_o, nd_o, w_o = oracle_c.check_batch(model_id, hdr, events, model0, max_nodes, threads,
                                           witness=witness)
    bad = np.nonzero((st_d != st_o) | (nd_d != nd_o))[0]
    assert len(bad) == 0, (f"{len(bad)} mismatches, first {bad[:5]}: "
                           f"dev {st_d[bad[:5]]}/{nd_d[bad[:5]]} oracle {st_o[bad[:5]]}/{nd_o[bad[:5]]}")
    if witness:
        lin = st_d == codec.STATUS_LIN
        for i in np.nonzero(lin)[0]:
            h = hdr[i]
            a, b = int(h["ev_off"]), int(h["ev_off"]) + int(h["n_ev"])
            assert np.array_equal(w_d[a:b], w_o[a:b]), f"witness mismatch at history {i}"
    assert tot["nodes"] == int(nd_d.sum())
    assert tot["linearisable"] == int((st_d == 1).sum())
    assert tot["nonlinearisable"] == int((st_d == 0).sum())
    assert tot["model_errors"] == int((st_d == 2).sum())
    assert tot["encode_errors"] == int((st_d == 3).sum())
    return st_d, nd_d, w_d


def test_kats_on_device(ctx):
    for name, (m, hist, status, nodes) in KATS.items():
        res = linearisable_batch(m, [hist], ctx=ctx, witness=True)
        assert res.verdict(0) == status, name
        assert int(res.nodes[0]) == nodes, name
        if status == "lin":
            assert replay_witness(m, hist, res.witness_of(0)), name


def test_timing_events():
    """Per-call timing events: off until qsmd_timing_reset (a lone caller
    does not pay three event packets a call), then stage 0 and the whole
    call per check call; knob timing_events 0 stops them again."""
    c = device.Context(0)
    try:
        hdr, ev, _ = gen.generate_config("bank_4x16", 1, 5000)
        c.check_arrays(models.MODEL_BANK, hdr, ev)
        with pytest.raises(device.DeviceError):
            c.last_kernel_ms()
        assert len(c.timing_read()[0]) == 0
        c.timing_reset()
        for _ in range(2):
            c.check_arrays(models.MODEL_BANK, hdr, ev)
        s0, call = c.timing_read()
        assert len(s0) == 2 and (s0 > 0).all() and (call >= s0).all()
        assert c.last_kernel_ms() > 0
        c.set_param("timing_events", 0)
        st, nd, _, _ = c.check_arrays(models.MODEL_BANK, hdr, ev)
        assert len(c.timing_read()[0]) == 2
        st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, None, 0, 8)
        assert (st == st_o).all() and (nd == nd_o).all()
    finally:
        c.close()


def test_automatic_stage0_budget():
    """The automatic stage-0 budget (the default until a budget is set): 24,
    16 after a call whose heavy list was short, back to 24 after one whose
    list was long.  Alternating config-2 batches (few heavy histories) and
    bug-laden config-3 batches (many) moves it both ways; each call's first
    heavy stage is then sized for the other budget's list (wave mode with a
    long list, lane mode with a short one).  Results stay the oracle's, and
    `stage0_budget_last` follows the hysteresis: config 2 at 24 sends < 1 in
    50 to the heavy stage (-> 16), config 3 at 16 > 1 in 5 (-> 24), config 2
    at 16 ~1 in 10 (stays)."""
    c = device.Context(0)
    try:
        batches = [(name, gen.generate_config(name, 9, 30000)) for name in ("bank_4x16", "bank_4x16_bugs")]
        used = []
        for name, (hdr, ev, _) in batches * 3 + batches[:1] * 2:
            _compare(c, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=10**7)
            used.append(c.get_param("stage0_budget_last"))
        assert used == [24, 16, 24, 16, 24, 16, 24, 16], used
    finally:
        c.close()


def test_wire_bytes_through_the_c_abi(ctx):
    """SchedulerHistory payload bytes (the reference's wire format, built by
    hand in tests/test_wire.py) -> qsmd.wire -> qsmd_check_batch: the KATs'
    verdicts and node counts."""
    from test_wire import KAT2_BYTES, KAT7_BYTES
    from qsmd import wire
    for payload, mid, kat in ((KAT2_BYTES, models.MODEL_TICKET, "KAT2_reference_example"),
                              (KAT7_BYTES, models.MODEL_BANK, "KAT7_bank_concurrent")):
        hdr, ev = wire.batch_arrays([payload] * 3, mid)
        st, nd, _, _ = ctx.check_arrays(mid, hdr, ev)
        _, _, status, nodes = KATS[kat]
        assert [codec.STATUS_NAMES[int(s)] for s in st] == [status] * 3 and list(nd) == [nodes] * 3


def test_linearisable_signature(ctx):
    """The reference signature: linearisable transition postcondition model0 history."""
    _, h2, _, _ = KATS["KAT2_reference_example"]
    _, h3, _, _ = KATS["KAT3_distinct_pids"]
    T = models.TICKET
    assert linearisable(T.transition, T.postcondition, T.init_model, h2, ctx=ctx) is False
    assert linearisable(T.transition, T.postcondition, T.init_model, h3, ctx=ctx) is True
    _, h8, _, _ = KATS["KAT8_bank_map_error"]
    B = models.BANK
    with pytest.raises(models.ModelError):
        linearisable(B.transition, B.postcondition, B.init_model, h8, ctx=ctx)
    with pytest.raises(NotImplementedError):
        linearisable(lambda m, e: m, lambda m, i, r: True, None, h3, ctx=ctx)


@pytest.mark.parametrize("model", ["ticket", "bank"])
def test_random_any_shape(ctx, model):
    """Ill-formed, shared-pid, pending and stray-response histories."""
    rng = random.Random(1234 if model == "ticket" else 4321)
    hs = []
    for _ in range(6000):
        if rng.random() < 0.5:
            hs.append(histgen.random_history(rng, model, rng.randint(0, 16), rng.randint(1, 5)))
        else:
            hs.append(histgen.wellformed_history(rng, model, rng.randint(0, 10), rng.randint(1, 5)))
    m = models.BY_NAME[model]
    b = codec.encode(m, hs)
    _compare(ctx, m.model_id, b.hdr, b.events, max_nodes=200000)


DEFAULTS = {"stage0_budget": 32, "memo_after": 32, "stage0_grid": 65536, "stage0w_budget": 32,
            "stage0w_budget_auto": 1, "heavy_mode": 2, "wave_max": 16384, "wave_min_rem": 4,
            "wave_grid": 0, "split_budget": 1024, "memo_lane_entries": 128, "memo_grid": 0, "split_xmemo": 1,
            "memo_lds": 1, "memo_lds_entries": 64, "dag_states": 128, "memo_lds_cap": 0, "fold": 1, "resume_cap": 0,
            "tail_cap": 256, "tail_min": 65536, "heavy_buckets": 1}


@pytest.fixture
def knobs(ctx):
    """Set tuning knobs for one test; every knob is restored afterwards."""
    def set_(**kw):
        for k, v in kw.items():
            ctx.set_param(k, v)
    yield set_
    for k, v in DEFAULTS.items():
        ctx.set_param(k, v)


@pytest.mark.parametrize("n_ev,n_pid", [(40, 3), (64, 6), (96, 4), (128, 8), (60, 20), (128, 100)])
@pytest.mark.parametrize("w_budget,heavy", [(32, 0), (4, 0), (4, 1), (0, 0)])
def test_stage_cascade(ctx, knobs, n_ev, n_pid, w_budget, heavy):
    """Histories beyond stage 0 (32 events / 8 pids) go through stage 0w
    (<= 64 events, <= 8 pids; over its node budget: the heavy stage, one
    wavefront or one lane per history) and the giant stage (everything
    else).  A 4-node budget sends most 0w histories to the heavy stage; 0
    = stage 0w searches them to the end."""
    rng = random.Random(n_ev * 1000 + n_pid)
    knobs(stage0w_budget=w_budget, heavy_mode=heavy)
    for model in ("ticket", "bank"):
        hs = [histgen.wellformed_history(rng, model, n_ev // 2, n_pid, p_pending=0.0)[:n_ev]
              for _ in range(300)]
        hs += [histgen.random_history(rng, model, n_ev, n_pid) for _ in range(300)]
        m = models.BY_NAME[model]
        b = codec.encode(m, hs)
        _compare(ctx, m.model_id, b.hdr, b.events, max_nodes=200000)


@pytest.mark.parametrize("model,n_ev", [("bank", 32), ("bank", 20), ("ticket", 24), ("ticket", 7),
                                        ("bank", 48), ("ticket", 64), ("bank", 33)])
def test_packed_uniform_batches(ctx, model, n_ev):
    """Batches whose histories are packed back to back with one length take the
    coalesced staging path; corrupt some events (encode errors) and widen some
    values (deferral beyond the compact stages) so every outcome goes through
    that path."""
    rng = random.Random(n_ev * 7 + len(model))
    m = models.BY_NAME[model]
    hs = []
    while len(hs) < 64 * 60:
        h = histgen.wellformed_history(rng, model, (n_ev + 1) // 2, rng.randint(1, 5), p_pending=0.0)
        if len(h) >= n_ev:
            hs.append(h[:n_ev])
    b = codec.encode(m, hs)
    ev = b.events.copy()
    nr = np.random.default_rng(n_ev)
    bad = nr.choice(len(ev), 40, replace=False)
    ev["code"][bad[:20]] = 9                                   # unknown constructor
    ev["val"][bad[20:]] = 1 << 20                              # > 19-bit: deferred
    for hdr in (b.hdr, b.hdr[1:]):                             # even and odd block start
        _compare(ctx, m.model_id, hdr, ev, max_nodes=200000)


def test_mixed_sizes_one_batch(ctx):
    rng = random.Random(7)
    hs = []
    for _ in range(3000):
        n = rng.choice([0, 1, 2, 8, 20, 32, 33, 50, 64, 65, 100, 128])
        hs.append(histgen.random_history(rng, "bank", n, rng.randint(1, 12)))
    b = codec.encode(models.BANK, hs)
    _compare(ctx, models.MODEL_BANK, b.hdr, b.events, max_nodes=100000)


@pytest.mark.parametrize("name,n", [("ticket_2x10", 20000), ("bank_4x16", 50000),
                                    ("bank_4x16_bugs", 50000), ("bank_6x24", 20000)])
@pytest.mark.parametrize("grid", [3, 77])
def test_stage0_grids(ctx, knobs, name, n, grid):
    """Stage 0 with fewer workgroups than groups (grid-stride: 3 workgroups
    take every group, 77 an uneven share each): the same results."""
    knobs(stage0_grid=grid)
    hdr, ev, _ = gen.generate_config(name, 3, n)
    _compare(ctx, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=10**7)


@pytest.mark.parametrize("name,n", [("ticket_2x10", 20000), ("bank_4x16", 50000),
                                    ("bank_4x16_bugs", 50000), ("bank_6x24", 20000)])
@pytest.mark.parametrize("budget", [0, 8, 32])
@pytest.mark.parametrize("heavy", [0, 1])
def test_generated_configs(ctx, knobs, name, n, budget, heavy):
    """The generated BASELINE configurations through the cascade: stage-0
    budget 0 (stage 0 searches everything), 8 (most histories go to the
    heavy stage) and 32 (the default); heavy stage in wave mode (one
    wavefront per history, LDS memo) and lane mode (one lane per history,
    HBM memo)."""
    knobs(stage0_budget=budget, stage0w_budget=budget, heavy_mode=heavy)
    hdr, ev, bug = gen.generate_config(name, 0, n)
    st, nd, _ = _compare(ctx, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=10**7)
    if name in ("bank_4x16", "bank_6x24"):
        assert (st == codec.STATUS_LIN).all()


@pytest.mark.parametrize("n", [1, 100, 64 * 16 * 3 + 17, 40000])
@pytest.mark.parametrize("heavy,grid", [(0, 65536), (1, 65536), (1, 3), (0, 77)])
def test_sharded_heavy_list(ctx, knobs, n, heavy, grid):
    """Stage 0's heavy list in 16 shards (a group appends to shard group %
    16; internal.h list_total / list_at): stage-0 budget 4 sends most
    histories there -- one group (a single shard), two, an uneven 3 x 16
    groups + 17 histories, 625 groups; grid-stride stage 0 (3 / 77
    workgroups); both heavy modes read the shards back as one list."""
    knobs(stage0_budget=4, heavy_mode=heavy, stage0_grid=grid)
    hdr, ev, _ = gen.generate_config("bank_4x16_bugs", 11, n)
    _compare(ctx, gen.CONFIGS["bank_4x16_bugs"]["model_id"], hdr, ev, max_nodes=10**7)


@pytest.mark.parametrize("name,n,budget,max_nodes", [("bank_4x16_bugs", 50000, 8, 0), ("bank_4x16", 50000, 4, 0),
                                                     ("bank_4x16_bugs", 20000, 8, 300), ("bank_6x24", 20000, 8, 0)])
@pytest.mark.parametrize("memo_after", [1, 24, 100, 1 << 40])
def test_lane_mode_memo_after(ctx, knobs, name, n, budget, max_nodes, memo_after):
    """Lane mode with the memo joining a search only after `memo_after`
    nodes (a short search runs as the plain DFS; 2^40: never): node counts,
    verdicts and witnesses stay the reference's (nodes entered before the
    memo joins are still recorded when they fail)."""
    knobs(heavy_mode=1, memo_lds=0, memo_after=memo_after, stage0_budget=budget, stage0w_budget=budget)
    hdr, ev, _ = gen.generate_config(name, 7, n)
    _compare(ctx, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=max_nodes or 10**7)


@pytest.mark.parametrize("bal", [28671, 28672, -28671, -28672, 200000])
@pytest.mark.parametrize("lds", [0, 2])
def test_lane_mode_key_range(ctx, knobs, bal, lds):
    """Lane mode keys a state's balances as i16; a 16-operation history moves
    an account by at most 16 x 256, so a model0 within +-28671 keeps every
    reachable state keyable and the memo runs, and one beyond it turns the
    memo off for the call (memo.hip keys_fit) -- exact either way: the
    reference's verdicts, node counts and witnesses on both sides of the
    bound, with HBM and LDS tables."""
    knobs(heavy_mode=1, memo_lds=lds, stage0_budget=8, stage0w_budget=8, memo_after=1)
    hdr, ev, _ = gen.generate_config("bank_4x16_bugs", 21, 20000)
    m0 = models.BankModel(0b1111, 0, (ctypes.c_int64 * 8)(bal, 7, -bal // 3, 0, 0, 0, 0, 0))
    _compare(ctx, models.MODEL_BANK, hdr, ev, m0, max_nodes=10**7)


LANE_CASES = [("bank_4x16_bugs", 50000, 64, 0),("bank_4x16_bugs", 20000, 8, 300), ("bank_4x16", 50000, 16, 0),
              ("ticket_2x10", 20000, 4, 0), ("bank_6x24", 20000, 16, 0), ("bank_6x24", 20000, 8, 500)]


@pytest.mark.parametrize("name,n,budget", [("bank_4x16", 60000, 12), ("bank_4x16_bugs", 20000, 20),
                                           ("bank_6x24", 20000, 12)])
def test_lane_mode_fold_consistent(ctx, knobs, name, n, budget):
    """Lane mode keeps the memo slot's balance fold in registers
    (LaneDFS::fold, updated by undo / try_next); the diagnostic build of the
    heavy stage (memo_stats_ptr) checks it against the balances in LDS after
    every try and counts the wavefront iterations where any lane's differs
    (stats word 12): 0, with the oracle's results."""
    torch = pytest.importorskip("torch")
    knobs(heavy_mode=1, memo_lds=0, memo_after=1, stage0_budget=budget, stage0w_budget=budget)
    hdr, ev, _ = gen.generate_config(name, 17, n)
    ctx.check_arrays(gen.CONFIGS[name]["model_id"], hdr, ev)   # (the launch's shape follows the last call's lists)
    groups = (n + 63) // 64
    stats = torch.zeros(groups * 16, dtype=torch.int64, device="cuda:0")
    ctx.set_param("memo_stats_groups", groups)
    ctx.set_param("memo_stats_ptr", stats.data_ptr())
    try:
        _compare(ctx, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=10**7)
        torch.cuda.synchronize()
    finally:
        ctx.set_param("memo_stats_ptr", 0)
    q = stats.view(groups, 16).cpu().numpy()
    q = q[q[:, 6] > 0]
    assert len(q) > 0 and int(q[:, 15].sum()) > 0        # the heavy stage ran, its iterations counted
    assert int(q[:, 12].sum()) == 0


@pytest.mark.parametrize("name,n,budget,max_nodes", LANE_CASES)
@pytest.mark.parametrize("entries", [128, 2])
@pytest.mark.parametrize("lds,lds_entries", [(0, 64), (2, 64), (2, 16), (2, 4)])
def test_lane_mode(ctx, knobs, name, n, budget, max_nodes, entries, lds, lds_entries):
    """Lane mode of the heavy stage (exact-count state memo in a private
    table per lane, in HBM or, lds=2, in LDS with 64 or 16 entries per
    lane): verdicts, node counts and witnesses must equal the reference's.
    2 entries: constant replacement; max_nodes: the budget falls inside
    reused subtrees."""
    knobs(heavy_mode=1, memo_lane_entries=entries, stage0_budget=budget, stage0w_budget=budget, memo_lds=lds,
          memo_lds_entries=lds_entries)
    hdr, ev, _ = gen.generate_config(name, 5, n)
    _compare(ctx, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=max_nodes or 10**7)


@pytest.mark.parametrize("cap", [1, 6, 40])
@pytest.mark.parametrize("name,n,budget", [("bank_4x16_bugs", 20000, 8), ("bank_4x16", 20000, 4),
                                           ("bank_6x24", 10000, 8), ("ticket_2x10", 20000, 4)])
def test_lane_mode_tail(ctx, knobs, name, n, budget, cap):
    """Lane mode's tail (api.hip tail_cap): the searches still running after
    `cap` wavefront iterations go to a wave-mode launch after the heavy
    stage and are searched there from the root (the state DAG, or the DFS
    when it does not fit); with max_nodes inside them, BUDGET.  The first
    call sets the heavy-count hint the tail needs (tail_min 0 here)."""
    knobs(heavy_mode=1, memo_lds=0, tail_cap=cap, tail_min=0, stage0_budget=budget, stage0w_budget=budget)
    hdr, ev, _ = gen.generate_config(name, 11, n)
    mid = gen.CONFIGS[name]["model_id"]
    for max_nodes in (10**7, 10**7, 60):
        _compare(ctx, mid, hdr, ev, max_nodes=max_nodes)
    assert ctx.get_param("tail_cap") == cap


@pytest.mark.parametrize("buckets,resume_cap", [(1, 0), (1, 3), (0, 0)])
@pytest.mark.parametrize("name,n,budget", [("bank_4x16_bugs", 30000, 12), ("bank_4x16", 30000, 4),
                                           ("ticket_2x10", 20000, 3)])
def test_heavy_buckets(ctx, knobs, name, n, budget, buckets, resume_cap):
    """The heavy stage's groups formed in order of predicted work (stage 0
    writes each heavy history's untried candidates on the stack, memo.hip's
    heavy_sort orders the list by them) against list order, with the saved
    states' slots cut to 3 per shard (the rest start at the root), lane
    mode, no tail; three calls, the first setting the heavy-count hint the
    ordering needs (tail_min 0)."""
    knobs(heavy_mode=1, memo_lds=0, tail_cap=0, tail_min=0, heavy_buckets=buckets, resume_cap=resume_cap,
          stage0_budget=budget, stage0w_budget=budget)
    hdr, ev, _ = gen.generate_config(name, 13, n)
    mid = gen.CONFIGS[name]["model_id"]
    for max_nodes in (10**7, 10**7, 80):
        _compare(ctx, mid, hdr, ev, max_nodes=max_nodes)


@pytest.mark.parametrize("name,n,budget,max_nodes", LANE_CASES)
@pytest.mark.parametrize("min_rem,grid,dag", [(4, 0, 128), (4, 0, 0), (0, 0, 0), (64, 0, 0), (0, 7, 0),
                                              (4, 7, 128), (4, 0, 6), (4, 0, 24),
                                              (4, 0, 4095)])  # (4095: cut to the LDS)
def test_wave_mode(ctx, knobs, name, n, budget, max_nodes, min_rem, grid, dag):
    """Wave mode of the heavy stage (csrc/wave.hip): one wavefront per
    history; the state DAG (dag: its capacity in states; 0 = off, 6 / 24 =
    many histories overflow it mid-build and run the DFS) or the DFS in
    wave-uniform registers with the exact-count memo in an 8-way LDS table
    per wavefront.  min_rem: memo only above this many remaining events (64:
    no memo at all, 0: at every node); grid 7: few wavefronts, many
    histories each (grid-stride, entry tags per history); max_nodes falls
    inside reused subtrees / below the DAG's exact count."""
    knobs(heavy_mode=0, wave_min_rem=min_rem, wave_grid=grid, stage0_budget=budget, stage0w_budget=budget,
          dag_states=dag)
    hdr, ev, _ = gen.generate_config(name, 6, n)
    _compare(ctx, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=max_nodes or 10**7)


@pytest.mark.parametrize("memo_lds", [1, 2])
def test_lds_tables_refused_run_hbm_tables(ctx, knobs, memo_lds):
    """Lane mode asks for LDS memo tables (memo_lds 2: always; 1: the short
    heavy list of a config-2 batch at the library's budget) and the device
    refuses the size (memo_lds_cap below it, the diagnostic knob): the call
    runs the HBM tables it then allocates.  Fresh memo_grid, so no table
    from an earlier test is there to be reused."""
    knobs(heavy_mode=1, memo_lds=memo_lds, memo_grid=37, memo_lds_cap=1024, stage0_budget=16)
    hdr, ev, _ = gen.generate_config("bank_4x16", 9, 50000)
    for _ in range(2):                    # (the second call: the hint-sized grid)
        st, _, _ = _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**7)
    assert (st == codec.STATUS_LIN).all()
    hdr, ev, _ = gen.generate_config("bank_4x16_bugs", 9, 50000)
    _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**7)


def test_lane_tables_too_large_fall_back_to_wave_mode(ctx, knobs):
    """Lane-mode tables the device cannot hold send the call to wave mode:
    the same results."""
    knobs(heavy_mode=1, memo_grid=65536, memo_lane_entries=65536, stage0_budget=8)
    hdr, ev, _ = gen.generate_config("bank_4x16_bugs", 21, 20000)
    for _ in range(2):
        _compare(ctx, models.MODEL_BANK, hdr, ev)


@pytest.mark.parametrize("split_budget", [1, 16, 200])
@pytest.mark.parametrize("heavy", [0, 1])
def test_heavy_handoff_to_giants(ctx, knobs, split_budget, heavy):
    """Heavy-stage searches past their cap (64 x split budget iterations) go
    to the giant stage and are searched there again from the root (whole,
    or cut into tasks after 16 x split budget iterations)."""
    knobs(split_budget=split_budget, heavy_mode=heavy, stage0_budget=4, stage0w_budget=4)
    for name, n in (("bank_4x16_bugs", 30000), ("ticket_2x10", 20000), ("bank_6x24", 5000)):
        hdr, ev, _ = gen.generate_config(name, 9, n)
        _compare(ctx, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=10**7)


@pytest.mark.parametrize("heavy,w_budget,split", [(0, 4, 64), (1, 4, 64), (0, 1, 1024), (1, 1, 1024),
                                                  (0, 0, 1024), (0, 4, 1)])
def test_model_error_in_the_heavy_stage(ctx, knobs, heavy, w_budget, split):
    """A 33-event unpaired Bank history that ends in Map.! after 7 nodes
    (found by tools/stress_parity.py --seed 11 --knobs, batch 219), through
    stage 0w's budget into both heavy-stage modes: the count stops at the
    raising node."""
    import os
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", "wave_model_error_case.npz"))
    hdr, ev, mid = f["hdr"], f["ev"], int(f["model_id"])
    knobs(heavy_mode=heavy, stage0_budget=4, stage0w_budget=w_budget, split_budget=split)
    st, nd, _ = _compare(ctx, mid, np.repeat(hdr, 3), ev, max_nodes=200000)
    assert (st == int(f["status"])).all() and (nd == int(f["nodes"])).all()


def test_tail_grids_follow_the_previous_call(ctx, knobs):
    """The tail launches are sized from the previous call's list sizes: a
    call with no <= 64-event heavy histories, then one with many (lane mode
    without room for them sends them to the giant stage), then a giant-free
    call after a giant one -- every result the reference's."""
    knobs(heavy_mode=1, stage0w_budget=4)
    for name, first, n in (("bank_4x16", 0, 20000), ("bank_6x24", 3, 5000), ("bank_6x24", 4, 5000),
                           ("bank_4x16_bugs", 7, 20000)):
        hdr, ev, _ = gen.generate_config(name, first, n)
        _compare(ctx, gen.CONFIGS[name]["model_id"], hdr, ev, max_nodes=10**7)
    rng = random.Random(5)
    hs = [histgen.wellformed_history(rng, "bank", 50, 3, p_pending=0.0) for _ in range(200)]   # 100 events: giants
    b = codec.encode(models.BANK, hs)
    _compare(ctx, models.MODEL_BANK, b.hdr, b.events, max_nodes=10**7)
    hdr, ev, _ = gen.generate_config("bank_4x16", 9, 20000)
    _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**7)


@pytest.mark.parametrize("model", ["ticket", "bank"])
@pytest.mark.parametrize("heavy,dag", [(0, 128), (0, 0), (1, 128)])
def test_heavy_any_shape(ctx, knobs, model, heavy, dag):
    """Unpaired, shared-pid, pending and stray-response histories (the
    general DFS mode), Map.! errors, node budgets and a non-default model0
    through the heavy stage (wave mode: the state DAG, or the DFS)."""
    rng = random.Random(77 if model == "ticket" else 78)
    hs = []
    for _ in range(4000):
        if rng.random() < 0.5:
            hs.append(histgen.random_history(rng, model, rng.randint(8, 32), rng.randint(1, 5)))
        else:
            hs.append(histgen.wellformed_history(rng, model, rng.randint(6, 16), rng.randint(1, 5)))
    m = models.BY_NAME[model]
    knobs(heavy_mode=heavy, stage0_budget=4, wave_min_rem=0, dag_states=dag)
    b = codec.encode(m, hs)
    for max_nodes in (0, 50, 3000):
        _compare(ctx, m.model_id, b.hdr, b.events, max_nodes=max_nodes)
    if model == "ticket":
        _compare(ctx, m.model_id, b.hdr, b.events, models.TicketModel(1, 0, 3), max_nodes=200000)


@pytest.mark.parametrize("wave_max", [1000, 16384])
def test_heavy_mode_auto_switches(ctx, knobs, wave_max):
    """heavy_mode 2 (the default) picks wave or lane mode from the routing of
    the last finished call (lane mode past wave_max heavy histories, or for
    a list under a fifth of the batch; wave mode for a short bug-laden
    list); results are exact whichever it picks and across the switches
    (bug-heavy batch, a clean one, the bug-heavy again, a small clean one,
    one with wide histories)."""
    knobs(heavy_mode=2, wave_max=wave_max)
    b3 = gen.generate_config("bank_4x16_bugs", 11, 30000)
    b2 = gen.generate_config("bank_4x16", 11, 30000)
    b2s = gen.generate_config("bank_4x16", 12, 300)
    b5 = gen.generate_config("bank_6x24", 11, 3000)
    for hdr, ev, _ in (b3, b3, b3, b2, b2, b3, b2s, b2s, b5, b2, b5):
        _compare(ctx, models.MODEL_BANK, hdr, ev)


def test_probe_routing(ctx, knobs):
    """qsmd_probe_read: how the last call routed its histories."""
    knobs(stage0_budget=32)
    hdr, ev, _ = gen.generate_config("bank_4x16", 0, 20000)
    st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, threads=8)
    ctx.check_arrays(models.MODEL_BANK, hdr, ev)
    pr = ctx.probe()
    assert pr["heavy32"] == int((nd_o > 32).sum()) and pr["deferred"] == 0 and pr["giants"] == 0


def test_concurrent_contexts_on_streams(ctx):
    """bench.py keeps several calls in flight: one context and stream each,
    running at the same time on one GPU.  Every call's results must be the
    oracle's (contexts share no device state)."""
    torch = pytest.importorskip("torch")
    from qsmd import device
    dev = torch.device("cuda:0")
    batches = [gen.generate_config(name, 31, n) for name, n in
               (("bank_4x16_bugs", 20000), ("bank_4x16", 40000), ("bank_6x24", 8000))]
    ctxs = [ctx, device.Context(0), device.Context(0)]
    streams = [torch.cuda.Stream(dev) for _ in ctxs]
    try:
        bufs = []
        for (hdr, ev, _), c, s in zip(batches, ctxs, streams):
            n = len(hdr)
            b = (torch.from_numpy(hdr.view(np.uint8)).to(dev), torch.from_numpy(ev.view(np.uint8)).to(dev),
                 torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev))
            bufs.append(b)
        torch.cuda.synchronize()
        for _ in range(3):
            for (hdr, ev, _), c, s, b in zip(batches, ctxs, streams, bufs):
                c.check_device(models.MODEL_BANK, b[0].data_ptr(), len(hdr), b[1].data_ptr(), len(ev),
                               b[2].data_ptr(), b[3].data_ptr(), None, None, stream=s.cuda_stream)
        torch.cuda.synchronize()
        for (hdr, ev, _), b in zip(batches, bufs):
            st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, None, 0, 8, witness=False)
            assert np.array_equal(b[2].cpu().numpy(), st_o)
            assert np.array_equal(b[3].cpu().numpy().astype(np.uint64), nd_o.astype(np.uint64))
    finally:
        for c in ctxs[1:]:
            c.close()


def test_one_context_two_streams(ctx):
    """Calls of ONE context enqueued back to back on two different streams:
    the library orders them (they share the context's workspace), so every
    call's results are the oracle's."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    batches = [gen.generate_config(name, 41, n) for name, n in (("bank_4x16_bugs", 20000), ("bank_4x16", 40000))]
    streams = [torch.cuda.Stream(dev) for _ in batches]
    bufs = []
    for hdr, ev, _ in batches:
        n = len(hdr)
        bufs.append((torch.from_numpy(hdr.view(np.uint8)).to(dev), torch.from_numpy(ev.view(np.uint8)).to(dev),
                     torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                     torch.zeros(8, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    for _ in range(4):
        for (hdr, ev, _), s, b in zip(batches, streams, bufs):
            ctx.check_device(models.MODEL_BANK, b[0].data_ptr(), len(hdr), b[1].data_ptr(), len(ev),
                             b[2].data_ptr(), b[3].data_ptr(), None, b[4].data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for (hdr, ev, _), b in zip(batches, bufs):
        st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, None, 0, 8, witness=False)
        assert np.array_equal(b[2].cpu().numpy(), st_o)
        assert np.array_equal(b[3].cpu().numpy().astype(np.uint64), nd_o.astype(np.uint64))
        tot = b[4].cpu().numpy()
        assert int(tot[7]) == int(nd_o.astype(np.int64).sum()) and int(tot[0]) == len(hdr)


def test_model0(ctx):
    rng = random.Random(99)
    hs = [histgen.wellformed_history(rng, "ticket", rng.randint(1, 6), 2) for _ in range(2000)]
    b = codec.encode(models.TICKET, hs)
    for n0 in (0, 5, -3):
        _compare(ctx, models.MODEL_TICKET, b.hdr, b.events, models.TicketModel(1, 0, n0))
    accts = ["p0", "p1", "p2"]
    model0 = {"p0": 10, "p1": 0, "p2": 3}
    hs = [histgen.wellformed_history(rng, "bank", rng.randint(1, 6), 3) for _ in range(2000)]
    b = codec.encode(models.BANK, hs, model0)
    packed = models.BANK.pack_model0(model0, models.BANK.new_account_map(model0))
    assert packed.exists == 0b111 and list(packed.balance)[:3] == [10, 0, 3]
    _compare(ctx, models.MODEL_BANK, b.hdr, b.events, packed)
    del accts


def test_budget(ctx, knobs):
    """The caller's max_nodes through every stage: stage-0 budgets 0 / 5 / 50
    (the heavy stage in wave and lane mode), stage-0w budgets 0 / 4 / 256,
    and the giant stage (a 1-node split budget)."""
    rng = random.Random(5)
    for n_ev in (40, 24):
        hs = [histgen.random_history(rng, "ticket", n_ev, 1) for _ in range(500)]
        b = codec.encode(models.TICKET, hs)
        for stage0, w_budget, heavy, split in ((0, 0, 0, 1024), (5, 0, 0, 1024), (50, 0, 1, 1024),
                                               (0, 4, 0, 1024), (0, 4, 1, 1024), (0, 256, 0, 1024),
                                               (5, 4, 0, 1)):
            knobs(stage0_budget=stage0, stage0w_budget=w_budget, heavy_mode=heavy, split_budget=split)
            for budget in (1, 7, 100, 1000):
                st, nd, _ = _compare(ctx, models.MODEL_TICKET, b.hdr, b.events, max_nodes=budget)
                assert (nd <= budget).all()


@pytest.mark.parametrize("name,shift", [("bank_4x16_bugs", 0), ("bank_4x16_bugs", 3000),
                                        ("bank_6x24", 0), ("bank_4x16", 0)])
def test_early_exit_batch(ctx, knobs, name, shift):
    """QSMD_FLAG_EARLY_EXIT_BATCH: like QuickCheck stopping at the first
    failing test, everything after the first non-linearisable (or raising)
    history is SKIPPED; everything up to it is exactly the full result."""
    from qsmd import device
    hdr, ev, _ = gen.generate_config(name, shift, 8000)
    mid = gen.CONFIGS[name]["model_id"]
    if name == "bank_6x24":                      # plant one failure deep in the batch
        ev = ev.copy()
        k = int(hdr[5000]["ev_off"]) + 47
        ev["val"][k] += 1 if ev["code"][k] == 7 else 0
        ev["code"][k] = 7 if ev["code"][k] != 7 else 7
    st_o, nd_o, _ = oracle_c.check_batch(mid, hdr, ev, threads=8, max_nodes=10**7)
    fails = np.nonzero((st_o == 0) | (st_o == 2))[0]
    cut = int(fails[0]) if len(fails) else len(hdr)
    knobs(stage0_budget=32 if shift else 0)
    st, nd, _, tot = ctx.check_arrays(mid, hdr, ev, flags=device.QSMD_FLAG_EXHAUSTIVE |
                                      device.QSMD_FLAG_EARLY_EXIT_BATCH, max_nodes=10**7)
    assert np.array_equal(st[:cut + 1], st_o[:cut + 1]) and np.array_equal(nd[:cut + 1], nd_o[:cut + 1])
    assert (st[cut + 1:] == codec.STATUS_SKIPPED).all() and (nd[cut + 1:] == 0).all()
    assert tot["skipped"] == max(0, len(hdr) - cut - 1)
    assert tot["nodes"] == int(nd_o[:cut + 1].sum())
    assert tot["checked"] == int(((st_o[:cut + 1] <= 2)).sum())


def test_early_exit_fixup_chunks(ctx, knobs):
    """The early-exit fixup runs in 512-history chunks, one workgroup each
    (a grid sized by them when the last call had no giants, 2 per CU when it
    had): a failure planted before, at and after chunk boundaries, at the
    batch's ends, and none, in a row of calls whose giant hint flips (a
    split knob that makes giants of the heavy histories, then none).
    Everything up to the failure is the oracle's, everything after it
    SKIPPED with 0 nodes, and the totals count exactly that."""
    from test_distributed import planted_stream
    from qsmd import device
    n = 5000
    for plant, split in [(None, 0), (511, 0), (512, 0), (513, 0), (0, 0), (n - 1, 0), (1023, 2), (4100, 2),
                         (2047, 0), (None, 2), (3000, 0)]:
        hdr, ev = planted_stream("bank_4x16", n, plant)
        st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, threads=8, max_nodes=10**7)
        fails = np.nonzero((st_o == 0) | (st_o == 2))[0]
        cut = int(fails[0]) if len(fails) else n
        knobs(split_budget=split if split else 1024, stage0_budget=8)
        st, nd, _, tot = ctx.check_arrays(models.MODEL_BANK, hdr, ev, max_nodes=10**7,
                                          flags=device.QSMD_FLAG_EXHAUSTIVE | device.QSMD_FLAG_EARLY_EXIT_BATCH)
        assert np.array_equal(st[:cut + 1], st_o[:cut + 1]), plant
        assert np.array_equal(nd[:cut + 1], nd_o[:cut + 1]), plant
        assert (st[cut + 1:] == codec.STATUS_SKIPPED).all() and (nd[cut + 1:] == 0).all(), plant
        assert tot["skipped"] == max(0, n - cut - 1), plant
        assert tot["nodes"] == int(nd_o[:cut + 1].sum()), plant
        assert tot["checked"] == int((st_o[:cut + 1] <= 2).sum()), plant


def test_encode_errors(ctx):
    hdr = np.zeros(5, dtype=codec.HDR_DTYPE)
    ev = np.zeros(8, dtype=codec.EV_DTYPE)
    hdr[0] = (0, 2, 1, 0xFF, 0, 0)            # wrong model
    hdr[1] = (0, 2, 0, 2, 0, 0)               # pid >= n_pid
    hdr[2] = (0, 200, 1, 2, 0, 0)             # too many events / beyond buffer
    hdr[3] = (6, 2, 1, 2, 0, 0)               # ok shape; bad code below
    hdr[4] = (4, 2, 1, 2, 0, 0)               # valid: Open a / Created
    ev[4] = (0, 0, 0, 0, 0)
    ev[5] = (0x80, 0, 0, 0, 0)
    ev[6] = (0, 9, 0, 0, 0)                   # unknown Bank request
    ev[7] = (0x80, 0, 0, 0, 0)
    st, nd, _, tot = ctx.check_arrays(models.MODEL_BANK, hdr, ev)
    assert list(st) == [3, 3, 3, 3, 1]
    assert tot["encode_errors"] == 4


@pytest.mark.parametrize("model", ["bank", "ticket"])
def test_host_entry_wide_only_bad_headers(ctx, knobs, model):
    """A host-entry batch with no history of <= 64 events skips the compact
    stages (the wave kernel's M128 launch takes the batch unlisted), so no
    compact stage validates the headers there: a wrong model_id and event
    ranges outside the batch must still be ENCODE_ERROR (nodes 0), never
    searched or read, and every other history the oracle's result."""
    knobs(heavy_mode=2)
    rng = random.Random(77 if model == "bank" else 78)
    m = models.BY_NAME[model]
    hs = [histgen.wellformed_history(rng, model, rng.randint(33, 64), rng.randint(2, 8), p_pending=0.0)
          for _ in range(48)]
    b = codec.encode(m, hs)
    hdr = b.hdr.copy()
    assert (hdr["n_ev"] > 64).all()
    other = models.MODEL_TICKET if m.model_id == models.MODEL_BANK else models.MODEL_BANK
    hdr["model_id"][3] = other                         # wrong model
    hdr["ev_off"][7] = len(b.events) - 10              # runs past the batch's events
    hdr["ev_off"][11] = 0x7FFFFFF0                     # far outside
    bad = [3, 7, 11]
    st, nd, _, tot = ctx.check_arrays(m.model_id, hdr, b.events, max_nodes=200000)
    assert (st[bad] == codec.STATUS_ENCODE_ERROR).all() and (nd[bad] == 0).all()
    good = np.setdiff1d(np.arange(len(hdr)), bad)
    st_o, nd_o, _ = oracle_c.check_batch(m.model_id, b.hdr, b.events, max_nodes=200000, threads=8)
    assert np.array_equal(st[good], st_o[good]) and np.array_equal(nd[good], nd_o[good])
    assert tot["encode_errors"] == len(bad)


# BASELINE.json configs at their single-GPU sizes: config 1 (TicketDispenser
# 2 x 10), config 2 (Bank 4 x 16, 1M: the headline), config 3 (Bank with
# injected bugs: 10M over 8 GPUs, i.e. 1.25M per GPU; 1M here), config 5
# (Bank 6 x 24, 100k, exhaustive).  Config 4 (one adversarial history) is
# tests/test_gpu_split.py::test_adversarial_ticket_memo.
FULL_SIZE = [("ticket_2x10", 1_000_000), ("bank_4x16", 1_000_000), ("bank_4x16_bugs", 1_000_000),
             ("bank_6x24", 100_000)]


@pytest.mark.parametrize("name,n", FULL_SIZE)
def test_device_resident_full_size(ctx, name, n):
    """Every generated BASELINE config at full single-GPU size through the
    device entry point (inputs resident in HBM, as bench.py runs them): the
    oracle's verdict and node count for every history, the witness of every
    linearisable one, and the totals; plus the size-independent properties
    (Bank without bugs: all linearisable by construction)."""
    torch = pytest.importorskip("torch")
    mid = gen.CONFIGS[name]["model_id"]
    hdr, ev, bug = gen.generate_config(name, 0, n)
    dev = torch.device("cuda:0")
    d_hdr = torch.from_numpy(hdr.view(np.uint8)).to(dev)
    d_ev = torch.from_numpy(ev.view(np.uint8)).to(dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nd = torch.empty(n, dtype=torch.int64, device=dev)
    d_w = torch.full((len(ev),), 0xFF, dtype=torch.uint8, device=dev)
    d_tot = torch.zeros(8, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.check_device(mid, d_hdr.data_ptr(), n, d_ev.data_ptr(), len(ev), d_st.data_ptr(), d_nd.data_ptr(),
                     d_w.data_ptr(), d_tot.data_ptr(), flags=device.QSMD_FLAG_EXHAUSTIVE | device.QSMD_FLAG_WITNESS,
                     max_nodes=10**7, stream=stream)
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()
    nd = d_nd.cpu().numpy().astype(np.uint64)
    w = d_w.cpu().numpy()
    tot = d_tot.cpu().numpy()
    st_o, nd_o, w_o = oracle_c.check_batch(mid, hdr, ev, max_nodes=10**7, threads=16, witness=True)
    bad = np.nonzero((st != st_o) | (nd != nd_o))[0]
    assert len(bad) == 0, f"{len(bad)} mismatches, first {bad[:5]}: dev {st[bad[:5]]}/{nd[bad[:5]]} " \
                          f"oracle {st_o[bad[:5]]}/{nd_o[bad[:5]]}"
    lin = st == codec.STATUS_LIN
    n_ev = hdr["n_ev"].astype(np.int64)
    assert hdr["ev_off"][0] == 0 and np.array_equal(np.cumsum(n_ev)[:-1], hdr["ev_off"][1:].astype(np.int64))
    mask = np.repeat(lin, n_ev)                                # the events of linearisable histories
    assert np.array_equal(w[mask], w_o[mask]), "witness mismatch"
    assert int(tot[0]) == int((st <= 2).sum()) and int(tot[1]) == int(lin.sum())
    assert int(tot[2]) == int((st == 0).sum()) and int(tot[7]) == int(nd.sum())
    if name in ("bank_4x16", "bank_6x24"):
        assert lin.all()
    if name == "bank_4x16_bugs":
        assert (st == codec.STATUS_NONLIN).sum() > n // 10   # the early-termination path is exercised


@pytest.mark.parametrize("name,n", [("bank_4x16", 1_000_000), ("bank_4x16_bugs", 1_250_000)])
def test_bench_knobs_in_flight_full_size(name, n):
    """bench.py's own knob set at full size: stage-0 budget 20, the heavy
    stage in lane mode with HBM memo tables (heavy_mode 1, memo_lds 0), four
    contexts on four streams with calls in flight, five distinct resident
    batches in rotation (step k checks batch k % 5 on slot k % 4, so every
    context's tail grids and lane tables come from another batch's call), on
    config 2 (1M per batch) and on config 3's per-GPU share of 10M over 8 GPUs
    (1.25M): every status and node count of every call equals the oracle's
    (the reference's test/Bank.hs:256-287 checks one history per call)."""
    torch = pytest.importorskip("torch")
    S, K, steps = 4, 5, 10
    mid = gen.CONFIGS[name]["model_id"]
    dev = torch.device("cuda:0")
    host, batches = [], []
    for k in range(K):
        hdr, ev, _ = gen.generate(gen.params(**gen.CONFIGS[name]), k * n, n, threads=16)
        host.append((hdr, ev))
        batches.append((torch.from_numpy(hdr.view(np.uint8)).to(dev), torch.from_numpy(ev.view(np.uint8)).to(dev),
                        len(ev)))
    ctxs = [device.Context(0, time_limit_ms=60000) for _ in range(S)]
    streams = [torch.cuda.Stream(dev) for _ in range(S)]
    outs = [(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
             torch.zeros(8, dtype=torch.int64, device=dev)) for _ in range(steps)]
    torch.cuda.synchronize()
    try:
        for c in ctxs:
            c.set_stage0_budget(20)
            c.set_param("heavy_mode", 1)
            c.set_param("memo_lds", 0)
        for k in range(steps):
            i = k % S
            d_hdr, d_ev, n_ev = batches[k % K]
            d_st, d_nd, d_tot = outs[k]
            with torch.cuda.stream(streams[i]):
                d_st.fill_(0xEE)
                ctxs[i].check_device(mid, d_hdr.data_ptr(), n, d_ev.data_ptr(), n_ev, d_st.data_ptr(),
                                     d_nd.data_ptr(), None, d_tot.data_ptr(), flags=device.QSMD_FLAG_EXHAUSTIVE,
                                     stream=streams[i].cuda_stream)
        torch.cuda.synchronize()
        results = [(o[0].cpu().numpy(), o[1].cpu().numpy().astype(np.uint64), o[2].cpu().numpy()) for o in outs]
    finally:
        for c in ctxs:
            c.close()
    oracle = [oracle_c.check_batch(mid, hdr, ev, threads=16)[:2] for hdr, ev in host]
    for k, (st, nd, tot) in enumerate(results):
        st_o, nd_o = oracle[k % K]
        bad = np.nonzero((st != st_o) | (nd != nd_o))[0]
        assert len(bad) == 0, f"step {k}: {len(bad)} mismatches, first {bad[:5]}"
        assert int(tot[0]) == int((st <= 2).sum()) and int(tot[7]) == int(nd.sum())
    if name == "bank_4x16":
        assert all((o[0] == codec.STATUS_LIN).all() for o in oracle)


@pytest.mark.parametrize("packed", [True, False])
def test_value_ranges_and_pairing(ctx, packed):
    """Stage 0 holds invocation values within 9-bit signed (-256..255) and
    response values within 25-bit signed (lane.h IVAL_BITS / RVAL_BITS);
    anything wider goes on to the next stage.  Put values on both sides of
    both bounds into generated Bank histories (packed uniform batch and a
    non-uniform one), and mix paired (every pid alternates) with unpaired
    histories inside one wavefront."""
    hdr, ev, _ = gen.generate_config("bank_4x16_bugs", 7, 64 * 40)
    ev = ev.copy()
    nr = np.random.default_rng(11)
    inv = np.nonzero((ev["kp"] & 0x80) == 0)[0]
    rsp = np.nonzero(((ev["kp"] & 0x80) != 0) & (ev["code"] == 7))[0]        # Balance responses
    iv = np.array([255, 256, -256, -257, 8191, 8192, -8192, -8193, 1 << 20, -(1 << 30)], dtype=np.int32)
    rv = np.array([(1 << 24) - 1, 1 << 24, -(1 << 24), -(1 << 24) - 1, 1 << 30], dtype=np.int32)
    ki = nr.choice(inv, 300, replace=False)
    kr = nr.choice(rsp, 300, replace=False)
    ev["val"][ki] = iv[nr.integers(0, len(iv), len(ki))]
    ev["val"][kr] = rv[nr.integers(0, len(rv), len(kr))]
    # unpaired: give a few histories a second invocation of the same pid
    # before its response (and a stray response) by swapping two events
    for h in nr.choice(len(hdr), 200, replace=False):
        o = int(hdr[h]["ev_off"])
        i = o + int(nr.integers(4, 30))
        ev[[i, i + 1]] = ev[[i + 1, i]]
    if not packed:
        hdr = hdr[nr.permutation(len(hdr))]
    _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**6)


def _concat(*batches):
    """One batch of several (hdr, events) batches, headers rebased."""
    hs, es, off = [], [], 0
    for hdr, ev in batches:
        h = hdr.copy()
        h["ev_off"] += off
        hs.append(h)
        es.append(ev)
        off += len(ev)
    return np.concatenate(hs), np.concatenate(es)


@pytest.mark.parametrize("fold", [0, 1])
def test_fold_stage0w(ctx, knobs, fold):
    """Lane mode's folded tail (knob fold 1, the default): after a call that
    deferred nothing to stage 0w, the next launches no stage 0w -- what stage
    0 defers then goes on to the giant stage.  A call stream whose deferred
    count changes under it (clean 4x16 batches, then a batch mixing in 6x24
    histories and wider ones, then clean again) stays the oracle's, and the
    probe still counts what stage 0 deferred."""
    knobs(heavy_mode=1, memo_lds=0, stage0_budget=16, fold=fold)
    b2 = gen.generate_config("bank_4x16", 21, 20000)[:2]
    b5 = gen.generate_config("bank_6x24", 21, 3000)[:2]
    rng = random.Random(8)
    wide = codec.encode(models.BANK, [histgen.wellformed_history(rng, "bank", rng.randint(33, 60), rng.randint(2, 8),
                                                                 p_pending=0.0) for _ in range(200)])
    mixed = _concat(b2, b5, (wide.hdr, wide.events))
    for hdr, ev in (b2, b2, mixed, b2, mixed, mixed, b2):
        _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**7)
        assert ctx.probe()["deferred"] == (3200 if len(hdr) > 20000 else 0)


@pytest.mark.parametrize("cap", [1, 7, 64])
def test_resume_cap(ctx, knobs, cap):
    """Lane mode's saved stage-0 states are capped per heavy-list shard
    (knob resume_cap; by default from the last call's heavy count): a heavy
    history past its shard's slots starts again at the root.  Exact either
    way, on the bug-laden batch with many heavy histories and a clean one."""
    knobs(heavy_mode=1, memo_lds=0, stage0_budget=8, resume_cap=cap)
    for name in ("bank_4x16_bugs", "bank_4x16"):
        hdr, ev, _ = gen.generate_config(name, 5, 20000)
        _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**7)


def test_host_waits_stay_with_the_context():
    """A context's host waits (qsmd_probe_read here) wait for that context's
    last call only -- its completion event or its one stream -- not for the
    device: context A's giant stage (one workgroup) is held back half a
    second (the giant_stall_us diagnostic) on stream sA while context B, on stream sB,
    finishes a call and reads its probe; sA is still busy when that returns.
    Both calls' results are the oracle's."""
    torch = pytest.importorskip("torch")
    import time
    dev = torch.device("cuda:0")
    rng = random.Random(31)
    ga = codec.encode(models.BANK, [histgen.wellformed_history(rng, "bank", 30, 12, p_pending=0.0)
                                    for _ in range(8)])                    # > 8 pids: the giant stage
    hb, eb, _ = gen.generate_config("bank_4x16", 3, 5000)
    A, B = device.Context(0), device.Context(0)
    sA, sB = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    try:
        A.set_param("giant_stall_us", 500000)
        A.set_param("giant_grid", 1)              # (A's stalled giant stage holds one CU, not the GPU)
        bufs = []
        for hdr, ev in ((ga.hdr, ga.events), (hb, eb)):
            n = len(hdr)
            bufs.append((torch.from_numpy(hdr.view(np.uint8)).to(dev), torch.from_numpy(ev.view(np.uint8)).to(dev),
                         torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)))
        torch.cuda.synchronize()
        (ha, ea, sta, nda), (hbd, ebd, stb, ndb) = bufs
        A.check_device(models.MODEL_BANK, ha.data_ptr(), len(ga.hdr), ea.data_ptr(), len(ga.events), sta.data_ptr(),
                       nda.data_ptr(), None, None, max_nodes=10**6, stream=sA.cuda_stream)
        t0 = time.perf_counter()
        B.check_device(models.MODEL_BANK, hbd.data_ptr(), len(hb), ebd.data_ptr(), len(eb), stb.data_ptr(),
                       ndb.data_ptr(), None, None, max_nodes=10**6, stream=sB.cuda_stream)
        B.probe()                                   # waits for B's call only
        waited = time.perf_counter() - t0
        busy = not sA.query()
        torch.cuda.synchronize()
        assert busy and waited < 0.4, (busy, waited)
        for (hdr, ev), st, nd in (((ga.hdr, ga.events), sta, nda), ((hb, eb), stb, ndb)):
            st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, None, 10**6, 8)
            assert np.array_equal(st.cpu().numpy(), st_o)
            assert np.array_equal(nd.cpu().numpy().astype(np.uint64), nd_o.astype(np.uint64))
    finally:
        A.close()
        B.close()


def test_caller_streams_destroyed_between_calls():
    """A plain HIP caller's lifetime pattern: create a stream, make a device
    call on it, synchronise it, destroy it -- then the next call on a new
    stream, a host wait of the context (qsmd_probe_read), qsmd_close.  The
    context waits on its completion event (ABI 3), never on the
    destroyed stream handle.  Results equal the oracle's."""
    torch = pytest.importorskip("torch")
    import ctypes
    dev = torch.device("cuda:0")
    hip = ctypes.CDLL("libamdhip64.so.7")     # (the runtime torch and libqsmd.so already share)
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    hdr, ev, _ = gen.generate_config("bank_4x16_bugs", 5, 20000)
    n = len(hdr)
    d_hdr = torch.from_numpy(hdr.view(np.uint8)).to(dev)
    d_ev = torch.from_numpy(ev.view(np.uint8)).to(dev)
    outs = [(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev))
            for _ in range(3)]
    torch.cuda.synchronize()
    st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, None, 10**7, 8)
    A = device.Context(0)
    try:
        for k, (st, nd) in enumerate(outs):
            s = ctypes.c_void_p()
            assert hip.hipStreamCreate(ctypes.byref(s)) == 0
            A.check_device(models.MODEL_BANK, d_hdr.data_ptr(), n, d_ev.data_ptr(), len(ev), st.data_ptr(),
                           nd.data_ptr(), None, None, max_nodes=10**7, stream=s.value)
            assert hip.hipStreamSynchronize(s) == 0
            assert hip.hipStreamDestroy(s) == 0
            if k == 1:
                A.probe()                        # a host wait after the stream is gone
        for st, nd in outs:
            assert np.array_equal(st.cpu().numpy(), st_o)
            assert np.array_equal(nd.cpu().numpy().astype(np.uint64), nd_o.astype(np.uint64))
    finally:
        A.close()                                # (the last call's stream destroyed too)


def test_packed_lookalike_layouts(ctx):
    """Batches with n_events == 32 n_hist that are NOT one packed block of
    32-event histories in header order come out as the oracle's: mixed
    lengths, permuted headers, shorter histories with trailing events, every
    header pointing one block on, and a partial last group.  (Round 5 built a
    speculative first staging step keyed on n_events / n_hist -- measured no
    faster, removed, DESIGN.md §10 -- and these are the layouts it had to
    reject.)"""
    rng = random.Random(31)
    hdr, ev, _ = gen.generate_config("bank_4x16", 77, 64 * 40 + 19)      # packed 32-event histories
    n = len(hdr)
    assert len(ev) == 32 * n
    _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**7)            # as laid out (partial last group)
    rot = hdr.copy()                                                      # each header points one block on
    rot["ev_off"] = (np.arange(n, dtype=np.int64) + 1) % n * 32
    for i in range(n):                                                    # (the history that was there)
        rot[i]["n_ev"], rot[i]["n_pid"] = hdr[(i + 1) % n]["n_ev"], hdr[(i + 1) % n]["n_pid"]
    _compare(ctx, models.MODEL_BANK, rot, ev, max_nodes=10**7)
    perm = hdr[np.random.default_rng(5).permutation(n)]                   # permuted headers
    _compare(ctx, models.MODEL_BANK, perm, ev, max_nodes=10**7)
    hs = [histgen.wellformed_history(rng, "bank", 8, rng.randint(1, 4), p_pending=0.0)[:16] for _ in range(2000)]
    short = codec.encode(models.BANK, hs)                                 # <= 16 events each, then padding
    pad = np.zeros(32 * len(short.hdr) - len(short.events), dtype=short.events.dtype)
    _compare(ctx, models.MODEL_BANK, short.hdr, np.concatenate([short.events, pad]), max_nodes=10**7)
    hs = []
    while len(hs) < 64 * 20:                                              # 28 / 36 alternating: 32 on average
        k = 28 if len(hs) % 2 == 0 else 36
        h = histgen.wellformed_history(rng, "bank", k // 2 + 2, rng.randint(1, 4), p_pending=0.0)
        if len(h) >= k:
            hs.append(h[:k])
    mixed = codec.encode(models.BANK, hs)
    assert len(mixed.events) == 32 * len(mixed.hdr)
    _compare(ctx, models.MODEL_BANK, mixed.hdr, mixed.events, max_nodes=10**7)


def test_stage0w_budget_auto(ctx, knobs):
    """The automatic stage-0w budget (the default until one is set): 24 with
    the heavy stage in lane mode, 48 in wave mode; setting "stage0w_budget"
    turns it off and "stage0w_budget_auto" 1 back on.  Config-5-shaped
    batches (6x24 Bank, every history 48 events) in both modes and at a set
    budget: the oracle's results."""
    assert ctx.get_param("stage0w_budget_auto") == 1
    hdr, ev, _ = gen.generate_config("bank_6x24", 5, 4000)
    for heavy in (1, 0):
        knobs(heavy_mode=heavy)
        _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**7)
    knobs(stage0w_budget=40)
    assert ctx.get_param("stage0w_budget_auto") == 0
    _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=10**7)
    knobs(stage0w_budget_auto=1)
    assert ctx.get_param("stage0w_budget_auto") == 1


def test_stage0_budget_last():
    """qsmd_get_param("stage0_budget_last"): the budget stage 0 ran with --
    the set one, capped below 2^31 (a saved state keeps its count in 32
    bits), 0xFFFFFFFF for none (budget 0) -- which bench.py's roofline uses
    to split stage 0's and the heavy stage's bytes."""
    c = device.Context(0)
    try:
        hdr, ev, _ = gen.generate_config("bank_4x16_bugs", 3, 3000)
        st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, threads=8)
        for budget, want in ((20, 20), (0, 0xFFFFFFFF), ((1 << 31) + 5, 0x7FFFFFFF)):
            c.set_stage0_budget(budget)
            st, nd, _, _ = c.check_arrays(models.MODEL_BANK, hdr, ev)
            assert c.get_param("stage0_budget_last") == want, budget
            assert (st == st_o).all() and (nd == nd_o).all()
    finally:
        c.close()
