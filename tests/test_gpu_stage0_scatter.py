"""Stage 0's packed scatter and its per-group shortcuts against the oracle.

A packed group's events are loaded in the order of csrc/scatter_map.h (a quad
of lanes per history for a power-of-two length; block order for any other)
and stored at [event][history], a full stage-0 group with two steps' loads in
flight together.  A word in a wrong row or column changes a
verdict or a node count, so every case compares status, node count and
witness per history with oracle_c (integer search: bit-exact, no tolerance)
and probe()'s heavy32 / deferred with the oracle's node counts at the stage
budget in force.  The shapes are the smallest at which a wrong map or a wrong
wave-uniform shortcut shows: every power-of-two length and some that are not,
group sizes around 1, 64 and 128, the unaligned and the unpacked paths beside
the mapped one, injected events and headers in one lane of a full group, an
initial model, and the stage budgets around the common search length.
"""

import random

import numpy as np
import pytest

import histgen
import oracle_c
from qsmd import codec, device, gen, models
from test_gpu_parity import DEFAULTS

pytestmark = pytest.mark.gpu

BANK, TICKET = models.MODEL_BANK, models.MODEL_TICKET
RESP = 0x80
NONLIN, LIN, ENCODE_ERROR, BUDGET, SKIPPED = (codec.STATUS_NONLIN, codec.STATUS_LIN, codec.STATUS_ENCODE_ERROR,
                                              codec.STATUS_BUDGET, codec.STATUS_SKIPPED)
STAGE_BUDGET = 20
MAXN = 200000


@pytest.fixture(scope="module")
def dev():
    """A context of this module's own at a fixed stage-0 / 0w budget."""
    c = device.Context(0, time_limit_ms=60000)
    c.set_param("stage0_budget", STAGE_BUDGET)
    c.set_param("stage0w_budget", STAGE_BUDGET)
    yield c
    c.close()


@pytest.fixture
def knobs(dev):
    def set_(**kw):
        for k, v in kw.items():
            dev.set_param(k, v)
    yield set_
    for k, v in DEFAULTS.items():
        dev.set_param(k, v)
    dev.set_param("stage0_budget", STAGE_BUDGET)
    dev.set_param("stage0w_budget", STAGE_BUDGET)


_ORACLE = {}


def oracle(key, model_id, hdr, ev, model0=None, max_nodes=0):
    """The oracle's (status, nodes, witness) of a batch, computed once per key."""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_c.check_batch(model_id, hdr, ev, model0, max_nodes, 8, witness=True)
    return _ORACLE[key]


def compare(dev, model_id, hdr, ev, ref, model0=None, max_nodes=0, budget=STAGE_BUDGET, deferred=0, stage="0"):
    """The device's arrays against the first len(hdr) of the oracle's, and the
    route: stage 0 hands on exactly `deferred` histories, and the heavy list
    of the searching stage holds exactly the histories whose search needs
    more nodes than the stage budget (none when the caller's max_nodes is the
    smaller bound: such a search ends BUDGET in the stage itself)."""
    st_o, nd_o, w_o = ref
    n = len(hdr)
    st_d, nd_d, w_d, tot = dev.check_arrays(model_id, hdr, ev, model0, max_nodes=max_nodes, witness=True)
    pr = dev.probe()
    bad = np.nonzero((st_d != st_o[:n]) | (nd_d != nd_o[:n]))[0]
    assert len(bad) == 0, (f"{len(bad)} mismatches, first {bad[:5]}: dev {st_d[bad[:5]]}/{nd_d[bad[:5]]} "
                           f"oracle {st_o[bad[:5]]}/{nd_o[bad[:5]]}")
    for i in np.nonzero(st_d == LIN)[0]:
        a, b = int(hdr[i]["ev_off"]), int(hdr[i]["ev_off"]) + int(hdr[i]["n_ev"])
        assert np.array_equal(w_d[a:b], w_o[a:b]), f"witness mismatch at history {i}"
    assert tot["nodes"] == int(nd_d.sum())
    assert tot["linearisable"] == int((st_d == LIN).sum()) and tot["nonlinearisable"] == int((st_d == NONLIN).sum())
    assert tot["encode_errors"] == int((st_d == ENCODE_ERROR).sum())
    over = 0 if (max_nodes and max_nodes <= budget) or budget == 0 else int((nd_o[:n] > budget).sum())
    want = {"deferred": deferred, "heavy32": over if stage == "0" else 0}
    if stage == "0w":
        want["heavy64"] = over
    assert {k: pr[k] for k in want} == want, (pr, want)
    return st_d, nd_d


_BATCHES = {}


def packed(model, n_ev, n_hist, seed=29, **kw):
    """A generated packed batch: n_hist distinct histories of n_ev events each."""
    key = (model, n_ev, n_hist, seed, tuple(sorted(kw.items())))
    if key not in _BATCHES:
        n_ops = n_ev // 2
        if model == BANK:
            par = dict(name="bank_4x16_bugs", n_clients=min(4, n_ops), prefix_ops=min(4, n_ops // 2))
        else:
            par = dict(name="ticket_2x10", prefix_ops=min(4, n_ops // 2))
        par.update(kw)
        hdr, ev, _ = gen.generate_config(first=seed * 1000, n_hist=n_hist, n_ops=n_ops, **par)
        assert (hdr["n_ev"] == n_ev).all() and (hdr["ev_off"] == np.arange(n_hist, dtype=np.int64) * n_ev).all()
        hdr.setflags(write=False)
        ev.setflags(write=False)
        _BATCHES[key] = (hdr, ev)
    return _BATCHES[key]


def short(n_ev, n_hist, seed=41):
    """n_hist random Bank histories of n_ev events on 3 pids, any shape
    (tests/histgen.py): the generator's histories of under 16 events are its
    sequential prefix, the same for all."""
    key = ("short", n_ev, n_hist, seed)
    if key not in _BATCHES:
        rng = random.Random(seed * 100 + n_ev)
        b = codec.encode(models.BANK, [histgen.random_history(rng, "bank", n_ev, 3) for _ in range(n_hist)])
        assert (b.hdr["n_ev"] == n_ev).all() and (b.hdr["ev_off"] == np.arange(n_hist, dtype=np.int64) * n_ev).all()
        _BATCHES[key] = (b.hdr, b.events)
    return _BATCHES[key]


def distinct(ev, n_ev, n):
    return len({ev[i * n_ev:(i + 1) * n_ev].tobytes() for i in range(n)})


SIZES = (1, 2, 63, 64, 65, 127, 129)


@pytest.mark.parametrize("n_ev", [2, 4, 8, 16, 32, 6, 10, 20, 30])
def test_packed_bank_lengths_and_group_sizes(dev, n_ev):
    """Packed Bank batches of every power-of-two length and of 6, 10, 20 and
    30 events, 1 to 129 histories: a lone history, a pair, a partial group, a
    whole one, one and a lone history, two less one, two and a lone one."""
    hdr, ev = packed(BANK, n_ev, 129) if n_ev >= 16 else short(n_ev, 129)
    assert distinct(ev, n_ev, 129) >= (129 if n_ev >= 6 else 100)
    ref = oracle(("bank", n_ev), BANK, hdr, ev)
    if n_ev >= 16:
        assert (ref[0] == NONLIN).sum() >= 8 and (ref[0] == LIN).sum() >= 8
    if n_ev >= 30:
        assert (ref[1] > STAGE_BUDGET).sum() >= 4
    for n in SIZES:
        compare(dev, BANK, hdr[:n], ev[:n * n_ev], ref)


@pytest.mark.parametrize("config,n_ev", [("bank_6x24", 48), ("bank_6x24", 64)])
def test_stage_0w_lengths_and_group_sizes(dev, config, n_ev):
    """Stage 0w (the 64-event instance of the same staging): bank_6x24's 48
    events (block order) and 64 events (the map with 8 histories per step),
    1, 64 and 65 histories.  No history fits stage 0, so stage 0w runs over
    the batch itself."""
    hdr, ev, _ = gen.generate_config(config, 31000, 65, n_ops=n_ev // 2)
    assert (hdr["n_ev"] == n_ev).all() and distinct(ev, n_ev, 65) == 65
    ref = oracle((config, n_ev), BANK, hdr, ev, max_nodes=MAXN)
    assert (ref[1] > STAGE_BUDGET).sum() >= 8 and (ref[0] == LIN).sum() >= 8
    for n in (1, 64, 65):
        compare(dev, BANK, hdr[:n], ev[:n * n_ev], ref, max_nodes=MAXN, stage="0w")


def test_stage_0w_behind_stage_0(dev):
    """A group of 32-event histories, then 65 of 64 events: stage 0 defers the
    65, stage 0w stages them packed from its list."""
    hdr32, ev32 = packed(BANK, 32, 129)
    hdr64, ev64, _ = gen.generate_config("bank_6x24", 31000, 65, n_ops=32)
    h2 = hdr64.copy()
    h2["ev_off"] += 64 * 32
    hdr, ev = np.concatenate([hdr32[:64], h2]), np.concatenate([ev32[:64 * 32], ev64])
    ref = oracle("0w behind 0", BANK, hdr, ev, max_nodes=MAXN)
    st_d, nd_d, _, _ = dev.check_arrays(BANK, hdr, ev, max_nodes=MAXN, witness=True)
    pr = dev.probe()
    assert np.array_equal(st_d, ref[0]) and np.array_equal(nd_d, ref[1])
    assert pr["deferred"] == 65 and pr["heavy32"] == int((ref[1][:64] > STAGE_BUDGET).sum())
    assert pr["heavy64"] == int((ref[1][64:] > STAGE_BUDGET).sum())


@pytest.mark.parametrize("model,n_ev", [(BANK, 32), (BANK, 20), (BANK, 4), (TICKET, 20)])
def test_odd_start_keeps_the_8_byte_path(dev, model, n_ev):
    """One dummy event before the batch: an odd first ev_off, 8-byte loads in
    block order."""
    hdr0, ev0 = packed(model, n_ev, 129) if n_ev >= 16 else short(n_ev, 129)
    ref = oracle((model, n_ev, "plain"), model, hdr0, ev0)
    hdr = hdr0.copy()
    hdr["ev_off"] += 1
    ev = np.concatenate([ev0[:1], ev0])
    for n in (1, 64, 129):
        st_d, nd_d, w_d, _ = dev.check_arrays(model, hdr[:n], ev[:1 + n * n_ev], witness=True)
        assert np.array_equal(st_d, ref[0][:n]) and np.array_equal(nd_d, ref[1][:n])
        assert np.array_equal(w_d[1:][st_d.repeat(n_ev) == LIN], ref[2][:n * n_ev][st_d.repeat(n_ev) == LIN])
        pr = dev.probe()
        assert pr["heavy32"] == int((ref[1][:n] > STAGE_BUDGET).sum()) and pr["deferred"] == 0


@pytest.mark.parametrize("where", [0, 30, 63])
def test_one_other_length_in_a_group_is_not_packed(dev, where):
    """The history at lane 0, 30 or 63 of the middle group of three has 30
    events among 32-event ones: that group stages lane by lane, its
    neighbours packed (the second one from an even, then shifted, start)."""
    hdr0, ev0 = packed(BANK, 32, 192)
    k = 64 + where
    keep = np.ones(len(ev0), dtype=bool)
    keep[k * 32 + 30:k * 32 + 32] = False
    ev = ev0[keep]
    hdr = hdr0.copy()
    hdr["n_ev"][k] = 30
    hdr["ev_off"][k + 1:] -= 2
    ref = oracle(("other length", where), BANK, hdr, ev)
    compare(dev, BANK, hdr, ev, ref)


def _injected():
    """Three groups of 32-event Bank histories; in the middle one, each in one
    lane of the otherwise clean full group: an illegal request code, an
    invocation value one past the compact field, a 5-client history with
    n_pid 5 (a pid above 3: the group compares three pid slices)."""
    if "injected" not in _BATCHES:
        hdr0, ev0 = packed(BANK, 32, 192)
        _, ev5 = packed(BANK, 32, 4, seed=37, n_clients=5, prefix_ops=5)
        hdr, ev = hdr0.copy(), ev0.copy()
        inv = lambda h: h * 32 + int(np.nonzero((ev["kp"][h * 32:(h + 1) * 32] & RESP) == 0)[0][3])
        ev["code"][inv(64 + 0)] = 5
        ev["val"][inv(64 + 17)] = 256
        ev[(64 + 40) * 32:(64 + 41) * 32] = ev5[:32]
        hdr["n_pid"][64 + 40] = 5
        ev["code"][inv(64 + 63)] = 6
        _BATCHES["injected"] = (hdr, ev)
    return _BATCHES["injected"]


def test_injected_events_in_one_lane_of_a_full_group(dev):
    hdr, ev = _injected()
    assert int((ev["kp"][(64 + 40) * 32:(64 + 41) * 32] & 0x7F).max()) == 4
    ref = oracle("injected", BANK, hdr, ev, max_nodes=MAXN)
    assert ref[0][64] == ENCODE_ERROR and ref[0][64 + 63] == ENCODE_ERROR and (ref[0] == ENCODE_ERROR).sum() == 2
    assert ref[0][64 + 40] != ENCODE_ERROR and ref[1][64 + 40] >= 16
    # the history with the wide value leaves stage 0: not on its heavy list
    st_d, nd_d, w_d, tot = dev.check_arrays(BANK, hdr, ev, max_nodes=MAXN, witness=True)
    pr = dev.probe()
    assert np.array_equal(st_d, ref[0]) and np.array_equal(nd_d, ref[1])
    for i in np.nonzero(st_d == LIN)[0]:
        assert np.array_equal(w_d[i * 32:(i + 1) * 32], ref[2][i * 32:(i + 1) * 32]), i
    in0 = np.ones(192, dtype=bool)
    in0[64 + 17] = False
    assert pr["deferred"] == 1 and pr["heavy32"] == int((ref[1][in0] > STAGE_BUDGET).sum())
    assert tot["encode_errors"] == 2


@pytest.mark.parametrize("where", [0, 31, 64, 128])
def test_an_empty_history(dev, where):
    """A history of no events (LINEARISABLE, 0 nodes) at the head, in the
    middle and at the end of a group and alone in the last one."""
    hdr0, ev0 = packed(BANK, 32, 129)
    hdr = hdr0.copy()
    hdr["n_ev"][where] = 0
    hdr["ev_off"][where + 1:] -= 32
    ev = np.concatenate([ev0[:where * 32], ev0[(where + 1) * 32:]])
    ref = oracle(("empty", where), BANK, hdr, ev)
    assert ref[0][where] == LIN and ref[1][where] == 0
    compare(dev, BANK, hdr, ev, ref)


@pytest.mark.parametrize("exists,vals", [(0b00000011, (50, 7, 0, 0, 0, 0, 0, 0)),
                                         (0b01000001, (50, 0, 0, 0, 0, 0, -3, 0)),
                                         (0b10000000, (0, 0, 0, 0, 0, 0, 0, 0))])
def test_initial_model(dev, exists, vals):
    """m0_exists != 0: accounts 0 and 1 open with 50 and 7 (the histories'
    OpenAccounts of them fail, the balances differ), a negative balance on an
    account no history opens (the invariant fails at every first node), and
    an untouched open account of 0 (the results of no initial model)."""
    hdr, ev = packed(BANK, 32, 129)
    m0 = models.BankModel(exists, 0, vals)
    ref = oracle(("m0", exists), BANK, hdr, ev, model0=m0)
    plain = oracle(("bank", 32), BANK, hdr, ev)
    if min(vals) < 0:
        assert (ref[0] == NONLIN).all() and (ref[1] == 1).all()
    elif exists == 0b10000000:
        assert np.array_equal(ref[0], plain[0]) and np.array_equal(ref[1], plain[1])
    else:
        assert not np.array_equal(ref[1], plain[1])
    for n in (64, 129):
        compare(dev, BANK, hdr[:n], ev[:n * 32], ref, model0=m0)


_C2 = {}


def config2():
    if not _C2:
        hdr, ev, _ = gen.generate_config("bank_4x16", 0, 4096)
        _C2["b"] = (hdr, ev)
    return _C2["b"]


@pytest.mark.parametrize("budget", [16, 17, 20])
def test_budgets_in_lane_mode(dev, knobs, budget):
    """4,096 config-2 histories at stage-0 budgets 16, 17 and 20 (9 in 10
    searches are 16 nodes long: the leaf at the budget, one node before it,
    and clear of it), the heavy stage in lane mode resuming the saved states."""
    hdr, ev = config2()
    ref = oracle("config2", BANK, hdr, ev)
    assert (ref[1] == 16).sum() > 2048 and (ref[1] > 20).sum() >= 16
    knobs(stage0_budget=budget, heavy_mode=1, memo_lds=0, memo_after=1)
    compare(dev, BANK, hdr, ev, ref, budget=budget)


def test_early_exit_with_a_planted_failure(dev):
    hdr, ev0 = config2()
    cut = 2500
    ev = gen.plant_failure(hdr, ev0, cut)
    ref = oracle("config2 planted", BANK, hdr, ev)
    assert ref[0][cut] == NONLIN and (ref[0][:cut] == LIN).all()
    st, nd, _, tot = dev.check_arrays(BANK, hdr, ev, flags=device.QSMD_FLAG_EXHAUSTIVE |
                                      device.QSMD_FLAG_EARLY_EXIT_BATCH)
    assert np.array_equal(st[:cut + 1], ref[0][:cut + 1]) and np.array_equal(nd[:cut + 1], ref[1][:cut + 1])
    assert (st[cut + 1:] == SKIPPED).all()
    assert tot["nodes"] == int(ref[1][:cut + 1].sum())


def test_caller_max_nodes_below_the_stage_budget(dev):
    hdr, ev = config2()
    ref = oracle("config2 max 12", BANK, hdr, ev, max_nodes=12)
    assert (ref[0] == BUDGET).sum() > 2048 and (ref[1][ref[0] == BUDGET] == 12).all()
    compare(dev, BANK, hdr, ev, ref, max_nodes=12)


@pytest.mark.parametrize("n", [64, 65])
def test_ticket_2x10(dev, n):
    """ticket_2x10: 20 events (block order), one shared pid."""
    hdr, ev = packed(TICKET, 20, 65)
    assert distinct(ev, 20, 65) >= 60
    ref = oracle("ticket_2x10", TICKET, hdr, ev)
    assert (ref[0] == LIN).sum() >= 8
    compare(dev, TICKET, hdr[:n], ev[:n * 20], ref)
