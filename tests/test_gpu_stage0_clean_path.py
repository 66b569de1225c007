"""Stage 0's staging of packed batches against the oracle.

A packed batch is staged by stage_packed (csrc/lane.h) with the compressed
words built without the per-event validity select, and -- when no lane of
the group met a suspect event -- finish_lane without its marker handling.
A group with any suspect event is staged again with the markers.
Every case compares statuses, node counts and witnesses with oracle_c through
the device entry (bit-exact: integer search, no tolerance), at the smallest
shapes at which these paths differ: every power-of-two length, whole and
partial groups, one and several groups, the unaligned and the general paths
beside them, and suspect events of every kind at the corners of a group.
"""

import numpy as np
import pytest

import oracle_c
from qsmd import codec, gen, models

pytestmark = pytest.mark.gpu

BANK, TICKET = models.MODEL_BANK, models.MODEL_TICKET
RESP = 0x80


def _compare(ctx, model_id, hdr, ev, max_nodes=0):
    st_d, nd_d, w_d, tot = ctx.check_arrays(model_id, hdr, ev, max_nodes=max_nodes, witness=True)
    st_o, nd_o, w_o = oracle_c.check_batch(model_id, hdr, ev, None, max_nodes, 8, witness=True)
    bad = np.nonzero((st_d != st_o) | (nd_d != nd_o))[0]
    assert len(bad) == 0, (f"{len(bad)} mismatches, first {bad[:5]}: dev {st_d[bad[:5]]}/{nd_d[bad[:5]]} "
                           f"oracle {st_o[bad[:5]]}/{nd_o[bad[:5]]}")
    for i in np.nonzero(st_d == codec.STATUS_LIN)[0]:
        a, b = int(hdr[i]["ev_off"]), int(hdr[i]["ev_off"]) + int(hdr[i]["n_ev"])
        assert np.array_equal(w_d[a:b], w_o[a:b]), f"witness mismatch at history {i}"
    assert tot["nodes"] == int(nd_d.sum())
    assert tot["encode_errors"] == int((st_d == 3).sum())
    return st_d, nd_d, st_o, nd_o


_BATCHES = {}


def _packed(model, n_ev, n_hist, seed=3):
    """A generated packed batch of n_hist histories of n_ev events each (the
    benchmark's generator at n_ev / 2 operations; mostly linearisable, with
    injected race bugs for Bank)."""
    key = (model, n_ev, n_hist, seed)
    if key not in _BATCHES:
        n_ops = n_ev // 2
        if model == BANK:      # (the generator wants an operation per Bank client)
            kw = dict(name="bank_4x16_bugs", n_clients=min(4, n_ops))
        else:
            kw = dict(name="ticket_2x10", pid_mode=gen.PID_PER_CLIENT)
        hdr, ev, _ = gen.generate_config(first=seed * 1000, n_hist=n_hist, n_ops=n_ops,
                                         prefix_ops=min(4, n_ops // 2), **kw)
        assert (hdr["n_ev"] == n_ev).all() and (hdr["ev_off"] == np.arange(n_hist, dtype=np.int64) * n_ev).all()
        hdr.setflags(write=False)
        ev.setflags(write=False)
        _BATCHES[key] = (hdr, ev)
    return _BATCHES[key]


@pytest.mark.parametrize("model", [BANK, TICKET])
@pytest.mark.parametrize("n_ev", [2, 4, 8, 16, 32])
def test_packed_pow2_lengths_and_group_sizes(ctx, model, n_ev):
    """1, 63, 64, 65 and 129 histories: a lone history, a partial group, a
    whole one, a whole one and a lone history, two and a lone one (the last
    group's guarded step; with 2 events per history one step holds them all)."""
    hdr, ev = _packed(model, n_ev, 129)
    for n in (1, 63, 64, 65, 129):
        _compare(ctx, model, hdr[:n], ev[:n * n_ev])


@pytest.mark.parametrize("model", [BANK, TICKET])
@pytest.mark.parametrize("n_ev", [2, 8, 32])
def test_odd_start_takes_the_unaligned_path(ctx, model, n_ev):
    """The same batch one event further on: an odd ev_off (8-byte loads)."""
    hdr, ev = _packed(model, n_ev, 129)
    hdr = hdr.copy()
    hdr["ev_off"] += 1
    ev = np.concatenate([ev[:1], ev])
    for n in (63, 129):
        _compare(ctx, model, hdr[:n], ev[:1 + n * n_ev])


@pytest.mark.parametrize("n_ev", [3, 31])
def test_non_power_of_two_lengths(ctx, n_ev):
    """Packed batches of 3 and 31 events (the general packed path): the
    histories of a longer generated batch cut short."""
    hdr32, ev32 = _packed(BANK, 32, 129)
    ev = np.concatenate([ev32[i * 32:i * 32 + n_ev] for i in range(129)])
    hdr = hdr32.copy()
    hdr["n_ev"] = n_ev
    hdr["ev_off"] = np.arange(129) * n_ev
    for n in (64, 129):                       # (31 x 64 even, 31 x 129 odd totals)
        _compare(ctx, BANK, hdr[:n], ev[:n * n_ev], max_nodes=100000)


def test_64_event_batch_through_stage_0w(ctx):
    """Bank 64-event histories: stage 0 passes them on, stage 0w (the 64-event
    instance of the same staging) stages them packed."""
    hdr, ev, _ = gen.generate_config("bank_6x24", 5, 129, n_ops=32, prefix_ops=6)
    assert (hdr["n_ev"] == 64).all()
    for n in (1, 63, 129):       # (no history for stage 0: stage 0w runs over the batch itself)
        _compare(ctx, BANK, hdr[:n], ev[:n * 64], max_nodes=200000)
    # behind a group of 32-event histories: stage 0w over stage 0's deferred list
    hdr32, ev32 = _packed(BANK, 32, 129)
    h2 = hdr.copy()
    h2["ev_off"] += 64 * 32
    _compare(ctx, BANK, np.concatenate([hdr32[:64], h2]), np.concatenate([ev32[:64 * 32], ev]), max_nodes=200000)
    assert ctx.probe()["deferred"] == 129


# ---- suspect events: the group is staged again with the markers

def _find(ev, lo, hi, k, want_resp):
    """The event of the wanted kind nearest to k within [lo, hi)."""
    for d in range(hi - lo):
        for j in (k + d, k - d):
            if lo <= j < hi and bool(ev["kp"][j] & RESP) == want_resp:
                return j
    raise AssertionError("no such event")


def _plant(kind, hdr, ev, h, pos):
    """Plant one suspect event of `kind` in history h at (or, for a kind that
    needs an invocation or a response, nearest to) event pos."""
    lo = int(hdr["ev_off"][h])
    hi = lo + int(hdr["n_ev"][h])
    k = lo + pos
    if kind == "code>4":                           # no such Bank request / Ticket constructor
        k = _find(ev, lo, hi, k, False)
        ev["code"][k] = 5
    elif kind == "pid>=8":
        ev["kp"][k] = (ev["kp"][k] & RESP) | 8
    elif kind == "pid>=n_pid/3":                   # (an error only where the history has a pid 3)
        hdr["n_pid"][h] = 3
        ev["kp"][k] = (ev["kp"][k] & RESP) | 3
    elif kind == "pid>=n_pid/4":
        hdr["n_pid"][h] = 4
        ev["kp"][k] = (ev["kp"][k] & RESP) | 5
    elif kind == "inv=256":                        # one past the 9-bit field: the next stage
        k = _find(ev, lo, hi, k, False)
        ev["val"][k] = 256
    elif kind == "resp=2^24":                      # one past the 25-bit field
        k = _find(ev, lo, hi, k, True)
        ev["val"][k] = 1 << 24
    elif kind == "junk":                           # a field the constructor does not use
        if ev["kp"][k] & RESP:
            ev["a"][k] = 0x10
        else:
            ev["b"][k] = 0x40 if ev["code"][k] != 4 else ev["b"][k]
            ev["a"][k] |= 0x20 if ev["code"][k] == 4 else 0
    else:
        raise AssertionError(kind)


KINDS = ["code>4", "pid>=8", "pid>=n_pid/3", "pid>=n_pid/4", "inv=256", "resp=2^24", "junk"]


def _planted(model, n_ev, every_group):
    """One group per (kind, history, event) with history and event each the
    first, a middle and the last of the group / the history; between two such
    groups a clean one unless every_group."""
    spots = [(kind, hh, pos) for kind in KINDS for hh in (0, 31, 63) for pos in (0, n_ev // 2, n_ev - 1)]
    stride = 1 if every_group else 2
    n_groups = len(spots) * stride
    hdr, ev = _packed(model, n_ev, 64 * n_groups + 7, seed=5)
    hdr, ev = hdr.copy(), ev.copy()
    for g, (kind, hh, pos) in enumerate(spots):
        _plant(kind, hdr, ev, 64 * g * stride + hh, pos)
    return hdr, ev


@pytest.mark.parametrize("every_group", [False, True])
@pytest.mark.parametrize("model,n_ev", [(BANK, 32), (BANK, 8), (TICKET, 16)])
def test_one_suspect_event_in_a_group(ctx, model, n_ev, every_group):
    """One suspect event -- a code above 4, a pid of 8, a pid beyond n_pid 3 or
    4, an invocation value of 256, a response value of 2^24, junk in an unused
    field -- at the first, a middle and the last event of the first, a middle
    and the last history of a group, its 63 neighbours clean; the groups
    between clean (the fast path beside the slow one) or planted too."""
    hdr, ev = _planted(model, n_ev, every_group)
    st, nd, st_o, _ = _compare(ctx, model, hdr, ev, max_nodes=100000)
    # the plants did what they are for: encode errors and wide histories
    assert (st_o == 3).sum() >= 9 * 3
    if model == BANK:
        assert ctx.probe()["deferred"] >= 9 * 2


@pytest.mark.parametrize("budget", [16, 17, 20])
def test_stage0_budgets_route_as_before(ctx, budget):
    """4,096 config-2 histories at stage-0 budgets 16 and 20 (and 17: with 9
    in 10 searches 16 nodes long, budgets 16 and 17 put the leaf exactly at
    the budget and one node before it): the heavy list holds exactly the
    histories whose search needs more nodes than the budget, and the final
    results are the oracle's."""
    hdr, ev, _ = gen.generate_config("bank_4x16", 0, 4096)
    ctx.set_param("stage0_budget", budget)
    try:
        st, nd, st_o, nd_o = _compare(ctx, BANK, hdr, ev)
        pr = ctx.probe()
    finally:
        ctx.set_param("stage0_budget", 32)
    assert (nd_o == 16).sum() > 2048
    assert pr["heavy32"] == int((nd_o > budget).sum()) and pr["deferred"] == 0 and pr["giants"] == 0
