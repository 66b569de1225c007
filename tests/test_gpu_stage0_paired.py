"""Stage 0's DFS step on the shapes at which its paths differ.

Written with the attempt to pair each operation of a packed group once and
search without the pid masks (HISTORY.md §10: measured, removed), and kept
for what stage 0 runs now (csrc/compact.hip, csrc/lane.h): one choice per
group of 64 between the pid compare over two slices (no searched history has
a pid above 3) and over three, and a step loop that lanes leave one by one.
Every case compares statuses, node counts and witnesses with oracle_c through
the device entry (integer search: bit-exact, no tolerance): packed batches at
every group size, several lengths and stage-0 budgets (a budget-stopped search
resumes in the heavy stage from the saved state), one history of a group
whose pids do not alternate invocation / response, operations without a
response, 1 to 8 pids in one group and one history with a pid above 3 among
63 without, unpacked and mixed-length batches, and searches that fail,
backtrack or raise.  Each test asserts on the oracle's side that the verdicts
it is about occur.
"""

import numpy as np
import pytest

import oracle_c
from qsmd import codec, device, gen, models

pytestmark = pytest.mark.gpu

BANK, TICKET = models.MODEL_BANK, models.MODEL_TICKET
RESP = 0x80
NONLIN, LIN, MODEL_ERROR, ENCODE_ERROR = (codec.STATUS_NONLIN, codec.STATUS_LIN, codec.STATUS_MODEL_ERROR,
                                          codec.STATUS_ENCODE_ERROR)
BUDGETS = (4, 16, 20, 0)            # stage-0 node budgets; 0: unlimited
SIZES = (1, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def dev():
    """A context of this module's own (the tests set its stage-0 budget)."""
    c = device.Context(0, time_limit_ms=60000)
    yield c
    c.close()


_ORACLE = {}


def oracle(key, model_id, hdr, ev, max_nodes=0):
    """The oracle's (status, nodes, witness) of a batch, computed once per key."""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_c.check_batch(model_id, hdr, ev, None, max_nodes, 8, witness=True)
    return _ORACLE[key]


def compare(dev, model_id, hdr, ev, ref, max_nodes=0):
    st_o, nd_o, w_o = ref
    st_d, nd_d, w_d, tot = dev.check_arrays(model_id, hdr, ev, max_nodes=max_nodes, witness=True)
    n = len(hdr)
    bad = np.nonzero((st_d != st_o[:n]) | (nd_d != nd_o[:n]))[0]
    assert len(bad) == 0, (f"{len(bad)} mismatches, first {bad[:5]}: dev {st_d[bad[:5]]}/{nd_d[bad[:5]]} "
                           f"oracle {st_o[bad[:5]]}/{nd_o[bad[:5]]}")
    for i in np.nonzero(st_d == LIN)[0]:
        a, b = int(hdr[i]["ev_off"]), int(hdr[i]["ev_off"]) + int(hdr[i]["n_ev"])
        assert np.array_equal(w_d[a:b], w_o[a:b]), f"witness mismatch at history {i}"
    assert tot["nodes"] == int(nd_d.sum())
    return st_d, nd_d


def at_budgets(dev, model_id, hdr, ev, ref, budgets=BUDGETS, max_nodes=0):
    try:
        for b in budgets:
            dev.set_param("stage0_budget", b)
            compare(dev, model_id, hdr, ev, ref, max_nodes)
    finally:
        dev.set_param("stage0_budget_auto", 1)


_BATCHES = {}


def packed(model, n_ev, n_hist, seed=7, **kw):
    """A generated packed batch: n_hist histories of n_ev events each, one pid
    per client, half of them with an injected bug."""
    key = (model, n_ev, n_hist, seed, tuple(sorted(kw.items())))
    if key not in _BATCHES:
        n_ops = n_ev // 2
        if model == BANK:
            par = dict(name="bank_4x16_bugs", n_clients=min(4, n_ops))
        else:
            par = dict(name="ticket_2x10", pid_mode=gen.PID_PER_CLIENT, n_clients=min(3, n_ops), p_bug=0.5)
        par.update(kw)
        par.setdefault("prefix_ops", min(par["n_clients"], n_ops))
        hdr, ev, _ = gen.generate_config(first=seed * 1000, n_hist=n_hist, n_ops=n_ops, **par)
        assert (hdr["n_ev"] == n_ev).all() and (hdr["ev_off"] == np.arange(n_hist, dtype=np.int64) * n_ev).all()
        hdr.setflags(write=False)
        ev.setflags(write=False)
        _BATCHES[key] = (hdr, ev)
    return _BATCHES[key]


def alternates(ev):
    """True when every pid's events alternate invocation, response."""
    open_ = set()
    for kp in ev["kp"]:
        pid, resp = int(kp) & 0x7F, bool(kp & RESP)
        if resp != (pid in open_):
            return False
        (open_.discard if resp else open_.add)(pid)
    return True


# ---- 1, 2: packed batches, every group size, lengths and budgets

@pytest.mark.parametrize("n_ev", [2, 8, 16, 30, 32])
@pytest.mark.parametrize("model", [BANK, TICKET])
def test_packed_batches_at_stage0_budgets(dev, model, n_ev):
    """1, 63, 64, 65 and 129 histories of 2, 8, 16, 30 and 32 events at stage-0
    budgets 4, 16, 20 and unlimited: a search the budget stops goes on in the
    heavy stage from the state stage 0 saved."""
    hdr, ev = packed(model, n_ev, 129)
    ref = oracle(("packed", model, n_ev), model, hdr, ev)
    assert all(alternates(ev[i * n_ev:(i + 1) * n_ev]) for i in range(129))
    if n_ev >= 16:      # searches longer than the smallest budget, ones that fail and ones that do not
        assert (ref[1] > 4).sum() >= 64 and (ref[0] == NONLIN).sum() >= 8 and (ref[0] == LIN).sum() >= 8
    if n_ev >= 30:      # and longer than every budget
        assert (ref[1] > 20).sum() >= 4
    for n in SIZES:
        at_budgets(dev, model, hdr[:n], ev[:n * n_ev], ref)


# ---- 3: one history of a group whose pids do not alternate

def _break(kind, ev, lo, n_ev):
    """Break the alternation of the history at events [lo, lo + n_ev)."""
    h = ev[lo:lo + n_ev]
    if kind == "inv_inv":            # a second invocation of a pid whose operation is outstanding
        open_ = set()
        for k in range(n_ev):
            pid, resp = int(h["kp"][k]) & 0x7F, bool(h["kp"][k] & RESP)
            if not resp and open_ - {pid}:
                h["kp"][k] = min(open_ - {pid})
                return
            (open_.discard if resp else open_.add)(pid)
        raise AssertionError("a sequential history")
    elif kind == "resp_first":
        h[[0, 1]] = h[[1, 0]]
    elif kind == "one_pid":          # every event on pid 0, as ticket_2x10's shared pid
        h["kp"] &= RESP
    else:
        raise AssertionError(kind)


@pytest.mark.parametrize("where", [0, 31, 63])
@pytest.mark.parametrize("kind", ["inv_inv", "resp_first", "one_pid"])
@pytest.mark.parametrize("model,n_ev", [(BANK, 32), (TICKET, 20)])
def test_one_history_that_does_not_alternate(dev, model, n_ev, kind, where):
    """A group of 64 in which exactly the history at lane 0, 31 or 63 has two
    invocations of a pid in a row, a response first, or all events on one pid:
    that history and its 63 neighbours match the oracle."""
    hdr, ev0 = packed(model, n_ev, 64, seed=11)
    ev = ev0.copy()
    _break(kind, ev, where * n_ev, n_ev)
    ok = [alternates(ev[i * n_ev:(i + 1) * n_ev]) for i in range(64)]
    assert ok.count(False) == 1 and not ok[where]
    ref = oracle(("broken", model, kind, where), model, hdr, ev, 200000)
    assert (ref[0] != ENCODE_ERROR).all()
    at_budgets(dev, model, hdr, ev, ref, budgets=(4, 20, 0), max_nodes=200000)


# ---- 4: operations without a response

def _unanswered():
    """129 Bank histories of 28 events: 32-event ones cut short (the pids whose
    response fell off end with an invocation), and at lanes 0, 40 and 128 a
    sequential run of 12 operations followed by one unanswered invocation of
    each of the 4 pids."""
    if "unanswered" not in _BATCHES:
        hdr32, ev32 = packed(BANK, 32, 129, seed=13)
        ev = np.concatenate([ev32[i * 32:i * 32 + 28] for i in range(129)])
        _, evs = packed(BANK, 28, 3, seed=17, prefix_ops=14)
        for k, lane in enumerate((0, 40, 128)):
            h = evs[k * 28:(k + 1) * 28].copy()
            for p in range(4):
                h[24 + p] = (p, models.BANK_REQ["CheckBalance"], p, 0, 0)
            ev[lane * 28:(lane + 1) * 28] = h
        hdr = hdr32.copy()
        hdr["n_ev"] = 28
        hdr["ev_off"] = np.arange(129) * 28
        _BATCHES["unanswered"] = (hdr, ev)
    return _BATCHES["unanswered"]


def test_operations_without_a_response(dev):
    hdr, ev = _unanswered()
    n_open = []
    for i in range(129):
        h = ev[i * 28:(i + 1) * 28]
        assert alternates(h)
        inv = np.bincount(h["kp"][(h["kp"] & RESP) == 0], minlength=4)
        n_open.append(int((inv - np.bincount(h["kp"][(h["kp"] & RESP) != 0] & 0x7F, minlength=4)).sum()))
    assert n_open[0] == n_open[40] == n_open[128] == 4 and sum(1 for x in n_open if 0 < x < 4) >= 32
    ref = oracle("unanswered", BANK, hdr, ev, 200000)
    assert (ref[0] == LIN).sum() >= 16 and (ref[0] == NONLIN).sum() >= 16 and ref[0][0] == LIN
    for n in (64, 129):
        at_budgets(dev, BANK, hdr[:n], ev[:n * 28], ref, budgets=(4, 20, 0), max_nodes=200000)


# ---- 5: 1 to 8 pids in one group

def _pids_1_to_8():
    if "pids" not in _BATCHES:
        parts = [packed(BANK, 32, 16, seed=19 + c, n_clients=c)[1] for c in range(1, 9)]
        ev = np.concatenate([parts[i % 8][(i // 8) * 32:(i // 8 + 1) * 32] for i in range(128)])
        hdr = packed(BANK, 32, 128, seed=19)[0].copy()
        hdr["n_pid"] = np.arange(128) % 8 + 1
        _BATCHES["pids"] = (hdr, ev)
    return _BATCHES["pids"]


def test_one_to_eight_pids_per_lane(dev):
    hdr, ev = _pids_1_to_8()
    for i in range(128):
        assert int((ev["kp"][i * 32:(i + 1) * 32] & 0x7F).max()) == i % 8
    ref = oracle("pids", BANK, hdr, ev, 200000)
    assert (ref[0] == LIN).sum() >= 16 and (ref[0] == NONLIN).sum() >= 16 and (ref[0] != ENCODE_ERROR).all()
    at_budgets(dev, BANK, hdr, ev, ref, budgets=(4, 20, 0), max_nodes=200000)


@pytest.mark.parametrize("where", [0, 31, 63])
def test_one_history_with_a_pid_above_3(dev, where):
    """63 histories of 4 pids and, at lane 0, 31 or 63, one of 8: the group
    compares three pid slices; the groups before and after it two."""
    hdr4, ev4 = packed(BANK, 32, 192, seed=23)
    _, ev8 = packed(BANK, 32, 16, seed=26, n_clients=8)
    hdr, ev = hdr4.copy(), ev4.copy()
    k = 64 + where
    ev[k * 32:(k + 1) * 32] = ev8[:32]
    hdr["n_pid"][k] = 8
    assert int((ev["kp"] & 0x7F).max()) == 7 and int((ev4["kp"] & 0x7F).max()) == 3
    ref = oracle(("pid_above_3", where), BANK, hdr, ev, 200000)
    assert (ref[0] != ENCODE_ERROR).all() and ref[1][k] >= 16
    at_budgets(dev, BANK, hdr, ev, ref, budgets=(4, 20, 0), max_nodes=200000)


@pytest.mark.parametrize("where", [0, 37, 63])
def test_a_pid_beyond_n_pid_is_an_encode_error(dev, where):
    hdr, ev = _pids_1_to_8()
    hdr = hdr[:64].copy()
    ev = ev[:64 * 32]
    hdr["n_pid"][where] = max(1, where % 8)          # (one less than the history's pids; lane 0 has one pid)
    if where % 8 == 0:
        ev = ev.copy()
        ev["kp"][where * 32 + 5] |= 1
    ref = oracle(("pid_beyond", where), BANK, hdr, ev, 200000)
    assert ref[0][where] == ENCODE_ERROR and (ref[0] == ENCODE_ERROR).sum() == 1
    at_budgets(dev, BANK, hdr, ev, ref, budgets=(20, 0), max_nodes=200000)


# ---- 6: batches that are not packed

def test_unpacked_and_mixed_length_batches(dev):
    """The same histories with their events in another order than their
    headers (every lane stages its own history), and histories of 16, 30 and
    32 events mixed in one batch."""
    hdr0, ev0 = packed(BANK, 32, 129)
    perm = np.random.default_rng(5).permutation(129)
    hdr = hdr0.copy()
    hdr["ev_off"][perm] = np.arange(129) * 32
    ev = np.concatenate([ev0[i * 32:(i + 1) * 32] for i in perm])
    ref0 = oracle(("packed", BANK, 32), BANK, hdr0, ev0)
    ref = oracle("shuffled", BANK, hdr, ev)
    assert np.array_equal(ref[0], ref0[0]) and np.array_equal(ref[1], ref0[1])
    at_budgets(dev, BANK, hdr, ev, ref, budgets=(4, 20, 0))

    hs, es, off = [], [], 0
    for i in range(129):
        n_ev = (16, 30, 32)[i % 3]
        h, e = packed(BANK, n_ev, 129)
        hh = h[i:i + 1].copy()
        hh["ev_off"] = off
        hs.append(hh)
        es.append(e[i * n_ev:(i + 1) * n_ev])
        off += n_ev
    hdr, ev = np.concatenate(hs), np.concatenate(es)
    ref = oracle("mixed", BANK, hdr, ev)
    assert (ref[0] == NONLIN).sum() >= 8 and (ref[0] == LIN).sum() >= 8
    at_budgets(dev, BANK, hdr, ev, ref, budgets=(4, 20, 0))


# ---- 7: failing searches, with backtracking through undo

def _bugs4096():
    """bank_4x16_bugs, and in every 16th history the first CheckBalance asks
    for account 7, which no history opens: `Map.!` raises where the search
    reaches it with the invariant intact (MODEL_ERROR)."""
    if "bugs4096" not in _BATCHES:
        hdr, ev, _ = gen.generate_config("bank_4x16_bugs", 0, 4096)
        for i in range(0, 4096, 16):
            h = ev[i * 32:(i + 1) * 32]
            k = np.nonzero(((h["kp"] & RESP) == 0) & (h["code"] == models.BANK_REQ["CheckBalance"]))[0]
            if len(k):
                h["a"][k[0]] = 7
        _BATCHES["bugs4096"] = (hdr, ev)
    return _BATCHES["bugs4096"]


@pytest.mark.parametrize("budget", [20, 0])
def test_bank_bugs_4096(dev, budget):
    hdr, ev = _bugs4096()
    ref = oracle("bugs4096", BANK, hdr, ev)
    st = ref[0]
    assert (st == NONLIN).sum() >= 1000 and (st == LIN).sum() >= 1000 and (st == MODEL_ERROR).sum() >= 64
    # backtracking: searches longer than one descent, failing and succeeding ones
    assert (ref[1][st == LIN] > 16).sum() >= 100 and (ref[1][st == NONLIN] > 32).sum() >= 100
    at_budgets(dev, BANK, hdr, ev, ref, budgets=(budget,))
