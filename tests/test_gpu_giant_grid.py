"""The giant stage's grid sized by what a call is expected to hold.

After a finished call without giants, deferred or wide histories the next
call's giant stage runs on one workgroup (api.hip, `kGiantIdleGrid`), on lane
mode's folded route too.  The stage takes its work from queues, so a call
that has giants after all must give the oracle's results on that grid; its
probe then puts the next call back on two workgroups per CU, and a giant-free
call after that brings the grid down again.  The yardstick for every status
and node count is the C oracle (oracle/oracle_c.py); a fresh context forced
to `giant_grid` 512 must agree, totals included.
"""

import random

import numpy as np
import pytest

import histgen
import oracle_c
from qsmd import codec, device, gen, models

pytestmark = pytest.mark.gpu

MAX_NODES = 10**6
ORDINARY = {"bank": "bank_4x16", "ticket": "ticket_2x10"}


def _concat(*parts):
    hs, es, off = [], [], 0
    for hdr, ev in parts:
        h = hdr.copy()
        h["ev_off"] += off
        hs.append(h)
        es.append(ev)
        off += len(ev)
    return np.concatenate(hs), np.concatenate(es)


def _sequential(rng, model, n_ops, big=False):
    """One pid, n_ops operations one after the other: one candidate per step."""
    h = []
    for _ in range(n_ops):
        if model == "ticket":
            h.append(("p0", ("L", rng.choice(histgen.TICKET_INV))))
            h.append(("p0", ("R", ("Number", rng.randint(300, 5000) if big else rng.randint(0, 3)))))
        else:
            h.append(("p0", ("L", ("Deposit", "p0", rng.randint(300, 5000) if big else rng.randint(1, 9)))))
            h.append(("p0", ("R", "DepositMade")))
    return h


def _nine_pids(rng, model):
    """9 pids with 2 operations each, interleaved at random (36 events)."""
    pids = [f"p{i}" for i in range(9)]
    todo = {p: 4 for p in pids}                 # events left: L R L R
    h = []
    while todo:
        p = rng.choice(sorted(todo))
        want = "L" if todo[p] % 2 == 0 else "R"
        ev = histgen.ticket_event(rng) if model == "ticket" else histgen.bank_event(rng, pids[:6])
        while ev[0] != want:
            ev = histgen.ticket_event(rng) if model == "ticket" else histgen.bank_event(rng, pids[:6])
        h.append((p, ev))
        todo[p] -= 1
        if not todo[p]:
            del todo[p]
    return h


def _outside_9_bits(rng, model, n_ev):
    """33..40 events on up to 8 pids with values the 9-bit field cannot hold."""
    h = histgen.wellformed_history(rng, model, n_ev // 2, rng.randint(2, 8), p_pending=0.0)
    out = []
    for pid, (kind, x) in h:
        if model == "bank" and kind == "L" and x[0] in ("Deposit", "Withdraw"):
            x = (x[0], x[1], x[2] + 1000)
        elif model == "bank" and kind == "L" and x[0] == "Transfer":
            x = (x[0], x[1], x[2] + 1000, x[3])
        elif model == "ticket" and kind == "R" and isinstance(x, tuple):
            x = ("Number", x[1] + 1000)
        out.append((pid, (kind, x)))
    return out


def _batches(model):
    """(call 1 / 3 / 4: no giant; call 2: the mix), as (hdr, events)."""
    rng = random.Random(41 if model == "bank" else 43)
    m = models.BY_NAME[model]
    clean = gen.generate_config(ORDINARY[model], 7, 128)[:2]
    ordinary = gen.generate_config(ORDINARY[model], 11, 100)[:2]
    hs = [_nine_pids(rng, model) for _ in range(48)]
    hs += [_outside_9_bits(rng, model, rng.randint(33, 40)) for _ in range(8)]
    hs += [_sequential(rng, model, rng.randint(17, 20), big=True) for _ in range(4)]           # 34..40 events
    hs += [_sequential(rng, model, rng.randint(33, 60)) for _ in range(6)]                     # over 64 events
    rng.shuffle(hs)
    rest = codec.encode(m, hs)
    assert not rest.encode_errors
    return clean, _concat(ordinary, (rest.hdr, rest.events))


_ORACLE = {}


def _oracle(model, key, hdr, ev):
    if (model, key) not in _ORACLE:
        _ORACLE[model, key] = oracle_c.check_batch(models.BY_NAME[model].model_id, hdr, ev, None, MAX_NODES, 8)[:2]
    return _ORACLE[model, key]


def _lane_context(**params):
    c = device.Context(0, time_limit_ms=60000)
    for k, v in dict(heavy_mode=1, memo_lds=0, **params).items():
        c.set_param(k, v)
    return c


def _check(c, model, key, hdr, ev):
    st, nd, _, tot = c.check_arrays(models.BY_NAME[model].model_id, hdr, ev, max_nodes=MAX_NODES)
    st_o, nd_o = _oracle(model, key, hdr, ev)
    bad = np.nonzero((st != st_o) | (nd != nd_o))[0]
    assert len(bad) == 0, (key, len(bad), bad[:5], st[bad[:5]], nd[bad[:5]], st_o[bad[:5]], nd_o[bad[:5]])
    assert tot["checked"] == len(hdr) and tot["nodes"] == int(nd_o.sum())
    assert tot["linearisable"] == int((st_o == 1).sum()) and tot["nonlinearisable"] == int((st_o == 0).sum())
    assert tot["model_errors"] == int((st_o == 2).sum())
    return st, nd, tot


@pytest.mark.parametrize("model", ["bank", "ticket"])
def test_giants_on_the_idle_grid(model):
    clean, mix = _batches(model)
    c, big = _lane_context(), _lane_context(giant_grid=512)
    try:
        # call 1: no probe yet -- two workgroups per CU as before; no giant, nothing deferred
        _check(c, model, "clean", *clean)
        up = c.get_param("giant_grid_last")
        assert up > 64 and up % 2 == 0, up
        p1 = c.probe()
        assert p1["deferred"] == 0 and p1["heavy64"] == 0 and p1["giants"] == 0, p1
        # call 2: nothing expected, the folded route, one workgroup -- and giants after all
        st, nd, tot = _check(c, model, "mix", *mix)
        assert c.get_param("giant_grid_last") == 1
        p = c.probe()
        assert p["deferred"] == 66 and p["giants"] >= 54, p
        # ... the same on a fresh context forced to 512 workgroups
        _check(big, model, "clean", *clean)
        st_b, nd_b, tot_b = _check(big, model, "mix", *mix)
        assert big.get_param("giant_grid_last") == 512
        assert np.array_equal(st, st_b) and np.array_equal(nd, nd_b) and tot == tot_b
        assert big.probe() == p
        # call 3: after giants, two workgroups per CU; call 4: down again
        _check(c, model, "clean", *clean)
        assert c.get_param("giant_grid_last") == up
        assert c.probe()["giants"] == 0 and c.probe()["deferred"] == 0
        _check(c, model, "clean", *clean)
        assert c.get_param("giant_grid_last") == 1
        # ... and the mix once more at the full grid's hint (call 5 runs on 1, call 6 on 2 per CU)
        _check(c, model, "mix", *mix)
        _check(c, model, "mix", *mix)
        assert c.get_param("giant_grid_last") == up
    finally:
        c.close()
        big.close()


def test_early_exit_grid_unchanged():
    """An early-exit call after a giant-free call keeps its own rule: one
    workgroup per fixup chunk, at least 8."""
    clean, _ = _batches("bank")
    hdr, ev0, _ = gen.generate_config("bank_4x16", 3, 2000)
    cut = 1200
    ev = gen.plant_failure(hdr, ev0, cut)
    st_o, nd_o = _oracle("bank", "planted", hdr, ev)
    assert st_o[cut] == codec.STATUS_NONLIN and (st_o[:cut] == codec.STATUS_LIN).all()
    c = _lane_context()
    try:
        _check(c, "bank", "clean", *clean)
        st, nd, _, tot = c.check_arrays(models.MODEL_BANK, hdr, ev, max_nodes=MAX_NODES,
                                        flags=device.QSMD_FLAG_EXHAUSTIVE | device.QSMD_FLAG_EARLY_EXIT_BATCH)
        assert c.get_param("giant_grid_last") == 8
        m = cut + 1
        assert np.array_equal(st[:m], st_o[:m]) and np.array_equal(nd[:m], nd_o[:m])
        assert (st[m:] == codec.STATUS_SKIPPED).all()
        assert tot["skipped"] == len(hdr) - m and tot["nodes"] == int(nd_o[:m].sum())
        # the next ordinary call: the early-exit call had no giant either -- one workgroup
        _check(c, "bank", "clean", *clean)
        assert c.get_param("giant_grid_last") == 1
    finally:
        c.close()
