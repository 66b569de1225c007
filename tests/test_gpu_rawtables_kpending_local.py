"""GPU parity of the keyed pending call's local mode (knob "kpending_local":
csrc/ksplit.hip's pending split, csrc/kpending.hip over the sub-headers,
ksplit_combine) on random raw tables whose responses move the state
(tests/rawtables.py), against the literal restatement
(tests/kpendinglocal_ref.py with closures that read the raw arrays).

tests/test_gpu_kpending_local.py runs the mode on named models only: identity
``on_resp``, one allowed response per (state, invocation), no table bit at or
above ``n_resp``.  Here an assumed response moves a key's state through the
fourth table, a pending invocation chooses among several allowed symbols, the
allowed word carries garbage above ``n_resp`` and bits post_err removes (rule 2
on a part whose only would-be children are such bits), parts pass pass 1's 256
nodes, and a `budget` part enters the combine rule
(tests/test_rawtables_host.py asserts all of that on the restatement alone).

Every comparison is exact -- status, node count, the eight totals,
"kpending_local_last" -- and no history is left out: the device runs with the
restatement's max_nodes, and a `budget` must match with its node count.
Through the host and the device entry, at `table_budget` 256, 0 and 4."""

import numpy as np
import pytest

import kpendinglocal_ref as klr
import ktablelocal_ref as kref
import pending_ref as pr
import rawtables as rt
from qsmd import codec, device
from qsmd.linearisability import linearisable_batch
from test_gpu_kpending_local import (BUDGETS, CODE, EXH, MAXN, assert_equal, check_local, expected, knobs,
                                     run_device, run_host, set_table)
from test_gpu_ktable_pending import assert_results as assert_pending5
from test_gpu_ktable_pending import run_host as run_pending_host5
from test_gpu_table_pending import budget_knob

pytestmark = pytest.mark.gpu

assert MAXN == rt.MAX_NODES and BUDGETS == (256, 0, 4)
CRASHED = ["k_max", "k_deep", "k_odd", "k_one", "k2_deep", "k2_r32"]
TWO_KEYS = ["k2_deep", "k2_r32"]
SETTINGS = list(rt.BATCHES)
NAME = {v: k for k, v in CODE.items()}


@pytest.fixture(scope="module")
def ctx():
    """This module's own context (a keyed table, once set, cannot be taken
    away: see test_gpu_ktable.py)."""
    c = device.Context(0, time_limit_ms=60000)
    assert c.get_param("table_budget") == BUDGETS[0]
    yield c
    c.close()


def encode(name, hists):
    batch = codec.encode(rt.model(name), [list(h) for h in hists], rt.model0_of(name))
    assert not batch.encode_errors
    return batch.hdr, batch.events


def codes(combined):
    return [(CODE[st], nd) for st, nd in combined]


def flat(parts):
    """The parts of a batch as one list of (status, nodes)."""
    return [(st, nd) for p in parts for _, st, nd in p]


def local_both(ctx, name, hdr, ev, want, n_split, parts=None, max_nodes=MAXN, budgets=BUDGETS):
    """Knob 1 through the host and the device entry at every budget against
    ``want``; with ``parts`` (every history split), pass 2 took the parts the
    per-part results predict."""
    m, model0 = rt.model(name), rt.model0_of(name)
    counts = {}
    for budget in budgets:
        with budget_knob(ctx, budget):
            st, nd, w, asm, tot, split = run_host(ctx, m, None, hdr, ev, 1, max_nodes, model0)
            pass2 = ctx.table_pass2()
            assert w is None and asm is None
            assert_equal(want, n_split, st, nd, tot, split)
            std, ndd, _, _, totd, splitd = run_device(ctx, m, None, hdr, ev, 1, max_nodes=max_nodes, model0=model0)
            assert_equal(want, n_split, std, ndd, totd, splitd)
            if parts is not None:
                assert pass2 == ctx.table_pass2() == rt.pass2_expected(flat(parts), budget), budget
            counts[budget] = pass2
    return counts


# ---------------------------------------------------------- 1. crashed batches

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", CRASHED)
def test_crashed_batches(ctx, name, setting):
    comp, K, model0 = rt.keyed_spec(name)
    hists, parts, combined, _ = rt.local_crash_case(name, setting)
    assert all(p is not None for p in parts)
    hdr, ev = encode(name, hists)
    want = codes(combined)
    # the restatement on the arrays is the restatement on the histories
    assert expected(ctx, rt.model(name), None, hdr, ev, MAXN, model0, rt.closures(comp)) == (want, len(hists))
    counts = local_both(ctx, name, hdr, ev, want, len(hists), parts)
    beyond = sum(1 for _, nd in flat(parts) if nd > 256)
    print(name, setting, "parts:", len(flat(parts)), "beyond 256 nodes:", beyond, "pass 2 took:", counts)
    assert counts[0] == 0 and counts[256] >= beyond
    if name == "k_max":         # the only per-key start vector with state 255; response bit 31 is a symbol
        assert model0 == (255, 0, 17, 255, 128, 3, 254, 1) and rt.spec(comp).nr == 32
    assert not ctx.timed_out()


# ----------------------------------------------------------- 2. a low max_nodes

@pytest.mark.parametrize("name", TWO_KEYS)
def test_low_max_nodes(ctx, name):
    """`budget` parts in the combine rule: deciding, behind a lower failing
    key, and sums beyond max_nodes.  At `table_budget` 4 the search is tiered,
    at 256 (above the limit) it is not; the arrays are the same."""
    low = rt.LOW_NODES
    seen = set()
    for setting in SETTINGS:
        hists, parts, combined, _ = rt.local_crash_case(name, setting, low)
        hdr, ev = encode(name, hists)
        counts = local_both(ctx, name, hdr, ev, codes(combined), len(hists), parts, max_nodes=low)
        assert counts[256] == counts[0] == 0
        print(name, setting, "pass 2 at budget 4 took:", counts[4])
        for p, (status, nodes) in zip(parts, combined):
            sts = [st for _, st, _ in p]
            if status == "budget":
                seen.add("decides")
            elif "budget" in sts:
                seen.add("behind")
            if nodes > low:
                seen.add("beyond")
    assert seen == {"decides", "behind", "beyond"}
    assert not ctx.timed_out()


# ---------------------------------------------------------- 3. against knob 0

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", CRASHED)
def test_knob_0_is_the_product(ctx, name, setting):
    """The same batches with the knob off: the product's results
    (pending_ref on the product closures), nothing split; and wherever the
    product decides, the local verdict agrees up to the {error, nonlin} swap."""
    m, model0 = rt.model(name), rt.model0_of(name)
    hists, ref = rt.crash_case(name, setting)
    assert hists is rt.local_crash_case(name, setting)[0]
    batch, st, nd, w, asm, tot = run_pending_host5(ctx, m, hists, model0)
    assert ctx.kpending_local_last() == 0
    assert_pending5(m, hists, ref, st, nd, w, asm, batch.hdr, tot, MAXN, model0)
    st0, nd0, _, _, tot0, split0 = run_host(ctx, m, None, batch.hdr, batch.events, 0, MAXN, model0)
    assert np.array_equal(st0, st) and np.array_equal(nd0, nd) and tot0 == tot and split0 == 0
    st1, _, _, _, _, split1 = run_host(ctx, m, None, batch.hdr, batch.events, 1, MAXN, model0)
    assert split1 == len(hists)
    decided = 0
    for whole, local in zip(st0, st1):
        whole, local = NAME[int(whole)], NAME[int(local)]
        if whole == "budget":
            decided += local != "budget"
        else:
            assert whole == local or {whole, local} == {"error", "nonlin"}, (whole, local)
    print(name, setting, "product budget decided key by key:", decided)
    assert not ctx.timed_out()


def test_a_product_error_that_is_lin_key_by_key(ctx):
    """rawtables.ERROR_LIN_KAT: the one kind of disagreement the batches above
    do not hold, in both modes."""
    m = rt.model("k2_r32")
    hdr, ev = encode("k2_r32", [rt.ERROR_LIN_KAT])
    for budget in BUDGETS:
        with budget_knob(ctx, budget):
            st, nd, _, _, _, split = run_host(ctx, m, None, hdr, ev, 0)
            assert (NAME[int(st[0])], int(nd[0]), split) == ("error", 20, 0)
    assert check_local(ctx, m, None, hdr, ev, closures=rt.closures("n_r32")) == ([(CODE["lin"], 20)], 1)
    assert not ctx.timed_out()


# -------------------------------------------------------------------- 4. walks

@pytest.mark.parametrize("name", ["k8_1inv", "k8_r2"])
def test_walks(ctx, name):
    """128 pids with a pending invocation each, 16 per key, several symbols
    allowed at every level and bits at and above n_resp in every allowed word
    (the history in the widest class, its parts in the narrowest); a short walk
    with one failing key; rule 2 where the allowed word is empty only after
    the cut and post_err."""
    comp, K, model0 = rt.keyed_spec(name)
    m = rt.model(name)
    hists, parts, combined, product = rt.walk_case(name)
    assert len(hists[0]) == 128 and all(len(sub) == 16 for _, sub in klr.split(rt.closures(comp), K, hists[0]))
    assert combined[0] == ("lin", 128) and combined[1][0] == "nonlin"
    if name == "k8_r2":
        assert len(hists) > 2 and ("lin", 0) in combined[2:]
    hdr, ev = encode(name, hists)
    assert expected(ctx, m, None, hdr, ev, MAXN, model0, rt.closures(comp)) == (codes(combined), len(hists))
    local_both(ctx, name, hdr, ev, codes(combined), len(hists), parts)
    assert ctx.kpending_local_last() == len(hists)
    # knob 0: the product
    batch, st, nd, w, asm, tot = run_pending_host5(ctx, m, hists, model0)
    assert ctx.kpending_local_last() == 0
    assert_pending5(m, hists, product, st, nd, w, asm, batch.hdr, tot, MAXN, model0)
    assert not ctx.timed_out()


# -------------------------------------------------------- 5. complete histories

@pytest.mark.parametrize("name", ["k_deep", "k_odd", "k_max"])
def test_complete_histories_equal_the_local_check_call(ctx, name):
    comp, K, model0 = rt.keyed_spec(name)
    m, c = rt.model(name), rt.closures(comp)
    for setting in SETTINGS:
        hists, _ = rt.check_case(name, setting)
        assert not any(pr.pending_invocations(h) for h in hists)
        hdr, ev = encode(name, hists)
        want = kref.check_arrays(c, K, hdr, ev, MAXN, model0)
        assert all(x is not None for x in want)
        want = codes(want)
        set_table(ctx, m, None)
        packed = m.pack_model0(model0, {})
        for budget in BUDGETS:
            with budget_knob(ctx, budget):
                with knobs(ctx, ktable_local=1):
                    st0, nd0, _, tot0 = ctx.check_arrays(5, hdr, ev, packed, EXH, MAXN)
                    split0 = ctx.ktable_local_last()
                st, nd, _, _, tot, split = run_host(ctx, m, None, hdr, ev, 1, MAXN, model0)
                assert np.array_equal(st, st0) and np.array_equal(nd, nd0) and tot == tot0
                assert split == split0 == len(hists)
                std, ndd, _, _, totd, splitd = run_device(ctx, m, None, hdr, ev, 1, model0=model0)
                assert np.array_equal(std, st0) and np.array_equal(ndd, nd0) and totd == tot0 and splitd == len(hists)
                assert_equal(want, len(hists), st, nd, tot, split)
    assert not ctx.timed_out()


# ---------------------------------------------------------------- 6. any shape

@pytest.mark.parametrize("setting", list(rt.ANY_SETTINGS))
def test_anyshape(ctx, setting):
    """Ill-formed and shared-pid histories, and the same with clients
    crashed: the ones the restatement splits against it, the others against
    the knob-0 call on the same batch."""
    import random
    name = "k_odd"
    comp, K, model0 = rt.keyed_spec(name)
    some = rt.anyshape_case(name, setting)[0]
    rng = random.Random(f"rawtables/kpending-local/anyshape/{setting}")
    hists = list(some) + [pr.crash(h, rng, rt.CRASH) for h in some]
    hdr, ev = encode(name, hists)
    m, c = rt.model(name), rt.closures(comp)
    want, n_split = expected(ctx, m, None, hdr, ev, MAXN, model0, c)
    assert n_split == sum(1 for h in hists if klr.split(c, K, h) is not None)
    # both kinds of history, and split ones that end a pid on an invocation
    assert n_split >= 10 and len(hists) - n_split >= 10
    assert sum(1 for h in hists if klr.split(c, K, h) is not None and pr.pending_invocations(h)) >= 5
    local_both(ctx, name, hdr, ev, want, n_split)
    assert not ctx.timed_out()


# ------------------------------------------- 7. replacing tables between calls

def test_replacing_tables_between_calls(ctx):
    """A smaller component after the 80 KB one, a workspace that shrinks and
    grows: nothing of the previous table or split is read."""
    for name in ("k_max", "k8_r2", "k_one", "k_max", "k_odd"):
        hists, parts, combined, _ = rt.local_crash_case(name, "3x10")
        assert all(p is not None for p in parts)
        local_both(ctx, name, *encode(name, hists), codes(combined), len(hists), parts, budgets=(256,))
        assert ctx.keyed_table is rt.model(name)
    assert not ctx.timed_out()


# ------------------------------------------------------------------ 8. drop-in

def test_drop_in(ctx):
    hists, _, combined, _ = rt.local_crash_case("k2_r32", "4x16")
    res = linearisable_batch(rt.model("k2_r32"), hists, ctx=ctx, pending="complete", kpending_local=True,
                             max_nodes=MAXN)
    assert [(res.verdict(i), int(res.nodes[i])) for i in range(len(hists))] == combined
    assert ctx.kpending_local_last() == len(hists) and ctx.get_param("kpending_local") == 0
    assert len({st for st, _ in combined}) >= 3
    assert not ctx.timed_out()
