"""Deep searches at the edges of every stage's value and slot ranges.

Every case does two things with a batch of model-consistent histories (the
searches descend: tests/test_metamorphic.py pins the batches, the oracle and
how many histories carry a balance past i16 / int32):

* oracle parity -- status, nodes, witness and totals against the C oracle
  (`_compare` of test_gpu_parity.py);
* self-consistency -- where the batch is a transformation (tests/metamorph.py:
  S_k, A_pi, P_sigma) of a generated one, the device's own status, node and
  witness arrays equal its arrays on the untransformed batch, run at default
  knobs in the same test.  No oracle is involved in that half.

`probe()` reports four counts of the last call: histories stage 0 passed on
(deferred), stage 0's and stage 0w's heavy lists, and giants.  It does not
report the wide list (what stage 0w passed on), so in wave mode it cannot
separate a history searched by the wide launches from one the compact stages
finished; only `giants` tells where a wide history ended up, and the tests
assert exactly what follows from the code: lane mode sends the whole wide
list to the giant stage; wave mode hands a wide history on when it has more
than 8 pids, when an invocation value is at or beyond +-2^24 (wave.hip
kWideValue), or when its search passes the split cap, so for wide values
`giants` is bounded from below there.  It does not report
whether a lane-mode call was folded either (fold 1: no stage-0w launch after
a call that deferred nothing).
"""

import functools

import numpy as np
import pytest

from metamorph import relabel_accounts, relabel_pids, scale
from qsmd import codec, device, gen, models
from test_gpu_parity import _compare, knobs  # noqa: F401  (knobs: the fixture)
from test_metamorphic import (BANK_BATCHES, FIRST, K_I16, K_I32, MAX_NODES, PI, PI_SWAP, SIGMA_8, SIGMA_128, SIGMA_MIX,
                              assert_same, bank_batch, event_mask, ticket_batch)

pytestmark = pytest.mark.gpu

BANK = sorted(BANK_BATCHES)
# the heavy stage: wave mode; lane mode with HBM and with LDS memo tables,
# the memo joining every search at its first node
HEAVY = [pytest.param(dict(heavy_mode=0), id="wave"),
         pytest.param(dict(heavy_mode=1, memo_lds=0, memo_after=1), id="lane-hbm"),
         pytest.param(dict(heavy_mode=1, memo_lds=2, memo_after=1), id="lane-lds")]
I9_MIN, I9_MAX = -256, 255                    # lane.h IVAL_BITS 9
R25 = 1 << 24                                 # lane.h RVAL_BITS 25
WIDE_VALUE = 1 << 24                          # wave.hip kWideValue


def holds_wide(hdr, ev):
    """Per history: some value outside the compact event words (whatever the
    history's length)."""
    resp = (ev["kp"] & 0x80) != 0
    v = ev["val"].astype(np.int64)
    wide = np.where(resp, (v < -R25) | (v >= R25), (v < I9_MIN) | (v > I9_MAX))
    return np.add.reduceat(wide.astype(np.int64), hdr["ev_off"].astype(np.int64)) > 0


def beyond_stage0(hdr, ev):
    """Per history: stage 0 cannot hold it (over 32 events, over 8 pids, an
    invocation value outside 9 signed bits or a response value outside 25)."""
    return holds_wide(hdr, ev) | (hdr["n_ev"] > 32) | (hdr["n_pid"] > 8)


def host_entry_deferred(hdr, ev):
    """probe()'s `deferred` after a host-entry call: what stage 0 passed on,
    and 0 when no history fits stage 0, for the host entry then launches none
    (api.hip: the route from the headers; see through_stage0)."""
    fits = (hdr["n_ev"] <= 32) & (hdr["n_pid"] <= 8)
    return int(beyond_stage0(hdr, ev).sum()) if fits.any() else 0


def handed_off_for_value(hdr, ev):
    """Per history: an invocation value at or beyond +-2^24 (wave mode's wide
    launches hand it to the giant stage)."""
    inv = (ev["kp"] & 0x80) == 0
    v = ev["val"].astype(np.int64)
    big = inv & ((v >= WIDE_VALUE) | (v <= -WIDE_VALUE))
    return np.add.reduceat(big.astype(np.int64), hdr["ev_off"].astype(np.int64)) > 0


def through_stage0(ctx, mid, hdr, ev, got, max_nodes=MAX_NODES):
    """The host entry reads the headers and launches no stage 0 for a batch
    none of whose histories fits it (api.hip: the route), and `deferred` is
    then 0.  The device entry always launches stage 0, which must pass every
    such history on: run the batch there, compare status, nodes and witness
    with `got` (the host entry's), and return the probe."""
    torch = pytest.importorskip("torch")
    assert not ((hdr["n_ev"] <= 32) & (hdr["n_pid"] <= 8)).any()
    dev = torch.device("cuda:0")
    n = len(hdr)
    d_hdr = torch.from_numpy(np.array(hdr).view(np.uint8)).to(dev)
    d_ev = torch.from_numpy(np.array(ev).view(np.uint8)).to(dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nd = torch.empty(n, dtype=torch.int64, device=dev)
    d_w = torch.full((len(ev),), 0xFF, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.check_device(mid, d_hdr.data_ptr(), n, d_ev.data_ptr(), len(ev), d_st.data_ptr(), d_nd.data_ptr(),
                     d_w.data_ptr(), None, flags=device.QSMD_FLAG_EXHAUSTIVE | device.QSMD_FLAG_WITNESS,
                     max_nodes=max_nodes, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pr = ctx.probe()
    assert_same("device entry", (d_st.cpu().numpy(), d_nd.cpu().numpy().astype(np.uint64), d_w.cpu().numpy()),
                got, hdr)
    return pr


def baseline(ctx, name):
    """The untransformed batch on the device at the knobs in force (the
    defaults at a test's start), checked against the oracle."""
    hdr, ev, _, _, _ = bank_batch(name)
    return _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=MAX_NODES)


def clean_call(ctx):
    """A call that defers nothing, so a following lane-mode call may fold."""
    hdr, ev, _, _, _ = bank_batch("bank_4x16")
    ctx.check_arrays(models.MODEL_BANK, hdr[:2048], ev[:2048 * 32], max_nodes=MAX_NODES)
    pr = ctx.probe()
    assert pr["deferred"] == 0 and pr["heavy64"] == 0, pr


@functools.lru_cache(maxsize=None)
def money_batch(name, money_max):
    hdr, ev, _ = gen.generate_config(name, FIRST, BANK_BATCHES[name], money_max=money_max)
    for a in (hdr, ev):
        a.flags.writeable = False
    return hdr, ev


@pytest.mark.parametrize("heavy", HEAVY)
@pytest.mark.parametrize("budget", [0, 8, 32])
@pytest.mark.parametrize("money_max", [255, 256])
@pytest.mark.parametrize("name", BANK)
def test_field_edge(ctx, knobs, name, money_max, budget, heavy):
    """Stage 0 (bank_4x16, bank_4x16_bugs: G32) and stage 0w (bank_6x24: G64)
    with money drawn from 1..255 -- every invocation value fits the 9-bit
    field, up to its upper bound -- and from 1..256, where exactly the
    histories holding a 256 (about 1.6 %) leave the compact stages.  Budgets
    0 (the compact stage searches to the end), 8 (most histories go to the
    heavy stage, which resumes saved states whose balances reach 16 x 255 /
    32 x 255) and 32.
    Route, confirmed by probe(): `deferred` is the number of histories over
    32 events at money_max 255 and that plus the histories holding a 256 at
    money_max 256 (computed on the host) -- for bank_6x24 through the device
    entry, see through_stage0, the host entry's own count being 0; in lane mode the histories holding
    a 256 are the wide list and all reach the giant stage (`giants` at least
    their number; exactly their number at budget 0, where no heavy stage
    hands anything on); in wave mode the wide launches search them and the
    probe cannot tell."""
    hdr, ev = money_batch(name, money_max)
    inv = (ev["kp"] & 0x80) == 0
    assert int(ev["val"][inv].max()) == money_max
    knobs(stage0_budget=budget, stage0w_budget=budget, **heavy)
    got = _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=MAX_NODES)
    pr = ctx.probe()
    over32 = int((hdr["n_ev"] > 32).sum())
    n_wide = int(holds_wide(hdr, ev).sum())
    n_beyond = int(beyond_stage0(hdr, ev).sum())
    print(name, money_max, budget, heavy, pr, "over32", over32, "wide", n_wide)
    assert over32 in (0, len(hdr)) and n_beyond == (over32 if over32 else n_wide)
    if money_max == 255:
        assert n_wide == 0
    else:
        assert 0 < n_wide < len(hdr) // 20
    if heavy["heavy_mode"] == 1:
        assert pr["giants"] >= n_wide, pr
        if budget == 0:
            assert pr["giants"] == n_wide, pr
    if over32:                                     # (bank_6x24: the host entry launched no stage 0)
        assert pr["deferred"] == 0, pr
        pr = through_stage0(ctx, models.MODEL_BANK, hdr, ev, got)
        print("  device entry", pr)
    assert pr["deferred"] == n_beyond, pr


@pytest.mark.parametrize("bal", [24575, 24576, -24575, -24576, 200000])
@pytest.mark.parametrize("lds", [0, 2])
def test_lane_mode_key_range_g64(ctx, knobs, bal, lds):
    """memo.hip keys_fit for G64: lane mode keys balances as i16, a 64-event
    history has at most 32 operations of at most 256 each, so a model0
    within +-(32767 - 256 x 32) = +-24575 keeps every reachable state keyable
    and the memo runs; beyond it the memo is off for the call.  Exact either
    way, with HBM and LDS tables, on bank_6x24 with money up to 255 at a
    stage-0w budget of 8 (nearly every history resumes in the heavy stage).
    The model0 balance sits on account 6 (7 on account 7), which no generated
    history opens, so the searches stay deep: with bal >= 0 the device's
    arrays equal its arrays without a model0 (an untouched account changes
    nothing); with bal < 0 the invariant fails at the first node of every
    history (NONLIN, 1 node: the root has one candidate, the first operation
    of the sequential prefix).  (test_lane_mode_key_range's model0 makes the
    accounts the histories open exist already, so its searches end at their
    first OpenAccount.)"""
    hdr, ev = money_batch("bank_6x24", 255)
    knobs(heavy_mode=1, memo_lds=lds, stage0_budget=8, stage0w_budget=8, memo_after=1)
    want = _compare(ctx, models.MODEL_BANK, hdr, ev, max_nodes=MAX_NODES)
    assert ctx.probe()["heavy64"] > len(hdr) // 2
    m0 = models.BankModel(0b11000000, 0, (0, 0, 0, 0, 0, 0, bal, 7))
    st, nd, w = _compare(ctx, models.MODEL_BANK, hdr, ev, m0, max_nodes=MAX_NODES)
    if bal >= 0:
        assert_same("model0 on untouched accounts", (st, nd, w), want, hdr)
        assert ctx.probe()["heavy64"] > len(hdr) // 2
    else:
        assert (st == codec.STATUS_NONLIN).all() and (nd == 1).all()


@pytest.mark.parametrize("k", [64, K_I16, 2621, 167772, 167773, K_I32])
@pytest.mark.parametrize("name", BANK)
def test_scaled_values_down_the_wide_list(ctx, knobs, name, k):
    """S_k with every history beyond the compact stages' event words: k = 64
    (no balance on a witness passes i16), 128 (over 100 do: wave mode's i16
    memo keys must not record them), 2621, 167772 (100 k = 16,777,200 < 2^24:
    the last k whose values all stay in wave mode's wide launches), 167773
    (a value of 100 becomes 16,777,300 >= 2^24: those histories are handed to
    the giant stage) and 21474836 (every value is >= 2^24, thousands of
    witnesses take a balance past INT32_MAX; the 10-16 % of histories with a
    value past int32 are dropped, the rest stay packed).
    Routes: wave mode with the state DAG (dag_states 128) and without (0):
    stage 0 / 0w -> wide list -> wide launches -> (handed off) giant stage;
    lane mode: wide list -> giant stage, unfolded (fold 0) and folded (fold 1
    after a call that deferred nothing: stage 0 -> giant stage, no stage 0w).
    probe(): `deferred` is every history that holds money (over 99 % of
    them: a scaled value is outside the 9-bit field; for bank_6x24 every
    history, counted through the device entry); `giants` is exactly those in
    lane mode, and at least the histories with an
    invocation value >= 2^24 in wave mode (at k = 21474836 all but at most 5
    of them; at k = 167773 those holding a 100, about 1 in 20 -- the hand-off
    is per history; below: no lower bound).  The probe cannot tell wave mode's wide launches from the
    compact stages, nor a folded call from an unfolded one."""
    hdr, ev, _, _, _ = bank_batch(name)
    st0, nd0, w0 = baseline(ctx, name)
    h2, e2, _, keep = scale(hdr, ev, k)
    want = (st0[keep], nd0[keep], w0[event_mask(hdr, keep)])
    n = len(h2)
    assert keep.all() if k < K_I32 else n >= len(hdr) * 4 // 5
    # (a history with no money in it -- OpenAccount and CheckBalance of empty
    # accounts only -- is its own image and stays in the compact stages)
    n_beyond, n_wide = int(beyond_stage0(h2, e2).sum()), int(holds_wide(h2, e2).sum())
    assert n_wide >= n * 99 // 100 and n_beyond == (n if name == "bank_6x24" else n_wide)
    big = int(handed_off_for_value(h2, e2).sum())
    if k <= 167772:
        assert big == 0
    elif k == K_I32:                               # (all but the few whose only money is a planted Balance)
        assert n_wide - 5 <= big <= n_wide
    else:
        assert 0 < big < n_wide
    for kn in (dict(heavy_mode=0, dag_states=128), dict(heavy_mode=0, dag_states=0),
               dict(heavy_mode=1, memo_lds=0, fold=1), dict(heavy_mode=1, memo_lds=0, fold=0)):
        knobs(**kn)
        if kn.get("fold"):
            clean_call(ctx)
        got = _compare(ctx, models.MODEL_BANK, h2, e2, max_nodes=MAX_NODES)
        pr = ctx.probe()
        print(name, k, kn, pr, "n", n, "wide", n_wide, "big", big)
        assert_same(f"S_{k} {kn}", got, want, h2)
        if name == "bank_6x24":                    # (no history fits stage 0: see through_stage0)
            assert pr["deferred"] == 0, (kn, pr)
        if kn["heavy_mode"] == 1:
            assert pr["giants"] == n_wide, (kn, pr)
        else:
            assert big <= pr["giants"] <= n_wide, (kn, pr)
        if name == "bank_6x24":
            pr = through_stage0(ctx, models.MODEL_BANK, h2, e2, got)
            print("  device entry", pr)
        assert pr["deferred"] == n_beyond, (kn, pr)


TRANSFORMS = {
    "A_pi": lambda hdr, ev: (hdr, relabel_accounts(ev, PI)[0]),
    "A_swap": lambda hdr, ev: (hdr, relabel_accounts(ev, PI_SWAP)[0]),
    "P_4to7": lambda hdr, ev: relabel_pids(hdr, ev, SIGMA_8),
    "P_128": lambda hdr, ev: relabel_pids(hdr, ev, SIGMA_128),
    "P_mix": lambda hdr, ev: relabel_pids(hdr, ev, SIGMA_MIX),
}


@pytest.mark.parametrize("heavy", HEAVY)
@pytest.mark.parametrize("budget", [0, 8])
@pytest.mark.parametrize("tr", sorted(TRANSFORMS))
@pytest.mark.parametrize("name", BANK)
def test_high_slots(ctx, knobs, name, tr, budget, heavy):
    """Accounts and pids in the slots the generated batches never use.
    A_pi ([5,2,7,0,6,1,3,4]) and A_swap (0..3 <-> 4..7) put deep searches on
    account slots 4..7 (the [account][lane] balances, LaneDFS::fold's rotate
    by 4 x account, the i16-pair memo keys); P_4to7 ([7,4,6,5,3,2,1,0],
    n_pid 8) puts the 4-client batches' pids on 4..7, P_mix ([1,5,2,6,0,4,3,7])
    on pairs that differ in pid bit 2 alone; both stay in the compact
    stages (`deferred` 0 and no giants, as untransformed: bank_6x24's 48-event
    histories never see stage 0 through the host entry);
    P_128 ([100,9,64,127,31,8,15,16], n_pid 128) takes every history past the
    compact stages for its pid count, and a history of more than 8 pids is
    the giant stage's in both heavy modes (wave.hip: the wide launches pass
    it on; `giants` = every history).  Stage budgets 0 and 8 (the heavy stage resumes the saved
    states) in both heavy modes."""
    hdr, ev, _, _, _ = bank_batch(name)
    want = baseline(ctx, name)
    h2, e2 = TRANSFORMS[tr](hdr, ev)
    knobs(stage0_budget=budget, stage0w_budget=budget, **heavy)
    got = _compare(ctx, models.MODEL_BANK, h2, e2, max_nodes=MAX_NODES)
    pr = ctx.probe()
    print(name, tr, budget, heavy, pr)
    assert_same(tr, got, want, hdr)
    if tr == "P_128":
        assert pr["giants"] == len(hdr), pr
    else:
        assert pr["deferred"] == host_entry_deferred(h2, e2) and pr["giants"] == 0, pr
        if budget == 8:
            assert pr["heavy32"] + pr["heavy64"] > len(hdr) // 2, pr


@pytest.mark.parametrize("name", BANK)
def test_composition(ctx, knobs, name):
    """A_pi . P_sigma . S_2 once per batch: with sigma into 4..7 everything
    stays in the compact stages (values up to 200 fit the 9-bit field) at a
    stage budget of 8 in lane and wave mode (no giants); with sigma into
    scattered pids (n_pid 128) every history is the giant stage's."""
    hdr, ev, _, _, _ = bank_batch(name)
    want = baseline(ctx, name)
    for sigma in (SIGMA_8, SIGMA_128):
        h2, e2, _, keep = scale(hdr, ev, 2)
        assert keep.all()
        h2, e2 = relabel_pids(h2, e2, sigma)
        e2, _ = relabel_accounts(e2, PI)
        for heavy in (0, 1):
            knobs(stage0_budget=8, stage0w_budget=8, heavy_mode=heavy, memo_lds=0, memo_after=1)
            got = _compare(ctx, models.MODEL_BANK, h2, e2, max_nodes=MAX_NODES)
            pr = ctx.probe()
            print(name, sigma, heavy, pr)
            assert_same("A.P.S", got, want, hdr)
            if sigma is SIGMA_8:
                assert pr["deferred"] == host_entry_deferred(h2, e2) and pr["giants"] == 0, pr
            else:
                assert pr["giants"] == len(hdr), pr


@pytest.mark.parametrize("heavy", [0, 1])
@pytest.mark.parametrize("budget", [8, 32])
@pytest.mark.parametrize("name,sigmas", [("ticket_2x10", ([5], [100])), ("ticket_8x32", (SIGMA_8,))])
def test_ticket_pids(ctx, knobs, name, sigmas, budget, heavy):
    """P_sigma on TicketDispenser: ticket_2x10's one shared pid 0 -> 5 (stage
    0) and -> 100 (n_pid 101: the giant stage's, every history), and the 8-pid,
    64-event batch (stage 0w and the heavy stage; lin, nonlin and BUDGET at
    max_nodes 10^6) under a permutation of 0..7."""
    hdr, ev, _, _, _, max_nodes = ticket_batch(name)
    want = _compare(ctx, models.MODEL_TICKET, hdr, ev, max_nodes=max_nodes)
    knobs(stage0_budget=budget, stage0w_budget=budget, heavy_mode=heavy, memo_lds=0, memo_after=1)
    for sigma in sigmas:
        h2, e2 = relabel_pids(hdr, ev, sigma)
        got = _compare(ctx, models.MODEL_TICKET, h2, e2, max_nodes=max_nodes)
        pr = ctx.probe()
        print(name, sigma, budget, heavy, pr)
        assert_same("P_sigma", got, want, hdr)
        assert pr["giants"] == (len(hdr) if max(sigma) >= 8 else 0), pr
