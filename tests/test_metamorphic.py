"""The three metamorphic relations of tests/metamorph.py on the CPU oracles.

S_k (scale), A_pi (account relabelling) and P_sigma (pid relabelling) leave
the reference's search tree isomorphic, so the C oracle (oracle/ref_cpu.c)
must return the same status, node count and witness for a transformed batch
as for the original.  tests/test_gpu_metamorphic.py asks the same of the
device; this file pins the oracle first, and asserts the conditions that give
the GPU tests their teeth (how many histories really carry a balance past
int32 / i16 once scaled).

Batches: bank_4x16 and bank_4x16_bugs (20000 histories), bank_6x24 (3000),
all from history index 5 with max_nodes 10**7; ticket_2x10 (5000) and
ticket_8x64 cut to 32 operations with p_bug 0.5 (2000, max_nodes 10**6: 8
pids, 64 events, lin / nonlin / BUDGET all present).
"""

import functools

import numpy as np
import pytest

import linearise_lists as LL
import oracle_c
from metamorph import I32_MAX, max_balance_on_witness, relabel_accounts, relabel_pids, scale
from qsmd import codec, gen, models

BANK_BATCHES = {"bank_4x16": 20000, "bank_4x16_bugs": 20000, "bank_6x24": 3000}
FIRST = 5
MAX_NODES = 10**7
K_I16 = 128                                  # the smallest round k with >= 100 histories past i16 (test_teeth_i16)
K_I32 = 21474836                             # floor((2^31 - 1) / 100)
SCALES = [2, 3, 81, 82, K_I16, 2621, 167772, 167773, K_I32]
PI = [5, 2, 7, 0, 6, 1, 3, 4]
PI_SWAP = [4, 5, 6, 7, 0, 1, 2, 3]           # 0..3 <-> 4..7
SIGMA_8 = [7, 4, 6, 5, 3, 2, 1, 0]           # n_pid 8
SIGMA_128 = [100, 9, 64, 127, 31, 8, 15, 16]  # n_pid 128
SIGMA_MIX = [1, 5, 2, 6, 0, 4, 3, 7]         # n_pid 8: pids that differ in bit 2 alone (1 / 5, 2 / 6, 0 / 4)
TICKET_BATCHES = {"ticket_2x10": (5000, {}, MAX_NODES),
                  "ticket_8x32": (2000, dict(n_ops=32, p_bug=0.5), 10**6)}


@functools.lru_cache(maxsize=None)
def bank_batch(name):
    """(hdr, ev, status, nodes, witness) of a Bank batch and the C oracle."""
    hdr, ev, _ = gen.generate_config(name, FIRST, BANK_BATCHES[name])
    st, nd, w = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, None, MAX_NODES, 8, witness=True)
    for a in (hdr, ev, st, nd, w):
        a.flags.writeable = False
    return hdr, ev, st, nd, w


@functools.lru_cache(maxsize=None)
def ticket_batch(name):
    n, over, max_nodes = TICKET_BATCHES[name]
    hdr, ev, _ = gen.generate_config("ticket_8x64" if name == "ticket_8x32" else name, FIRST, n, **over)
    st, nd, w = oracle_c.check_batch(models.MODEL_TICKET, hdr, ev, None, max_nodes, 8, witness=True)
    for a in (hdr, ev, st, nd, w):
        a.flags.writeable = False
    return hdr, ev, st, nd, w, max_nodes


@functools.lru_cache(maxsize=None)
def witness_peak(name):
    """Per history of a Bank batch: the largest balance on the oracle's
    witness path, unscaled (-1 for a history that is not linearisable).  The
    peak after S_k is k times it."""
    hdr, ev, st, _, w = bank_batch(name)
    peak = np.array(max_balance_on_witness(hdr, ev, w), dtype=np.int64)
    peak[st != codec.STATUS_LIN] = -1
    return peak


def event_mask(hdr, keep):
    return np.repeat(keep, hdr["n_ev"].astype(np.int64))


def assert_same(name, got, want, hdr_t):
    """Status and nodes equal; the witness equal over every linearisable
    history's events (histories are back to back in header order)."""
    st, nd, w = got
    st0, nd0, w0 = want
    assert np.array_equal(st, st0), f"{name}: {int((st != st0).sum())} statuses differ"
    assert np.array_equal(nd, nd0), f"{name}: {int((nd != nd0).sum())} node counts differ"
    m = event_mask(hdr_t, st == codec.STATUS_LIN)
    assert np.array_equal(w[:len(m)][m], w0[:len(m)][m]), f"{name}: witnesses differ"


def test_helpers_on_a_hand_made_batch():
    """scale keeps a packed batch packed and drops exactly the histories with
    a value outside int32; relabel_* touch only the fields they name; the
    witness replay follows insertWith (Withdraw on an absent account: +m)."""
    hdr = np.zeros(3, dtype=codec.HDR_DTYPE)
    ev = np.zeros(12, dtype=codec.EV_DTYPE)
    for i in range(3):
        hdr[i] = (4 * i, 4, 2, models.MODEL_BANK, i, 0)
    # each history: Withdraw 1 m / WithdrawalMade, Transfer 1 -> 3 m / Balance m (pid 1)
    for i, m in enumerate((10, 30000, 7)):
        ev[4 * i + 0] = (0, 2, 1, 1, m)
        ev[4 * i + 1] = (0x80, 2, 0, 0, 0)
        ev[4 * i + 2] = (1, 4, 1, 3, m)
        ev[4 * i + 3] = (0x81, 7, 0, 0, m)
    m0 = models.BankModel(0b10, 0, (0, 5, 0, 0, 0, 0, 0, 0))
    h2, e2, m2, keep = scale(hdr, ev, 100000, m0)
    assert keep.tolist() == [True, False, True]
    assert h2["ev_off"].tolist() == [0, 4] and h2["tag"].tolist() == [0, 2] and len(e2) == 8
    assert e2["val"].tolist() == [10**6, 0, 10**6, 10**6, 7 * 10**5, 0, 7 * 10**5, 7 * 10**5]
    assert m2.balance[1] == 500000 and m2.exists == 0b10 and m0.balance[1] == 5
    assert ev["val"][0] == 10                                   # inputs untouched
    e3, m3 = relabel_accounts(ev, PI, m0)
    assert e3["a"].tolist()[:4] == [2, 0, 2, 0] and e3["b"].tolist()[:4] == [1, 0, 0, 0]
    assert m3.exists == 0b100 and m3.balance[2] == 5 and m3.balance[1] == 0
    h4, e4 = relabel_pids(hdr, ev, [100, 9])
    assert e4["kp"].tolist()[:4] == [100, 0x80 | 100, 9, 0x80 | 9] and (h4["n_pid"] == 101).all()
    w = np.full(12, 0xFF, dtype=np.uint8)
    w[0:2] = [0, 2]
    w[8:10] = [2, 0]
    assert max_balance_on_witness(hdr, ev, w, 3) == [30, 0, 21]
    with pytest.raises(ValueError):
        relabel_pids(hdr, ev, [3, 3])


@pytest.mark.parametrize("name", sorted(BANK_BATCHES))
@pytest.mark.parametrize("k", SCALES)
def test_oracle_scale(name, k):
    hdr, ev, st, nd, w = bank_batch(name)
    h2, e2, _, keep = scale(hdr, ev, k)
    if k < K_I32:
        assert keep.all()
    got = oracle_c.check_batch(models.MODEL_BANK, h2, e2, None, MAX_NODES, 8, witness=True)
    assert_same(f"S_{k}", got, (st[keep], nd[keep], w[event_mask(hdr, keep)]), h2)


@pytest.mark.parametrize("name", sorted(BANK_BATCHES))
@pytest.mark.parametrize("pi", [PI, PI_SWAP])
def test_oracle_accounts(name, pi):
    hdr, ev, st, nd, w = bank_batch(name)
    e2, _ = relabel_accounts(ev, pi)
    got = oracle_c.check_batch(models.MODEL_BANK, hdr, e2, None, MAX_NODES, 8, witness=True)
    assert_same("A_pi", got, (st, nd, w), hdr)


@pytest.mark.parametrize("name", sorted(BANK_BATCHES))
@pytest.mark.parametrize("sigma", [SIGMA_8, SIGMA_128, SIGMA_MIX])
def test_oracle_pids_bank(name, sigma):
    hdr, ev, st, nd, w = bank_batch(name)
    h2, e2 = relabel_pids(hdr, ev, sigma)
    got = oracle_c.check_batch(models.MODEL_BANK, h2, e2, None, MAX_NODES, 8, witness=True)
    assert_same("P_sigma", got, (st, nd, w), hdr)


@pytest.mark.parametrize("name", sorted(BANK_BATCHES))
def test_oracle_composition(name):
    """A_pi . P_sigma . S_2 with a model0 on the accounts the histories never
    open (6, 7 -> pi: 3, 4), against the same model0 unscaled, unrelabelled."""
    hdr, ev, _, _, _ = bank_batch(name)
    m0 = models.BankModel(0b11000000, 0, (0, 0, 0, 0, 0, 0, 300, 11))
    want = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, m0, MAX_NODES, 8, witness=True)
    h2, e2, m2, keep = scale(hdr, ev, 2, m0)
    assert keep.all() and m2.balance[6] == 600
    h2, e2 = relabel_pids(h2, e2, SIGMA_128)
    e2, m2 = relabel_accounts(e2, PI, m2)
    assert m2.exists == 0b11000 and m2.balance[3] == 600 and m2.balance[4] == 22
    got = oracle_c.check_batch(models.MODEL_BANK, h2, e2, m2, MAX_NODES, 8, witness=True)
    assert_same("A.P.S", got, want, hdr)


@pytest.mark.parametrize("name,sigmas", [("ticket_2x10", ([5], [100])),
                                         ("ticket_8x32", (SIGMA_8, SIGMA_128))])
def test_oracle_pids_ticket(name, sigmas):
    """ticket_2x10 runs every client on one shared pid (0 -> 5, 0 -> 100);
    the 8 x 32 batch has 8 pids and all three outcomes."""
    hdr, ev, st, nd, w, max_nodes = ticket_batch(name)
    if name == "ticket_8x32":
        assert (hdr["n_pid"] == 8).all() and (hdr["n_ev"] == 64).all()
        for s in (codec.STATUS_LIN, codec.STATUS_NONLIN, codec.STATUS_BUDGET):
            assert (st == s).sum() > 0, s
    else:
        assert (hdr["n_pid"] == 1).all()
    for sigma in sigmas:
        h2, e2 = relabel_pids(hdr, ev, sigma)
        got = oracle_c.check_batch(models.MODEL_TICKET, h2, e2, None, max_nodes, 8, witness=True)
        assert_same("P_sigma", got, (st, nd, w), hdr)


def _literal_history(h, ev):
    o, n = int(h["ev_off"]), int(h["n_ev"])
    ident = {q: q for q in range(8)}
    out = []
    for e in ev[o:o + n]:
        pid = int(e["kp"]) & 0x7F
        if int(e["kp"]) & 0x80:
            out.append((pid, ("R", models.BANK.decode_resp(int(e["code"]), int(e["val"])))))
        else:
            out.append((pid, ("L", models.BANK.decode_inv(int(e["code"]), int(e["a"]), int(e["b"]),
                                                          int(e["val"]), ident))))
    return out


@pytest.mark.parametrize("k", SCALES)
def test_literal_oracle_on_scaled_histories(k):
    """oracle/linearise_lists.py (Python integers: they never wrap) against
    the C oracle on 300 scaled histories per k, 150 each from bank_4x16 and
    bank_4x16_bugs: pins the C oracle's own i64 balances.  At k = 21474836 at
    least 50 of the 300 take a balance past INT32_MAX on their witness."""
    past = 0
    for name in ("bank_4x16", "bank_4x16_bugs"):
        hdr, ev, _, _, _ = bank_batch(name)
        h2, e2, _, keep = scale(hdr, ev, k)
        h2 = h2[:150]
        st, nd, _ = oracle_c.check_batch(models.MODEL_BANK, h2, e2, None, 20000, 4)
        for i, h in enumerate(h2):
            lit = LL.check("bank", _literal_history(h, e2), max_nodes=20000)
            assert (lit[0], lit[1]) == (codec.STATUS_NAMES[int(st[i])], int(nd[i])), (name, k, i)
        past += int((witness_peak(name)[keep][:150] * k > I32_MAX).sum())
    if k == K_I32:
        assert past >= 50, past


def test_teeth_i32():
    """At k = 21474836 at most 20 % of each batch is dropped, and at least
    1000 retained histories per batch are linearisable with a balance above
    INT32_MAX on the oracle's witness path: a 32-bit balance anywhere on the
    device's route flips those verdicts.  Measured (retained / linearisable /
    above INT32_MAX): bank_4x16 17996 / 17996 / 8876, bank_4x16_bugs 17980 /
    10105 / 4963, bank_6x24 2532 / 2532 / 1589."""
    for name, n in BANK_BATCHES.items():
        hdr, ev, st, _, _ = bank_batch(name)
        _, _, _, keep = scale(hdr, ev, K_I32)
        above = (witness_peak(name)[keep] * K_I32 > I32_MAX)
        print(name, int(keep.sum()), int((st[keep] == codec.STATUS_LIN).sum()), int(above.sum()))
        assert (~keep).sum() <= n // 5, name
        assert above.sum() >= 1000, name


def test_teeth_i16():
    """The i16 memo keys of wave mode: at k = 128 at least 100 linearisable
    histories of bank_4x16_bugs take a balance above 32767 on the oracle's
    witness path, at k = 64 none does (and 100 k stays below 2^24, inside
    wave mode's wide launches).  Measured: the largest balance on a witness
    path of bank_4x16_bugs is 427 unscaled; histories above 32767 at k = 64 /
    82 / 100 / 120 / 128: 0 / 3 / 14 / 65 / 121 (bank_4x16: 0 / 0 / 10 / 90 /
    181, bank_6x24: 0 / 1 / 2 / 24 / 47).  82 gives too few, so k = 128."""
    peak = witness_peak("bank_4x16_bugs")
    over = int((peak * K_I16 > 32767).sum())
    print("peak", int(peak.max()), "above 32767 at k", K_I16, over, "at 64", int((peak * 64 > 32767).sum()))
    assert 100 * K_I16 < 1 << 24
    assert over >= 100
    assert int((peak * 64 > 32767).sum()) == 0
