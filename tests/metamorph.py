"""Metamorphic transformations of encoded batches (numpy only).

The reference's Bank model (test/Bank.hs:92-131) only adds, subtracts and
compares money, compares accounts for equality, and the search
(src/Linearisability.hs:25-69) only compares pids for equality and orders
candidates by position.  So three transformations of a history leave its
search tree isomorphic -- the verdict, the node count and the witness (event
indices) are unchanged:

  S_k   scale: every invocation's val, every Balance response's val and every
        model0 balance times k > 0
  A_pi  account relabelling: a permutation of 0..7 applied to `a`, to `b` of
        Transfers, and to model0's exists bits and balances
  P_s   pid relabelling: an injective map into 0..127 applied to the pid bits
        of `kp`, n_pid raised to max s + 1 (TicketDispenser too)

Arrays are in the include/qsmd.h layout (qsmd.codec HDR_DTYPE / EV_DTYPE);
model0 is None or a qsmd.models.BankModel.  Nothing is modified in place.
"""

import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
EV_RESP = 0x80
BANK_OPEN, BANK_DEPOSIT, BANK_WITHDRAW, BANK_CHECK, BANK_TRANSFER = 0, 1, 2, 3, 4
BANK_BALANCE = 7
N_ACCOUNTS = 8


def _copy_model0(model0):
    m = type(model0)()
    m.exists = model0.exists
    for q in range(N_ACCOUNTS):
        m.balance[q] = model0.balance[q]
    return m


def _money(ev):
    """The events whose val is money: invocations and Balance responses."""
    resp = (ev["kp"] & EV_RESP) != 0
    return ~resp | (ev["code"] == BANK_BALANCE)


def scale(hdr, ev, k, model0=None):
    """S_k on a Bank batch.  Returns (hdr', ev', model0', keep): keep[i] says
    that every scaled value of history i fits int32 (the products are taken in
    int64); the other histories are dropped, and the kept ones are laid out
    back to back in header order with their headers rebased, so a packed
    uniform batch stays one (the coalesced staging path is still taken)."""
    if k <= 0:
        raise ValueError("S_k needs k > 0")
    n_ev = hdr["n_ev"].astype(np.int64)
    off = hdr["ev_off"].astype(np.int64)
    idx = np.repeat(off - (np.cumsum(n_ev) - n_ev), n_ev) + np.arange(int(n_ev.sum()), dtype=np.int64)
    owner = np.repeat(np.arange(len(hdr)), n_ev)
    e = ev[idx]                                          # the batch's events, history by history
    v = e["val"].astype(np.int64)
    v = np.where(_money(e), v * int(k), v)
    fits = (v >= I32_MIN) & (v <= I32_MAX)
    keep = np.ones(len(hdr), dtype=bool)
    keep[owner[~fits]] = False
    sel = keep[owner]
    e2 = e[sel].copy()
    e2["val"] = v[sel].astype(np.int32)
    h2 = hdr[keep].copy()
    kept = n_ev[keep]
    h2["ev_off"] = (np.cumsum(kept) - kept).astype(np.uint32)
    m2 = None
    if model0 is not None:
        m2 = _copy_model0(model0)
        for q in range(N_ACCOUNTS):
            b = int(model0.balance[q]) * int(k)
            if not (I64_MIN <= b <= I64_MAX):
                raise ValueError("scaled model0 balance outside int64")
            m2.balance[q] = b
    return h2, e2, m2, keep


def relabel_accounts(ev, pi, model0=None):
    """A_pi on a Bank batch.  Returns (ev', model0')."""
    pi = np.asarray(pi, dtype=np.uint8)
    if sorted(pi.tolist()) != list(range(N_ACCOUNTS)):
        raise ValueError("A_pi needs a permutation of 0..7")
    inv = (ev["kp"] & EV_RESP) == 0
    e2 = ev.copy()
    e2["a"] = np.where(inv, pi[ev["a"] & 7], ev["a"])
    xfer = inv & (ev["code"] == BANK_TRANSFER)
    e2["b"] = np.where(xfer, pi[ev["b"] & 7], ev["b"])
    m2 = None
    if model0 is not None:
        m2 = type(model0)()
        m2.exists = 0
        for q in range(N_ACCOUNTS):
            if (model0.exists >> q) & 1:
                m2.exists |= 1 << int(pi[q])
            m2.balance[int(pi[q])] = model0.balance[q]
    return e2, m2


def relabel_pids(hdr, ev, sigma):
    """P_sigma.  sigma[p] is the new pid of pid p; it must be injective, into
    0..127, and cover every pid the headers admit.  Returns (hdr', ev')."""
    sigma = [int(x) for x in sigma]
    if len(set(sigma)) != len(sigma) or min(sigma) < 0 or max(sigma) > 127:
        raise ValueError("P_sigma needs an injective map into 0..127")
    if int(hdr["n_pid"].max(initial=0)) > len(sigma) or int((ev["kp"] & 0x7F).max(initial=0)) >= len(sigma):
        raise ValueError("sigma does not cover the batch's pids")
    s = np.asarray(sigma, dtype=np.uint8)
    e2 = ev.copy()
    e2["kp"] = (ev["kp"] & EV_RESP) | s[ev["kp"] & 0x7F]
    h2 = hdr.copy()
    h2["n_pid"] = max(sigma) + 1
    return h2, e2


def max_balance_on_witness(hdr, ev, witness, k=1):
    """Replay each history's witness (the linearisation the search found: per
    history, the event indices of the invocations in order, 0xFF-terminated)
    on the Bank model with Python integers, every money value times k, and
    return the largest balance any account reaches, one int per history (0
    for an empty witness).  Only meaningful for linearisable histories.
    next' of test/Bank.hs:92-101: Open -> 0 when absent; Deposit and Withdraw
    with insertWith semantics (absent -> +m); Transfer = Withdraw a, Deposit b."""
    k = int(k)
    out = []
    code, acc, bcc, val = ev["code"], ev["a"], ev["b"], ev["val"]
    for h in hdr:
        o, n = int(h["ev_off"]), int(h["n_ev"])
        bal = {}
        top = 0
        for j in witness[o:o + n]:
            if j == 0xFF:
                break
            e = o + int(j)
            c, a, m = int(code[e]), int(acc[e]), int(val[e]) * k
            if c == BANK_OPEN:
                bal.setdefault(a, 0)
            elif c == BANK_DEPOSIT:
                bal[a] = bal[a] + m if a in bal else m
            elif c in (BANK_WITHDRAW, BANK_TRANSFER):
                bal[a] = bal[a] - m if a in bal else m
                if c == BANK_TRANSFER:
                    b = int(bcc[e])
                    bal[b] = bal[b] + m if b in bal else m
            if bal:
                top = max(top, max(bal.values()))
        out.append(top)
    return out
