"""Models and settings shared by the table-generator tests
(test_table_gen_host.py, test_gpu_table_gen.py).

TEST INFRASTRUCTURE ONLY.
"""

from __future__ import annotations

import functools

import numpy as np

import tablegen as tg
import wtablegen as wg
from linearise_lists import ModelError
from qsmd import gen
from qsmd.models import TableModel, WideTableModel

AT_INVOKE, IN_WINDOW = gen.LIN_AT_INVOKE, gen.LIN_IN_WINDOW
PER_CLIENT, SHARED = gen.PID_PER_CLIENT, gen.PID_SHARED

CLOSURES = {"register": tg.REGISTER, "lock": tg.LOCK, "ticket16": tg.ticket_closures(16), "kv": wg.KV,
            "big": wg.BIG}


def _random_tables(rng, ns, ni, nr, wide):
    """Seeded random tables with post_err.  post keeps one bit in eight and
    post_err removes a quarter of those, so many (state, invocation) pairs
    accept nothing: requests fall back, executions get stuck."""
    pw = (nr + 31) // 32
    shape = (ns, ni, pw) if wide else (ns, ni)
    bits = lambda: rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    post = bits() & bits() & bits()
    err = bits() & bits()
    # (bits at or above n_resp stay set: the generator must ignore them)
    on_inv = rng.integers(0, ns, size=(ns, ni))
    on_resp = rng.integers(0, ns, size=(ns, nr))
    cls = WideTableModel if wide else TableModel
    return cls(list(range(ns)), list(range(ni)), list(range(nr)), on_inv, on_resp, post, err,
               init_state=int(rng.integers(0, ns)))


@functools.lru_cache(maxsize=None)
def model(name):
    if name in ("kv", "big"):
        return wg.wide_table(name)
    if name == "rand_narrow":          # the maximal narrow table: an 80 KB blob
        return _random_tables(np.random.default_rng(0x7AB1E), 256, 32, 32, False)
    if name == "rand_wide":            # post_words 3: responses in the second and third word
        return _random_tables(np.random.default_rng(0x71DE), 300, 40, 70, True)
    if name == "one_resp":             # a single response symbol: the bug can only swap
        return TableModel([0, 1], ["a", "b"], ["ok"], [[1, 0], [0, 1]], [[0], [1]], [[1, 1], [1, 0]])
    c = CLOSURES[name]
    return TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                    raises=ModelError)


def _kv_weights():
    w = np.random.default_rng(5).integers(0, 4, size=len(wg.KV_INVS)).astype(np.uint32)
    w[:3] = 0
    return tuple(int(x) for x in w)


# (id, model, parameters, first, ev_base, weights)
CASES = [
    ("reg_4x16_bugs", "register", dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=IN_WINDOW,
                                       pid_mode=PER_CLIENT, p_bug=0.5, seed=0x5EED), 0, 0, None),
    ("reg_1x1", "register", dict(n_clients=1, n_ops=1, prefix_ops=0, lin_policy=AT_INVOKE, pid_mode=PER_CLIENT,
                                 p_bug=1.0, seed=1), 123457, 0, None),
    ("reg_32x64_shared", "register", dict(n_clients=32, n_ops=64, prefix_ops=0, lin_policy=IN_WINDOW,
                                          pid_mode=SHARED, overlap=3, p_bug=0.3, seed=2), (1 << 33) + 5, 1000,
     None),
    ("reg_all_prefix", "register", dict(n_clients=4, n_ops=16, prefix_ops=16, lin_policy=IN_WINDOW,
                                        pid_mode=PER_CLIENT, p_bug=1.0, seed=3), 0, 0, None),
    ("reg_prefix_past_k", "register", dict(n_clients=3, n_ops=5, prefix_ops=40, lin_policy=AT_INVOKE,
                                           pid_mode=SHARED, p_bug=0.5, seed=4), 0, 1000, None),
    ("lock_3x10_w", "lock", dict(n_clients=3, n_ops=10, prefix_ops=2, lin_policy=AT_INVOKE, pid_mode=PER_CLIENT,
                                 overlap=1, p_bug=0.2, seed=5), 123457, 0, (6, 1, 6)),
    ("lock_zero_weight", "lock", dict(n_clients=4, n_ops=16, prefix_ops=0, lin_policy=IN_WINDOW,
                                      pid_mode=PER_CLIENT, seed=6), 0, 0, (6, 0, 6)),
    # only Unlock has a weight, and the unlocked state accepts no response for it: W = 0, then stuck
    ("lock_fallback", "lock", dict(n_clients=2, n_ops=8, prefix_ops=1, lin_policy=IN_WINDOW, pid_mode=PER_CLIENT,
                                   p_bug=0.5, seed=7), 0, 0, (0, 1, 0)),
    ("ticket_2x10_shared", "ticket16", dict(n_clients=2, n_ops=10, prefix_ops=4, lin_policy=AT_INVOKE,
                                            pid_mode=SHARED, p_bug=0.5, seed=15), 0, 0, None),
    ("ticket_8x16", "ticket16", dict(n_clients=8, n_ops=16, prefix_ops=1, lin_policy=IN_WINDOW,
                                     pid_mode=PER_CLIENT, overlap=3, seed=8), (1 << 33) + 5, 0, (8, 1)),
    ("kv_4x16_bugs", "kv", dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=IN_WINDOW, pid_mode=PER_CLIENT,
                                p_bug=0.5, seed=9), 0, 0, None),
    ("kv_3x10_w", "kv", dict(n_clients=3, n_ops=10, prefix_ops=0, lin_policy=AT_INVOKE, pid_mode=SHARED,
                             overlap=3, p_bug=0.1, seed=10), 123457, 1000, _kv_weights()),
    ("big_4x16", "big", dict(n_clients=4, n_ops=16, prefix_ops=2, lin_policy=IN_WINDOW, pid_mode=PER_CLIENT,
                             p_bug=0.5, seed=11), (1 << 33) + 5, 0, None),
    ("rand_narrow_5x64", "rand_narrow", dict(n_clients=5, n_ops=64, prefix_ops=3, lin_policy=IN_WINDOW,
                                             pid_mode=PER_CLIENT, p_bug=0.5, seed=12), 0, 0, None),
    ("rand_narrow_3x7", "rand_narrow", dict(n_clients=3, n_ops=7, prefix_ops=0, lin_policy=AT_INVOKE,
                                            pid_mode=SHARED, overlap=1, p_bug=0.5, seed=13), 123457, 0, None),
    ("rand_wide_4x16", "rand_wide", dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=IN_WINDOW,
                                         pid_mode=PER_CLIENT, p_bug=0.5, seed=14), 0, 0, None),
    ("rand_wide_32x64", "rand_wide", dict(n_clients=32, n_ops=64, prefix_ops=0, lin_policy=AT_INVOKE,
                                          pid_mode=PER_CLIENT, overlap=1, p_bug=0.5, seed=16), 0, 1000, None),
    ("one_resp_swap", "one_resp", dict(n_clients=2, n_ops=4, prefix_ops=1, lin_policy=IN_WINDOW,
                                       pid_mode=PER_CLIENT, p_bug=1.0, seed=17), 0, 0, None),
    ("one_resp_single", "one_resp", dict(n_clients=2, n_ops=3, prefix_ops=2, lin_policy=IN_WINDOW,
                                         pid_mode=PER_CLIENT, p_bug=1.0, seed=18), 0, 0, None),
]
CASE_IDS = [c[0] for c in CASES]


def host(case, n, first=None, threads=8):
    """qsmd.gen.generate_table on a case: (hdr, events, flags)."""
    _, name, kw, first0, ev_base, w = case
    p = gen.table_params(inv_weight=w, **kw)
    return gen.generate_table(p, model(name), first0 if first is None else first, n, threads, ev_base)


def history(m, hdr, events, i):
    """History i as the oracle takes it: [(pid, ("L", inv) | ("R", resp))]."""
    o, n = int(hdr[i]["ev_off"]) - int(hdr[0]["ev_off"]), int(hdr[i]["n_ev"])
    out = []
    for e in events[o:o + n]:
        kp, code = int(e["kp"]), int(e["code"])
        out.append((kp & 0x7F, ("R", m.resps[code]) if kp & 0x80 else ("L", m.invs[code])))
    return out
