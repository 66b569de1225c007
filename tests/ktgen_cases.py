"""Models and settings shared by the keyed-table generator tests
(test_ktable_gen_host.py, test_gpu_ktable_gen.py).

TEST INFRASTRUCTURE ONLY.
"""

from __future__ import annotations

import functools

import numpy as np

import ktablegen as kg
import tgen_cases as tc
from qsmd import gen
from qsmd.models import KeyedTableModel, TableModel

AT_INVOKE, IN_WINDOW = tc.AT_INVOKE, tc.IN_WINDOW
PER_CLIENT, SHARED = tc.PER_CLIENT, tc.SHARED

LATER = (1 << 33) + 5


@functools.lru_cache(maxsize=None)
def model(name, n_keys):
    """The keyed model over a component: tgen_cases.model's register, lock,
    one_resp and rand_narrow (256 x 32 x 32 with post_err, an 80 KB blob), or
    full32 below."""
    return KeyedTableModel(component(name), n_keys)


@functools.lru_cache(maxsize=None)
def component(name):
    if name == "full32":
        # every state accepts a response for each of 32 invocations: on 8 keys a
        # request draws below(256), the most the 8 x 32 pairs can weigh
        rng = np.random.default_rng(0xF32)
        return TableModel(list(range(3)), list(range(32)), ["a", "b"], rng.integers(0, 3, size=(3, 32)),
                          rng.integers(0, 3, size=(3, 2)), rng.integers(1, 4, size=(3, 32)).astype(np.uint32))
    return tc.model(name)


@functools.lru_cache(maxsize=None)
def product(name, n_keys):
    """The product closures of a tablegen model (register, lock)."""
    return kg.product(tc.CLOSURES[name], n_keys)


# (id, component, keys, parameters, first, ev_base, inv weights, key weights)
CASES = [
    ("reg1_1x1", "register", 1, dict(n_clients=1, n_ops=1, prefix_ops=0, lin_policy=AT_INVOKE, pid_mode=PER_CLIENT,
                                     p_bug=1.0, seed=1), 123457, 0, None, None),
    # one key: the kernel's request() takes the component's own one-word pick
    ("reg1_4x16_bugs", "register", 1, dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=IN_WINDOW,
                                           pid_mode=PER_CLIENT, p_bug=0.5, seed=0x5EED), 0, 0, None, None),
    ("lock1_zero_inv", "lock", 1, dict(n_clients=4, n_ops=16, prefix_ops=2, lin_policy=IN_WINDOW,
                                       pid_mode=PER_CLIENT, p_bug=0.5, seed=19), LATER, 0, (1, 0, 1), (1,)),
    ("lock1_fallback", "lock", 1, dict(n_clients=2, n_ops=8, prefix_ops=1, lin_policy=IN_WINDOW,
                                       pid_mode=PER_CLIENT, p_bug=0.5, seed=20), 0, 0, (0, 1, 0), None),
    ("rand1_5x64", "rand_narrow", 1, dict(n_clients=5, n_ops=64, prefix_ops=3, lin_policy=IN_WINDOW,
                                          pid_mode=PER_CLIENT, p_bug=0.5, seed=21), 0, 0, None, None),
    ("reg4_4x16_bugs", "register", 4, dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=IN_WINDOW,
                                           pid_mode=PER_CLIENT, p_bug=0.5, seed=0x5EED), 0, 0, None, None),
    ("reg8_32x64_shared", "register", 8, dict(n_clients=32, n_ops=64, prefix_ops=0, lin_policy=IN_WINDOW,
                                              pid_mode=SHARED, overlap=3, p_bug=0.3, seed=2), 0, 0, None, None),
    ("reg4_later_shard", "register", 4, dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=AT_INVOKE,
                                             pid_mode=PER_CLIENT, p_bug=0.5, seed=3), LATER, 1000, None, None),
    ("lock8_w", "lock", 8, dict(n_clients=3, n_ops=10, prefix_ops=2, lin_policy=AT_INVOKE, pid_mode=PER_CLIENT,
                                overlap=1, p_bug=0.2, seed=5), 123457, 0, (6, 1, 6), None),
    ("lock8_zero_inv", "lock", 8, dict(n_clients=4, n_ops=16, prefix_ops=0, lin_policy=IN_WINDOW,
                                       pid_mode=PER_CLIENT, seed=6), 0, 0, (1, 0, 1), None),
    ("lock8_zero_inv_w", "lock", 8, dict(n_clients=4, n_ops=16, prefix_ops=0, lin_policy=IN_WINDOW,
                                         pid_mode=PER_CLIENT, seed=6), 0, 0, (6, 0, 6), (1, 2, 3, 4, 5, 6, 7, 8)),
    ("reg8_hot_key", "register", 8, dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=IN_WINDOW,
                                         pid_mode=PER_CLIENT, p_bug=0.5, seed=7), 0, 0, None,
     (8, 1, 1, 1, 1, 1, 1, 0)),
    ("reg4_zero_key", "register", 4, dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=IN_WINDOW,
                                          pid_mode=PER_CLIENT, p_bug=0.5, seed=8), LATER, 0, None, (1, 0, 1, 1)),
    # only Unlock has a weight, and an unlocked lock accepts no response for it: W = 0, then stuck
    ("lock2_fallback", "lock", 2, dict(n_clients=2, n_ops=8, prefix_ops=1, lin_policy=IN_WINDOW,
                                       pid_mode=PER_CLIENT, p_bug=0.5, seed=9), 0, 0, (0, 1, 0), None),
    ("lock3_fallback_w", "lock", 3, dict(n_clients=2, n_ops=8, prefix_ops=1, lin_policy=AT_INVOKE,
                                         pid_mode=PER_CLIENT, p_bug=0.5, seed=10), 0, 0, (0, 3, 0), (2, 0, 1)),
    ("one_resp2_swap", "one_resp", 2, dict(n_clients=2, n_ops=4, prefix_ops=1, lin_policy=IN_WINDOW,
                                           pid_mode=PER_CLIENT, p_bug=1.0, seed=17), 0, 0, None, None),
    ("one_resp2_single", "one_resp", 2, dict(n_clients=2, n_ops=3, prefix_ops=2, lin_policy=IN_WINDOW,
                                             pid_mode=PER_CLIENT, p_bug=1.0, seed=18), 0, 0, None, None),
    ("rand8_5x64", "rand_narrow", 8, dict(n_clients=5, n_ops=64, prefix_ops=3, lin_policy=IN_WINDOW,
                                          pid_mode=PER_CLIENT, p_bug=0.5, seed=12), 0, 0, None, None),
    ("rand8_3x7", "rand_narrow", 8, dict(n_clients=3, n_ops=7, prefix_ops=0, lin_policy=AT_INVOKE,
                                         pid_mode=SHARED, overlap=1, p_bug=0.5, seed=13), 123457, 0, None, None),
    ("rand8_3x7_w", "rand_narrow", 8, dict(n_clients=3, n_ops=7, prefix_ops=1, lin_policy=IN_WINDOW,
                                           pid_mode=PER_CLIENT, p_bug=0.5, seed=14), 0, 1000,
     tuple((i * 7) % 5 for i in range(32)), (3, 0, 1, 2, 5, 1, 1, 4)),
    ("full32_8_4x16", "full32", 8, dict(n_clients=4, n_ops=16, prefix_ops=2, lin_policy=IN_WINDOW,
                                        pid_mode=PER_CLIENT, p_bug=0.5, seed=22), 0, 0, None, None),
    ("reg4_all_prefix", "register", 4, dict(n_clients=4, n_ops=16, prefix_ops=16, lin_policy=IN_WINDOW,
                                            pid_mode=PER_CLIENT, p_bug=1.0, seed=15), 0, 0, None, None),
    ("reg4_prefix_past_k", "register", 4, dict(n_clients=3, n_ops=5, prefix_ops=40, lin_policy=AT_INVOKE,
                                               pid_mode=SHARED, p_bug=0.5, seed=16), 0, 1000, None, None),
]
CASE_IDS = [c[0] for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def params(c):
    return gen.ktable_params(inv_weight=c[6], key_weight=c[7], **c[3])


def host(c, n, first=None, threads=8):
    """qsmd.gen.generate_ktable on a case: (hdr, events, flags)."""
    return gen.generate_ktable(params(c), model(c[1], c[2]), c[4] if first is None else first, n, threads, c[5])


def history(m, hdr, events, i):
    """History i as the oracle takes it on the product closures:
    [(pid, ("L", (key, inv)) | ("R", resp))]."""
    o, n = int(hdr[i]["ev_off"]) - int(hdr[0]["ev_off"]), int(hdr[i]["n_ev"])
    out = []
    for e in events[o:o + n]:
        kp, code = int(e["kp"]), int(e["code"])
        out.append((kp & 0x7F, ("R", m.resps[code]) if kp & 0x80 else ("L", (int(e["a"]), m.component.invs[code]))))
    return out
