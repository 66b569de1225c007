"""The keyed model's local mode (knob "ktable_local", include/qsmd.h), restated
literally: the split of a history by key, the literal oracle
(oracle/linearise_lists.py) with the component's closures on every part, and
the rule that combines the parts' results.

TEST INFRASTRUCTURE ONLY.  Written from the definition, not from
qsmd.models.KeyedTableModel.split_history, which the tests compare with it.

A history here is the tests' list of ``(pid, ("L", (key, inv)))`` /
``(pid, ("R", resp))``; ``component`` is a tablegen model dict.
"""

from __future__ import annotations

from linearise_lists import linearisable as oracle_linearisable

MAX_EVENTS = 128
FAILING_FIRST = ("lin",)        # a part with another status decides the history


def splittable_shape(shape, n_keys):
    """``shape``: per event ``(pid, is_response, key or None, symbol_ok)``.
    None when the history is not splittable, else for every event the key of
    its operation.  Condition 2 is tested per pid on the pid's own events."""
    if len(shape) > MAX_EVENTS:
        return None
    for pid, is_resp, key, ok in shape:
        if not ok or (not is_resp and not (isinstance(key, int) and 0 <= key < n_keys)):
            return None
    keys = [None] * len(shape)
    for pid in {s[0] for s in shape}:
        mine = [n for n, s in enumerate(shape) if s[0] == pid]
        if len(mine) % 2:
            return None
        for q, n in enumerate(mine):
            if shape[n][1] != bool(q % 2):      # invocation, response, invocation, ...
                return None
        for inv, resp in zip(mine[0::2], mine[1::2]):
            keys[inv] = keys[resp] = shape[inv][2]
    return keys


def _hashable(x):
    try:
        hash(x)
        return True
    except TypeError:
        return False


def split(component, n_keys, history):
    """None, or [(key, sub_history)] in ascending key order (the keyed
    events, unchanged)."""
    invs, resps = component["invs"], component["resps"]
    shape = []
    for pid, (kind, x) in history:
        if kind == "L":
            pair = isinstance(x, tuple) and len(x) == 2
            shape.append((pid, False, x[0] if pair and not isinstance(x[0], bool) else None,
                          pair and _hashable(x[1]) and x[1] in invs))
        else:
            shape.append((pid, True, None, _hashable(x) and x in resps))
    keys = splittable_shape(shape, n_keys)
    if keys is None:
        return None
    return [(k, [e for e, ke in zip(history, keys) if ke == k]) for k in sorted(set(keys))]


def unkeyed(sub_history):
    """A part in the component's own symbols."""
    return [(pid, (kind, x[1] if kind == "L" else x)) for pid, (kind, x) in sub_history]


def combine(results):
    """[(status, nodes)] of the parts, ascending keys -> the history's."""
    status = "lin"
    for st, _ in results:
        if st not in FAILING_FIRST:
            status = st
            break
    return status, sum(n for _, n in results)


def check(component, n_keys, history, max_nodes=0, model0=None):
    """None when the history is not splittable (the product route), else
    ``(status, nodes)`` of the local mode."""
    parts = split(component, n_keys, history)
    if parts is None:
        return None
    init = (component["init"],) * n_keys if model0 is None else model0
    results = []
    for k, sub in parts:
        st, nd, _ = oracle_linearisable(component["transition"], component["postcondition"], init[k],
                                        unkeyed(sub), max_nodes)
        results.append((st, nd))
    return combine(results)


def split_arrays(hdr, events, n_events, n_keys, n_inv, n_resp):
    """The same definition on one encoded history (a codec.HDR_DTYPE record
    and the events array): None, or [(key, [event indices, history-local])]."""
    off, n = int(hdr["ev_off"]), int(hdr["n_ev"])
    if int(hdr["model_id"]) != 5 or n > MAX_EVENTS or off + n > n_events:
        return None
    shape = []
    for e in events[off:off + n]:
        is_resp = bool(e["kp"] & 0x80)
        shape.append((int(e["kp"]) & 0x7F, is_resp, None if is_resp else int(e["a"]),
                      int(e["code"]) < (n_resp if is_resp else n_inv)))
    keys = splittable_shape(shape, n_keys)
    if keys is None:
        return None
    return [(k, [j for j, ke in enumerate(keys) if ke == k]) for k in sorted(set(keys))]


def check_arrays(component, n_keys, hdr, events, max_nodes=0, model0=None, n_events=None):
    """Per header: None (the product route) or ``(status, nodes)``, the parts
    decoded with the component's symbol lists in table order."""
    invs, resps = component["invs"], component["resps"]
    n_events = len(events) if n_events is None else n_events
    init = (component["init"],) * n_keys if model0 is None else model0
    out = []
    for h in hdr:
        parts = split_arrays(h, events, n_events, n_keys, len(invs), len(resps))
        if parts is None:
            out.append(None)
            continue
        off = int(h["ev_off"])
        results = []
        for k, idx in parts:
            sub = []
            for j in idx:
                e = events[off + j]
                sub.append((int(e["kp"]) & 0x7F, ("R", resps[int(e["code"])]) if e["kp"] & 0x80
                            else ("L", invs[int(e["code"])])))
            st, nd, _ = oracle_linearisable(component["transition"], component["postcondition"], init[k], sub,
                                            max_nodes)
            results.append((st, nd))
        out.append(combine(results))
    return out
