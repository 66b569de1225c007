"""The keyed pending call's local mode (knob "kpending_local", include/qsmd.h),
restated literally: when a history with pending invocations is splittable, its
split by key, the pending rule (tests/pending_ref.py) with the component's
closures on every part, and the rule that combines the parts' results.

TEST INFRASTRUCTURE ONLY.  Written from the definition, not from
qsmd.models.KeyedTableModel.split_history, which the tests compare with it.

A history here is the tests' list of ``(pid, ("L", (key, inv)))`` /
``(pid, ("R", resp))``; ``component`` is a tablegen model dict.

Splittable: at most 128 events, every symbol one of the model's and every
invocation's key below ``n_keys``, and per pid the events alternate invocation,
response, ... from an invocation; they may end on an invocation, which is
pending and belongs to its own key.  :func:`refusal` names the first reason a
history is not splittable.
"""

from __future__ import annotations

from pending_ref import linearisable_pending

MAX_EVENTS = 128
REASONS = ("too_long", "symbol", "key", "lone_response", "two_in_flight")


def refusal_shape(shape, n_keys):
    """``shape``: per event ``(pid, is_response, key or None, symbol_ok)``.
    None when splittable, else one of REASONS."""
    if len(shape) > MAX_EVENTS:
        return "too_long"
    for pid, is_resp, key, ok in shape:
        if not ok:
            return "symbol"
        if not is_resp and not (isinstance(key, int) and not isinstance(key, bool) and 0 <= key < n_keys):
            return "key"
    for pid in sorted({s[0] for s in shape}):
        mine = [s[1] for s in shape if s[0] == pid]
        for q, is_resp in enumerate(mine):
            if is_resp != bool(q % 2):          # invocation, response, invocation, ...
                return "lone_response" if is_resp else "two_in_flight"
    return None


def splittable_shape(shape, n_keys):
    """None when the history is not splittable, else for every event the key
    of its operation."""
    if refusal_shape(shape, n_keys) is not None:
        return None
    keys = [None] * len(shape)
    for pid in {s[0] for s in shape}:
        mine = [n for n, s in enumerate(shape) if s[0] == pid]
        for q, n in enumerate(mine):
            keys[n] = shape[n][2] if q % 2 == 0 else keys[mine[q - 1]]
    return keys


def _hashable(x):
    try:
        hash(x)
        return True
    except TypeError:
        return False


def shape_of(component, history):
    invs, resps = component["invs"], component["resps"]
    shape = []
    for pid, (kind, x) in history:
        if kind == "L":
            pair = isinstance(x, tuple) and len(x) == 2
            shape.append((pid, False, x[0] if pair else None, pair and _hashable(x[1]) and x[1] in invs))
        else:
            shape.append((pid, True, None, _hashable(x) and x in resps))
    return shape


def refusal(component, n_keys, history):
    return refusal_shape(shape_of(component, history), n_keys)


def split(component, n_keys, history):
    """None, or [(key, sub_history)] in ascending key order (the keyed
    events, unchanged)."""
    keys = splittable_shape(shape_of(component, history), n_keys)
    if keys is None:
        return None
    return [(k, [e for e, ke in zip(history, keys) if ke == k]) for k in sorted(set(keys))]


def unkeyed(sub_history):
    """A part in the component's own symbols."""
    return [(pid, (kind, x[1] if kind == "L" else x)) for pid, (kind, x) in sub_history]


def combine(results):
    """[(status, nodes)] of the parts, ascending keys -> the history's: the
    status of the lowest key whose part is not linearisable, the nodes summed."""
    status = "lin"
    for st, _ in results:
        if st != "lin":
            status = st
            break
    return status, sum(n for _, n in results)


def _search(component, sub, max_nodes, init):
    st, nd, _ = linearisable_pending(component, sub, max_nodes, init)
    return st, nd


def check(component, n_keys, history, max_nodes=0, model0=None):
    """None when the history is not splittable (the product route), else
    ``(status, nodes)`` of the local mode."""
    parts = split(component, n_keys, history)
    if parts is None:
        return None
    init = (component["init"],) * n_keys if model0 is None else model0
    return combine([_search(component, unkeyed(sub), max_nodes, init[k]) for k, sub in parts])


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
            results.append(_search(component, sub, max_nodes, init[k]))
        out.append(combine(results))
    return out
