"""Host-side mirror of the reference module ``Linearisability``
(src/Linearisability.hs:1-7 exports ``History``, ``linearisable``, ``trace``,
``wellformed``), with the search itself on the GPU.

* :func:`linearisable` keeps the reference signature
  ``linearisable transition postcondition model0 history -> Bool``
  (src/Linearisability.hs:52-58).  ``transition``/``postcondition`` must be
  the closures of a :class:`~qsmd.models.DeviceModel`: the reference's
  Bank / TicketDispenser models, or a :class:`~qsmd.models.TableModel` (any
  finite-state model, tabulated from its closures by
  ``TableModel.from_closures``; beyond 256 states or 32 symbols a
  :class:`~qsmd.models.WideTableModel`); any other closure raises -- there is no CPU
  search to fall back to.  Model exceptions propagate as in Haskell
  (:class:`~qsmd.models.ModelError` for ``Map.!``, test/Bank.hs:128).
* :func:`linearisable_batch` is the throughput entry point.
* :func:`explain_batch` / :func:`explain` (table models) say where a history
  went wrong: the deepest linearised path of its search, the model there and
  the operations that could not follow (:class:`Explanation`).
* :func:`trace` (src/Linearisability.hs:73-93) and :func:`wellformed`
  (src/Linearisability.hs:97-135) are host utilities; :func:`replay_witness`
  re-checks a GPU witness against the host model.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import codec, device
from .models import (BY_ID, BY_NAME, DeviceModel, EncodeError, KeyedTableModel, ModelError, TableModel,
                     WideTableModel)

__all__ = ["linearisable", "linearisable_batch", "trace", "wellformed", "replay_witness",
           "CheckResult", "NotSequential", "BudgetExceeded", "wellformed_batch",
           "explain", "explain_batch", "explanation_from_path", "Explanation", "ExplainResult"]


class BudgetExceeded(RuntimeError):
    """max_nodes was reached before the search decided (not a reference outcome)."""


def _device_model(transition, postcondition) -> DeviceModel:
    for m in BY_ID.values():
        if transition is m.transition and postcondition is m.postcondition:
            return m
    # a TableModel's closures are bound methods (a new object at every
    # attribute access, so `is` never matches): found through their __self__
    # (a WideTableModel is a TableModel: the owner's model_id tells them apart)
    owner = getattr(transition, "__self__", None)
    if (isinstance(owner, TableModel) and getattr(postcondition, "__self__", None) is owner
            and getattr(transition, "__func__", None) is TableModel.transition
            and getattr(postcondition, "__func__", None) is TableModel.postcondition):
        return owner
    if (isinstance(owner, KeyedTableModel) and getattr(postcondition, "__self__", None) is owner
            and getattr(transition, "__func__", None) is KeyedTableModel.transition
            and getattr(postcondition, "__func__", None) is KeyedTableModel.postcondition):
        return owner
    raise NotImplementedError(
        "no device model for these closures: pass the closures of the reference's Bank "
        "(test/Bank.hs) or TicketDispenser (test/TicketDispenser.hs) models, or tabulate a "
        "finite-state model with qsmd.models.TableModel.from_closures (WideTableModel beyond "
        "256 states or 32 symbols; KeyedTableModel for a map of small states) and pass its "
        ".transition / .postcondition")


def _as_model(model) -> DeviceModel:
    if isinstance(model, DeviceModel):
        return model
    if isinstance(model, str):
        return BY_NAME[model]
    return BY_ID[int(model)]


@dataclass
class CheckResult:
    batch: codec.Batch
    status: np.ndarray
    nodes: np.ndarray
    witness: np.ndarray | None
    totals: dict = field(default_factory=dict)
    # pending="complete" with a witness: per witness level the assumed response
    # symbol, device.QSMD_ASSUMED_NONE for an observed one (the witness layout)
    assumed: np.ndarray | None = field(default=None, kw_only=True)

    def verdict(self, i):
        return codec.STATUS_NAMES[int(self.status[i])]

    def assumed_of(self, i):
        """Per level of history i's witness the assumed response symbol (an
        index into the model's ``resps``), None for an observed response."""
        w = self.witness_of(i)
        if w is None or self.assumed is None:
            return None
        off = int(self.batch.hdr[i]["ev_off"])
        return [None if x == device.QSMD_ASSUMED_NONE else int(x) for x in self.assumed[off: off + len(w)]]

    def witness_of(self, i):
        """Invocation-event indices of the linearisation of history i."""
        if self.witness is None or self.status[i] != codec.STATUS_LIN:
            return None
        h = self.batch.hdr[i]
        w = self.witness[h["ev_off"]: h["ev_off"] + h["n_ev"]]
        out = []
        for x in w:
            if x == codec.WITNESS_END:
                break
            out.append(int(x))
        return out


def linearisable_batch(model, histories, model0=None, *, max_nodes=0, witness=False,
                       flags=device.QSMD_FLAG_EXHAUSTIVE, ctx=None, table_memo=None,
                       ktable_local=None, pending=None, pending_memo=None, kpending_local=None) -> CheckResult:
    """Check many histories in one device call.  ``table_memo`` (table models:
    entries per lane slot of the second pass's state memo, 0 = off) sets the
    context's "table_memo" knob for this call and restores it afterwards;
    with a :class:`KeyedTableModel` the knob is the keyed path's own,
    "ktable_memo".  ``ktable_local`` (a :class:`KeyedTableModel` only): None
    leaves the context's "ktable_local" knob alone, True / False set it for
    this call in the same way -- every splittable history is then checked key
    by key (include/qsmd.h; :meth:`KeyedTableModel.split_history`).

    ``pending`` (a :class:`TableModel` or a :class:`KeyedTableModel`): None is
    the reference's rule -- an invocation that never got its response is an
    operation that never happened.  ``"complete"`` also lets it take effect,
    at any point after its invocation, with any response the model allows
    (qsmd_check_pending_batch, for a keyed model qsmd_check_kpending_batch,
    include/qsmd.h): with ``witness`` the result's ``assumed`` names the
    responses that were assumed.  With raise tables this can read ``error``
    where None reads ``lin``; "table_memo" is ignored, and for a keyed model
    so are "ktable_memo" and "ktable_local" (the plain search on the product).
    ``kpending_local`` (only with ``pending="complete"`` and a
    :class:`KeyedTableModel`): None leaves the context's "kpending_local" knob
    alone, True / False set it for this call and restore it afterwards --
    every history that is splittable with pending invocations
    (:meth:`KeyedTableModel.split_history` with ``pending=True``) is then
    checked key by key; a call with ``witness`` searches the product whole.
    ``pending_memo`` (only with ``pending="complete"`` and a
    :class:`TableModel`: entries per lane slot, 0 = off) sets the pending
    call's own memo knob, "pending_memo", for this call and restores it
    afterwards; every result is the plain call's."""
    m = _as_model(model)
    if pending not in (None, "complete"):
        raise ValueError('pending: None or "complete"')
    if pending_memo is not None and not pending:
        raise ValueError('pending_memo: only with pending="complete"')
    keyed = isinstance(m, KeyedTableModel)
    if pending and not keyed and (not isinstance(m, TableModel) or isinstance(m, WideTableModel)):
        raise NotImplementedError('pending="complete": a TableModel or a KeyedTableModel only '
                                  '(QSMD_MODEL_TABLE, QSMD_MODEL_KTABLE)')
    if pending_memo is not None and keyed:
        raise ValueError("pending_memo: the keyed pending call has no memo")
    if kpending_local is not None and not (pending and keyed):
        raise ValueError('kpending_local: only with a KeyedTableModel and pending="complete"')
    batch = codec.encode(m, histories, model0)
    accounts0 = m.new_account_map(model0)
    packed = m.pack_model0(model0, accounts0)
    ctx = ctx or device.default_context()
    if isinstance(m, WideTableModel):
        if ctx.wide_table is not m:
            ctx.set_wide_table(m)
    elif isinstance(m, TableModel):
        if ctx.table is not m:
            ctx.set_table(m)
    elif isinstance(m, KeyedTableModel) and ctx.keyed_table is not m:
        ctx.set_keyed_table(m)
    saved = None
    knob = "ktable_memo" if isinstance(m, KeyedTableModel) else "table_memo"
    if table_memo is not None:
        saved = ctx.get_param(knob)
        ctx.set_param(knob, table_memo)
    saved_local = None
    if ktable_local is not None and isinstance(m, KeyedTableModel):
        saved_local = ctx.get_param("ktable_local")
        ctx.set_param("ktable_local", 1 if ktable_local else 0)
    saved_pending = None
    if pending_memo is not None:
        saved_pending = ctx.get_param("pending_memo")
        ctx.set_param("pending_memo", pending_memo)
    saved_klocal = None
    if kpending_local is not None:
        saved_klocal = ctx.get_param("kpending_local")
        ctx.set_param("kpending_local", 1 if kpending_local else 0)
    assumed = None
    try:
        if pending and keyed:
            status, nodes, wit, assumed, totals = ctx.check_kpending_arrays(batch.hdr, batch.events, packed, flags,
                                                                            max_nodes, witness)
        elif pending:
            status, nodes, wit, assumed, totals = ctx.check_pending_arrays(m.model_id, batch.hdr, batch.events,
                                                                           packed, flags, max_nodes, witness)
        else:
            status, nodes, wit, totals = ctx.check_arrays(m.model_id, batch.hdr, batch.events, packed,
                                                          flags, max_nodes, witness)
    finally:
        if saved is not None:
            ctx.set_param(knob, saved)
        if saved_local is not None:
            ctx.set_param("ktable_local", saved_local)
        if saved_pending is not None:
            ctx.set_param("pending_memo", saved_pending)
        if saved_klocal is not None:
            ctx.set_param("kpending_local", saved_klocal)
    return CheckResult(batch, status, nodes, wit, totals, assumed=assumed)


def linearisable(transition, postcondition, model0, history, *, max_nodes=0, ctx=None, table_memo=None,
                 ktable_local=None, pending=None, pending_memo=None, kpending_local=None) -> bool:
    """``linearisable`` (src/Linearisability.hs:52-69) on the GPU
    (``table_memo``, ``ktable_local``, ``pending``, ``pending_memo``, ``kpending_local``: see
    :func:`linearisable_batch`)."""
    m = _device_model(transition, postcondition)
    res = linearisable_batch(m, [history], model0, max_nodes=max_nodes, ctx=ctx, table_memo=table_memo,
                             ktable_local=ktable_local, pending=pending, pending_memo=pending_memo,
                             kpending_local=kpending_local)
    st = int(res.status[0])
    if st == codec.STATUS_LIN:
        return True
    if st == codec.STATUS_NONLIN:
        return False
    if st == codec.STATUS_MODEL_ERROR:
        raise ModelError("the postcondition raises" if isinstance(m, (TableModel, KeyedTableModel))
                         else "Map.!: given key is not an element in the map")
    if st == codec.STATUS_ENCODE_ERROR:
        raise EncodeError(res.batch.encode_errors.get(0, "history cannot be encoded"))
    raise BudgetExceeded(f"search stopped after {int(res.nodes[0])} nodes")


# ---------------------------------------------------------------------------
# trace (src/Linearisability.hs:73-93)
# ---------------------------------------------------------------------------

def pretty_print_pid(pid) -> str:
    """``prettyPrintProcessId = reverse . takeWhile (/= ':') . reverse . show``."""
    s = str(pid)
    return s.rsplit(":", 1)[-1]


def trace(transition, model0, history, model: DeviceModel | None = None) -> str:
    """Pretty-print a history with the model state before each event, applied
    in *history* order (src/Linearisability.hs:76-93)."""
    m = model
    if m is None:
        for cand in BY_ID.values():
            if transition is cand.transition:
                m = cand
        if m is None and isinstance(getattr(transition, "__self__", None), (TableModel, KeyedTableModel)):
            m = transition.__self__
        if m is None:
            raise NotImplementedError("trace needs a DeviceModel to show values")
    out = []
    cur = model0
    for pid, ev in history:
        kind, x = ev
        if kind == "L":
            out.append(f"{m.show_model(cur)}\n  ==> {m.show_inv(x)}  [{pretty_print_pid(pid)}]\n")
        else:
            out.append(f"{m.show_model(cur)}\n  <== {m.show_resp(x)}  [{pretty_print_pid(pid)}]\n")
        cur = transition(cur, ev)
    return "".join(out)


# ---------------------------------------------------------------------------
# wellformed (src/Linearisability.hs:97-135)
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class NotSequential:
    """``NotSequential`` constructors (src/Linearisability.hs:97-104)."""
    kind: str
    args: tuple


def _is_sequential(history):
    """``isSequential`` (src/Linearisability.hs:109-128)."""
    if history and history[0][1][0] == "R":
        pid, (_, resp) = history[0]
        return NotSequential("FirstEventIsntInvocation", (pid, resp))
    i = 0
    n = len(history)
    while True:
        rest = n - i
        if rest == 0:
            return None
        p0, (k0, x0) = history[i]
        if rest == 1:
            return NotSequential("LoneResponse", (p0, x0)) if k0 == "R" else None
        p1, (k1, x1) = history[i + 1]
        if k0 == "L" and k1 == "R":
            if p0 == p1:
                i += 2
                continue
            return NotSequential("InvocationFollowedByNonMatchingResponse", (p0, x0, p1, x1))
        if k0 == "L" and k1 == "L":
            return NotSequential("InvocationFollowedByInvocation", (p0, x0, p1, x1))
        if k0 == "R" and k1 == "R":
            return NotSequential("ResponseFollowedByResponse", (p0, x0, p1, x1))
        return NotSequential("ResponseFollowedByInvocation", (p0, x0, p1, x1))


def wellformed_batch(pids, histories, ctx=None):
    """Batched ``wellformed pids history`` on the GPU (csrc/wellformed.hip,
    src/Linearisability.hs:130-135, call site test/Bank.hs:281-283): for each
    history None (``Right ()``) or the first :class:`NotSequential`, checking
    each pid's subhistory in ``pids`` order.  Same results as
    :func:`wellformed` one history at a time."""
    from . import codec, device
    hdr, events, pid_index = codec.encode_shape(histories)
    ranks = [pid_index[p] for p in pids if p in pid_index]
    own = ctx is None
    if own:
        ctx = device.Context(0)
    try:
        res = ctx.wellformed_arrays(hdr, events, ranks)
    finally:
        if own:
            ctx.close()
    out = []
    for h, r in zip(histories, res):
        code = int(r["code"])
        if code == 0:
            out.append(None)
            continue
        if code == codec.WF_ENCODE_ERROR:
            raise ValueError("history not encodable")
        e0, e1 = h[int(r["ev0"])], h[int(r["ev1"])]
        kind = codec.WF_KINDS[code]
        if kind in ("FirstEventIsntInvocation", "LoneResponse"):
            out.append(NotSequential(kind, (e0[0], e0[1][1])))
        else:
            out.append(NotSequential(kind, (e0[0], e0[1][1], e1[0], e1[1][1])))
    return out


def wellformed(pids, history):
    """Returns None (``Right ()``) or the first :class:`NotSequential`
    (``Left err``), checking each pid's subhistory in ``pids`` order."""
    for pid in pids:
        err = _is_sequential([e for e in history if e[0] == pid])
        if err is not None:
            return err
    return None


# ---------------------------------------------------------------------------
# witness replay (host re-check of a GPU linearisation)
# ---------------------------------------------------------------------------

def _replay_pending(m, history, witness, model0, assumed) -> bool:
    """:func:`replay_witness` under ``pending="complete"`` (a TableModel or a
    KeyedTableModel): ``assumed[d]`` is None for an observed level, else the
    index of the response symbol assumed there."""
    if len(assumed) != len(witness):
        return False
    cur = m.init_model if model0 is None else model0
    removed = set()

    def allowed(state, inv):
        t = m
        if isinstance(m, KeyedTableModel):      # the component's tables at that key's state
            k, inv = m._split(inv)
            t, state = m.component, m._model(state)[k]
        s, i = t._state(state), t.encode_inv(inv, None)[0]
        err = 0 if t.post_err is None else int(t.post_err[s, i])
        return int(t.post[s, i]) & ~err & ((1 << len(t.resps)) - 1)

    for j, a in zip(witness, assumed):
        if not 0 <= j < len(history) or j in removed or history[j][1][0] != "L":
            return False
        pid, (_, inv) = history[j]
        first_resp = _first(history, removed, "R")
        if first_resp is not None and j > first_resp:
            return False
        r = _first(history, removed, "R", pid)
        if a is None:
            if r is None:
                return False
            resp = history[r][1][1]
            if not m.postcondition(cur, inv, resp):
                return False
            removed.add(r)
        else:
            # assumed: the pid has no remaining response there, the model allows the symbol
            if r is not None or not 0 <= a < len(m.resps) or not (allowed(cur, inv) >> a) & 1:
                return False
            resp = m.resps[a]
        cur = m.transition(m.transition(cur, ("L", inv)), ("R", resp))
        removed.add(_first(history, removed, "L", pid))
    if not witness and any(k == "R" for _, (k, _) in history):
        return False                    # the root without a child succeeds only with no response at all
    # a leaf: no candidate has a child, observed or assumed
    first_resp = _first(history, removed, "R")
    for i, (p, (k, inv)) in enumerate(history[:len(history) if first_resp is None else first_resp]):
        if i in removed or k != "L":
            continue
        if _first(history, removed, "R", p) is not None or allowed(cur, inv):
            return False
    return True


def replay_witness(model, history, witness, model0=None, assumed=None) -> bool:
    """Re-run the operations named by ``witness`` (invocation event indices,
    one per level) with the host model: each step pairs the chosen
    invocation with the first remaining response of its pid and removes the
    first remaining invocation and response of that pid (Lemma L1).  True iff
    every postcondition holds and the final state has no further child.

    ``assumed`` (``pending="complete"``, a :class:`TableModel` or a
    :class:`KeyedTableModel`): one entry
    per level, None for an observed response or the index of the response
    symbol assumed there (:meth:`CheckResult.assumed_of`).  An assumed level is
    replayed with the named response: its pid must have no remaining response
    there, the model must allow the symbol, and only the invocation is
    removed."""
    m = _as_model(model)
    if assumed is not None:
        return _replay_pending(m, list(history), [int(j) for j in witness], model0, list(assumed))
    if not witness:                     # only `linearisable _ _ _ [] = True` (:59)
        return len(history) == 0
    cur = m.init_model if model0 is None else model0
    removed = set()
    for j in witness:
        pid, (kind, inv) = history[j]
        if kind != "L" or j in removed:
            return False
        # first remaining response of this pid must come after every remaining
        # invocation we could pick (takeInvocations prefix)
        first_resp = next((i for i, (p, (k, _)) in enumerate(history)
                           if i not in removed and k == "R"), len(history))
        if j > first_resp:
            return False
        r = next((i for i, (p, (k, _)) in enumerate(history)
                  if i not in removed and k == "R" and p == pid), None)
        if r is None:
            return False
        resp = history[r][1][1]
        if not m.postcondition(cur, inv, resp):
            return False
        cur = m.transition(m.transition(cur, ("L", inv)), ("R", resp))
        i0 = next(i for i, (p, (k, _)) in enumerate(history)
                  if i not in removed and k == "L" and p == pid)
        removed.add(i0)
        removed.add(r)
    # leaf: no remaining invocation before the first remaining response has a response
    first_resp = next((i for i, (p, (k, _)) in enumerate(history)
                       if i not in removed and k == "R"), len(history))
    for i, (p, (k, _)) in enumerate(history[:first_resp]):
        if i in removed or k != "L":
            continue
        if any(ii not in removed and kk == "R" and pp == p
               for ii, (pp, (kk, _)) in enumerate(history)):
            return False
    return True


# ---------------------------------------------------------------------------
# explain: the deepest linearised path of a search (include/qsmd.h
# qsmd_explain_batch; the table models)
# ---------------------------------------------------------------------------

def _first(history, removed, kind, pid=None):
    """The first remaining event of ``kind`` (of ``pid``), or None."""
    return next((i for i, (p, (k, _)) in enumerate(history)
                 if i not in removed and k == kind and (pid is None or p == pid)), None)


@dataclass
class Explanation:
    """Where the search of one history stood at the end of its reported path.

    ``prefix``: the path's operations ``(pid, inv, resp)``; ``model``: the
    model value after them; ``stuck``: for every candidate there (the
    remaining invocations below the first remaining response, in order)
    ``(pid, inv, resp or None, outcome)``, the outcome one of ``"no response"``
    (the pid has no remaining response: no child), ``"postcondition false"``,
    ``"raises"`` and -- never on a NONLINEARISABLE path, whose end is a node
    no candidate passes; on a BUDGET path (the search stopped early) or a
    MODEL_ERROR path (an earlier candidate's subtree failed before the raising
    one was tried) -- ``"passes"``."""
    status: str
    prefix: list
    model: object
    stuck: list
    model0: object = None
    device_model: DeviceModel | None = None

    def pretty(self) -> str:
        """The prefix in the format of :func:`trace` (the model before each
        event, the operations in path order), then the model reached and one
        line per stuck candidate."""
        m = self.device_model
        hist = []
        for pid, inv, resp in self.prefix:
            hist += [(pid, ("L", inv)), (pid, ("R", resp))]
        out = [trace(m.transition, self.model0, hist, model=m), f"{m.show_model(self.model)}\n"]
        for pid, inv, resp, outcome in self.stuck:
            r = "" if resp is None else f" <== {m.show_resp(resp)}"
            out.append(f"  =/=> {m.show_inv(inv)}{r}  [{pretty_print_pid(pid)}]: {outcome}\n")
        return "".join(out)


def explanation_from_path(model, history, path, status, model0=None) -> Explanation:
    """The :class:`Explanation` a reported path stands for (pure host code).

    ``path``: invocation event indices, one per level, replayed by the rule of
    :func:`replay_witness` -- each step pairs the chosen invocation with the
    first remaining response of its pid and removes the pid's first remaining
    invocation and that response; the model is advanced with the model's own
    ``transition``.  ``status``: a status name or number (it is only carried
    along).  ValueError for a path that is no path of this history."""
    m = _as_model(model)
    history = list(history)
    start = m.init_model if model0 is None else model0
    cur = start
    removed, prefix = set(), []
    for j in path:
        j = int(j)
        if not 0 <= j < len(history) or j in removed or history[j][1][0] != "L":
            raise ValueError(f"path entry {j}: not a remaining invocation")
        pid, (_, inv) = history[j]
        r = _first(history, removed, "R", pid)
        if r is None:
            raise ValueError(f"path entry {j}: its pid has no remaining response")
        resp = history[r][1][1]
        prefix.append((pid, inv, resp))
        cur = m.transition(m.transition(cur, ("L", inv)), ("R", resp))
        removed |= {_first(history, removed, "L", pid), r}
    first_resp = _first(history, removed, "R")
    stuck = []
    for i, (pid, (kind, inv)) in enumerate(history[:len(history) if first_resp is None else first_resp]):
        if i in removed or kind != "L":
            continue
        r = _first(history, removed, "R", pid)
        if r is None:
            stuck.append((pid, inv, None, "no response"))
            continue
        resp = history[r][1][1]
        try:
            outcome = "passes" if m.postcondition(cur, inv, resp) else "postcondition false"
        except ModelError:
            outcome = "raises"
        stuck.append((pid, inv, resp, outcome))
    name = status if isinstance(status, str) else codec.STATUS_NAMES[int(status)]
    return Explanation(name, prefix, cur, stuck, start, m)


@dataclass
class ExplainResult(CheckResult):
    """:class:`CheckResult` of an explain call: ``witness`` holds the reported
    paths (the witness layout), ``depth`` / ``state`` the qsmd_explain records."""
    histories: list = field(default_factory=list)
    depth: np.ndarray | None = None
    state: np.ndarray | None = None
    model0: object = None

    def path_of(self, i):
        """Invocation-event indices of history i's reported path."""
        h = self.batch.hdr[i]
        out = []
        for x in self.witness[h["ev_off"]: h["ev_off"] + h["n_ev"]]:
            if x == codec.WITNESS_END:
                break
            out.append(int(x))
        return out

    def witness_of(self, i):
        return self.path_of(i) if self.status[i] == codec.STATUS_LIN else None

    def state_of(self, i):
        """The device's state record of history i as a model value."""
        return decode_state(self.batch.model, int(self.state[i]))

    def explanation(self, i) -> Explanation:
        if self.status[i] == codec.STATUS_ENCODE_ERROR:
            raise EncodeError(self.batch.encode_errors.get(i, "history cannot be encoded"))
        e = explanation_from_path(self.batch.model, self.histories[i], self.path_of(i), int(self.status[i]),
                                  self.model0)
        if len(e.prefix) != int(self.depth[i]) or tuple_or(e.model) != tuple_or(self.state_of(i)):
            raise RuntimeError(f"history {i}: the path does not replay to the device's record")
        return e


def tuple_or(x):
    """A keyed model's value as a plain tuple (its in-between values compare
    as one, but print their class); any other value as it is."""
    return tuple(x) if isinstance(x, tuple) else x


def decode_state(model, word):
    """A qsmd_explain ``state`` word as a value of ``model``: the state index
    (table and wide table models), key k's component state index in bits
    8k .. 8k + 7 (keyed models)."""
    m = _as_model(model)
    if isinstance(m, KeyedTableModel):
        return tuple(m.component.states[(word >> (8 * k)) & 0xFF] for k in range(m.n_keys))
    if isinstance(m, TableModel):
        return m.states[word]
    raise NotImplementedError("explain: the table models only")


def explain_batch(model, histories, model0=None, *, max_nodes=0, ctx=None) -> ExplainResult:
    """Explain many histories in one device call (qsmd_explain_batch; a
    :class:`TableModel`, :class:`WideTableModel` or :class:`KeyedTableModel`):
    status and nodes of :func:`linearisable_batch` without a memo, and per
    history the deepest linearised path of the search -- always the plain
    search, for a keyed model on the product; a history whose search passes
    ``max_nodes`` reads ``budget`` with the deepest path seen so far."""
    m = _as_model(model)
    if not isinstance(m, (TableModel, KeyedTableModel)):
        raise NotImplementedError("explain: the table models only (TableModel, WideTableModel, KeyedTableModel)")
    histories = [list(h) for h in histories]
    batch = codec.encode(m, histories, model0)
    packed = m.pack_model0(model0, m.new_account_map(model0))
    ctx = ctx or device.default_context()
    if isinstance(m, WideTableModel):
        if ctx.wide_table is not m:
            ctx.set_wide_table(m)
    elif isinstance(m, TableModel):
        if ctx.table is not m:
            ctx.set_table(m)
    elif ctx.keyed_table is not m:
        ctx.set_keyed_table(m)
    status, nodes, path, rec, totals = ctx.explain_arrays(m.model_id, batch.hdr, batch.events, packed,
                                                          device.QSMD_FLAG_EXHAUSTIVE, max_nodes)
    return ExplainResult(batch, status, nodes, path, totals, histories, rec["depth"].copy(), rec["state"].copy(),
                         model0)


def explain(transition, postcondition, model0, history, *, max_nodes=0, ctx=None) -> Explanation:
    """:func:`explain_batch` for one history, with :func:`linearisable`'s
    signature: the :class:`Explanation` of its search (``.status`` says how it
    ended; :class:`EncodeError` for a history that cannot be encoded)."""
    m = _device_model(transition, postcondition)
    return explain_batch(m, [history], model0, max_nodes=max_nodes, ctx=ctx).explanation(0)
