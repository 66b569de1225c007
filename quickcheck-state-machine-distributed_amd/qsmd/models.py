"""Device models: the user closures the reference passes to ``linearisable``.

The reference's search calls only the model closures its callers pass
(``src/Linearisability.hs:52-58``).  On the GPU those closures are compiled
device functors (``csrc/models.hip``); this module is their host side:

* the constructor <-> code tables of include/qsmd.h,
* the Haskell model functions themselves (used on the host for ``trace``
  printing and witness replay, never for the search),
* ``init_model`` and the packing of a non-default ``model0``.

Values use the same shapes as the Haskell constructors:

TicketDispenser (test/TicketDispenser.hs:51-102)
    inv  ``'TakeTicket' | 'Reset'``
    resp ``('Number', i) | 'Ok'``
    model ``None`` (Nothing) | ``int`` (Just n)

Bank (test/Bank.hs:41-131)
    inv  ``('OpenAccount', a) | ('Deposit', a, m) | ('Withdraw', a, m)
         | ('CheckBalance', a) | ('Transfer', a, m, b)``
    resp ``'AccountCreated' | 'DepositMade' | 'WithdrawalMade' |
         'TransferMade' | 'AccountAlreadyExists' | 'AccountDoesntExist' |
         'InsufficientFunds' | ('Balance', v)``
    model ``dict`` account -> int (Data.Map, treated as immutable)
"""

from __future__ import annotations

import ctypes

MODEL_TICKET = 1
MODEL_BANK = 2

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
BANK_MAX_ACCOUNTS = 8


class ModelError(Exception):
    """The reference model raises (Haskell exception), e.g. ``Map.!`` on a
    missing account in Bank's ``post`` (test/Bank.hs:128)."""


class EncodeError(ValueError):
    """A value cannot be represented in the include/qsmd.h encoding."""


def _i32(v):
    if not isinstance(v, int) or isinstance(v, bool) or not (I32_MIN <= v <= I32_MAX):
        raise EncodeError(f"value {v!r} outside int32")
    return v


class DeviceModel:
    """Host half of a device functor pair (transition, postcondition)."""

    name = ""
    model_id = 0

    # -- Haskell semantics (host replay / trace only) ---------------------
    @staticmethod
    def transition(model, ev):
        raise NotImplementedError

    @staticmethod
    def postcondition(model, inv, resp):
        raise NotImplementedError

    init_model = None

    # -- encoding ----------------------------------------------------------
    def new_account_map(self, model0):
        return {}

    def encode_inv(self, inv, accounts):
        raise NotImplementedError

    def encode_resp(self, resp):
        raise NotImplementedError

    def pack_model0(self, model0, accounts):
        """Return a ctypes struct for ``model0`` or None for init_model."""
        raise NotImplementedError

    def show_model(self, model):
        return repr(model)

    def show_inv(self, inv):
        return repr(inv)

    def show_resp(self, resp):
        return repr(resp)


# ---------------------------------------------------------------------------
# TicketDispenser
# ---------------------------------------------------------------------------

class TicketModel(ctypes.Structure):
    _fields_ = [("is_just", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("n", ctypes.c_int64)]


class TicketDispenser(DeviceModel):
    name = "ticket"
    model_id = MODEL_TICKET
    init_model = None                               # Nothing

    INV = {"TakeTicket": 0, "Reset": 1}
    INV_NAMES = {v: k for k, v in INV.items()}

    @staticmethod
    def transition(m, ev):                          # TicketDispenser.hs:81-85
        kind, x = ev
        if kind == "R":
            return m
        if x == "TakeTicket":
            return None if m is None else m + 1
        return 0

    @staticmethod
    def postcondition(m, inv, resp):                # TicketDispenser.hs:99-102
        if inv == "TakeTicket" and isinstance(resp, tuple) and resp[0] == "Number":
            return m is not None and resp[1] == m + 1
        return inv == "Reset" and resp == "Ok"

    def encode_inv(self, inv, accounts):
        if inv not in self.INV:
            raise EncodeError(f"unknown TicketDispenser request {inv!r}")
        return self.INV[inv], 0, 0, 0

    def encode_resp(self, resp):
        if resp == "Ok":
            return 1, 0
        if isinstance(resp, tuple) and len(resp) == 2 and resp[0] == "Number":
            return 0, _i32(resp[1])
        raise EncodeError(f"unknown TicketDispenser response {resp!r}")

    def decode_inv(self, code, a, b, val, accounts):
        return self.INV_NAMES[code]

    def decode_resp(self, code, val):
        return ("Number", val) if code == 0 else "Ok"

    def pack_model0(self, model0, accounts):
        if model0 is None:
            return None
        return TicketModel(1, 0, _i32(model0))

    def show_model(self, m):
        return "Nothing" if m is None else f"Just {m}"

    def show_inv(self, inv):
        return inv

    def show_resp(self, resp):
        return "Ok" if resp == "Ok" else f"Number {resp[1]}"


# ---------------------------------------------------------------------------
# Bank
# ---------------------------------------------------------------------------

class BankModel(ctypes.Structure):
    _fields_ = [("exists", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("balance", ctypes.c_int64 * BANK_MAX_ACCOUNTS)]


BANK_REQ = {"OpenAccount": 0, "Deposit": 1, "Withdraw": 2, "CheckBalance": 3, "Transfer": 4}
BANK_REQ_NAMES = {v: k for k, v in BANK_REQ.items()}
BANK_RESP = {"AccountCreated": 0, "DepositMade": 1, "WithdrawalMade": 2, "TransferMade": 3,
             "AccountAlreadyExists": 4, "AccountDoesntExist": 5, "InsufficientFunds": 6}
BANK_RESP_NAMES = {v: k for k, v in BANK_RESP.items()}
BANK_BALANCE = 7


def _bank_deposit(model, a, money):
    m2 = dict(model)
    m2[a] = model[a] + money if a in model else money
    return m2


def _bank_withdraw(model, a, money):
    m2 = dict(model)
    m2[a] = model[a] - money if a in model else money
    return m2


class Bank(DeviceModel):
    name = "bank"
    model_id = MODEL_BANK

    @property
    def init_model(self):                           # M.empty
        return {}

    @staticmethod
    def transition(model, ev):                      # Bank.hs:92-101  (next')
        kind, x = ev
        if kind == "R":
            return model
        op = x[0]
        if op == "OpenAccount":
            if x[1] in model:
                return model
            m2 = dict(model)
            m2[x[1]] = 0
            return m2
        if op == "Deposit":
            return _bank_deposit(model, x[1], x[2])
        if op == "Withdraw":
            return _bank_withdraw(model, x[1], x[2])
        if op == "CheckBalance":
            return model
        if op == "Transfer":
            return _bank_deposit(_bank_withdraw(model, x[1], x[2]), x[3], x[2])
        raise ValueError(x)

    @staticmethod
    def postcondition(model, req, resp):            # Bank.hs:118-131  (post)
        if not all(v >= 0 for v in model.values()):     # invariant, :103-104
            return False
        op = req[0]
        if op == "OpenAccount":
            return resp == ("AccountAlreadyExists" if req[1] in model else "AccountCreated")
        if op == "Deposit":
            return resp == "DepositMade"
        if op in ("Withdraw", "Transfer"):
            ok = req[1] in model and model[req[1]] >= req[2]
            made = "WithdrawalMade" if op == "Withdraw" else "TransferMade"
            return resp == (made if ok else "InsufficientFunds")
        if op == "CheckBalance":
            if isinstance(resp, tuple) and resp[0] == "Balance":
                if req[1] not in model:
                    raise ModelError("Map.!: given key is not an element in the map")
                return resp[1] == model[req[1]]
            return False
        raise ValueError(req)

    # accounts are arbitrary Eq/Ord values (ProcessIds in the reference);
    # each history maps them to dense indices 0..7 in order of first mention,
    # after the keys of a non-empty model0.
    def new_account_map(self, model0):
        accounts = {}
        for k in (model0 or {}):
            accounts[k] = len(accounts)
        return accounts

    @staticmethod
    def _acc(accounts, a):
        if a not in accounts:
            if len(accounts) >= BANK_MAX_ACCOUNTS:
                raise EncodeError("more than 8 accounts in one history")
            accounts[a] = len(accounts)
        return accounts[a]

    def encode_inv(self, req, accounts):
        if not isinstance(req, tuple) or not req or req[0] not in BANK_REQ:
            raise EncodeError(f"unknown Bank request {req!r}")
        op = req[0]
        code = BANK_REQ[op]
        if op in ("OpenAccount", "CheckBalance"):
            if len(req) != 2:
                raise EncodeError(repr(req))
            return code, self._acc(accounts, req[1]), 0, 0
        if op in ("Deposit", "Withdraw"):
            if len(req) != 3:
                raise EncodeError(repr(req))
            return code, self._acc(accounts, req[1]), 0, _i32(req[2])
        if len(req) != 4:
            raise EncodeError(repr(req))
        a = self._acc(accounts, req[1])
        b = self._acc(accounts, req[3])
        return code, a, b, _i32(req[2])

    def encode_resp(self, resp):
        if isinstance(resp, tuple) and len(resp) == 2 and resp[0] == "Balance":
            return BANK_BALANCE, _i32(resp[1])
        if isinstance(resp, str) and resp in BANK_RESP:
            return BANK_RESP[resp], 0
        raise EncodeError(f"unknown Bank response {resp!r}")

    def decode_inv(self, code, a, b, val, accounts):
        inv_acc = {v: k for k, v in accounts.items()}
        op = BANK_REQ_NAMES[code]
        if op in ("OpenAccount", "CheckBalance"):
            return (op, inv_acc[a])
        if op in ("Deposit", "Withdraw"):
            return (op, inv_acc[a], val)
        return (op, inv_acc[a], val, inv_acc[b])

    def decode_resp(self, code, val):
        return ("Balance", val) if code == BANK_BALANCE else BANK_RESP_NAMES[code]

    def pack_model0(self, model0, accounts):
        if not model0:
            return None
        m = BankModel()
        for k, v in model0.items():
            idx = accounts[k]
            m.exists |= 1 << idx
            m.balance[idx] = _i32(v)
        return m

    def show_model(self, model):
        items = ",".join(f"({k!r},{v})" for k, v in sorted(model.items(), key=lambda kv: repr(kv[0])))
        return f"fromList [{items}]"

    def show_inv(self, req):
        return " ".join(str(x) for x in req)

    def show_resp(self, resp):
        return resp if isinstance(resp, str) else f"Balance {resp[1]}"


# ---------------------------------------------------------------------------
# Table-driven models (include/qsmd.h QSMD_MODEL_TABLE)
# ---------------------------------------------------------------------------

MODEL_TABLE = 3
TABLE_MAX_STATES = 256
TABLE_MAX_SYMBOLS = 32


class TableModelStruct(ctypes.Structure):
    """``qsmd_table_model``."""
    _fields_ = [("n_states", ctypes.c_uint32), ("n_inv", ctypes.c_uint32),
                ("n_resp", ctypes.c_uint32), ("init_state", ctypes.c_uint32),
                ("on_inv", ctypes.c_void_p), ("on_resp", ctypes.c_void_p),
                ("post", ctypes.c_void_p), ("post_err", ctypes.c_void_p)]


class TableModel(DeviceModel):
    """Any finite-state model as run-time tables: no device functor, no
    recompile.  ``states``, ``invs`` and ``resps`` are lists of hashable
    values (at most 256 / 32 / 32); a step from state ``s`` with invocation
    ``i`` and response ``r`` (indices) is

        postcondition = bit r of post[s][i]      (post_err: it raises)
        next state    = on_resp[on_inv[s][i]][r]

    ``transition`` and ``postcondition`` are the table lookups on the state
    *values*, with the reference's signatures, so
    ``linearisable(m.transition, m.postcondition, model0, history)`` finds
    ``m``.  Build one from explicit tables or from closures
    (:meth:`from_closures`)."""

    name = "table"
    model_id = MODEL_TABLE
    # the limits and the table formats (WideTableModel widens them)
    MAX_STATES = TABLE_MAX_STATES
    MAX_SYMBOLS = TABLE_MAX_SYMBOLS
    STATE_DTYPE = "uint8"

    @staticmethod
    def _post_shape(ns, ni, nr):
        return (ns, ni)

    @staticmethod
    def _post_entry(bits, nr):
        """A postcondition bitset (a Python int, bit r = response r) as a table entry."""
        return bits

    @staticmethod
    def _post_bit(entry, r):
        return (int(entry) >> r) & 1

    def __init__(self, states, invs, resps, on_inv, on_resp, post, post_err=None, init_state=0):
        import numpy as np
        self.states, self.invs, self.resps = list(states), list(invs), list(resps)
        ns, ni, nr = len(self.states), len(self.invs), len(self.resps)
        if not 1 <= ns <= self.MAX_STATES:
            raise EncodeError(f"{ns} states: a {self.name} model has 1..{self.MAX_STATES}")
        if not 1 <= ni <= self.MAX_SYMBOLS or not 1 <= nr <= self.MAX_SYMBOLS:
            raise EncodeError(f"{ni} invocation / {nr} response symbols: a {self.name} model has "
                              f"1..{self.MAX_SYMBOLS} of each")
        self.state_index = {v: k for k, v in enumerate(self.states)}
        self.inv_index = {v: k for k, v in enumerate(self.invs)}
        self.resp_index = {v: k for k, v in enumerate(self.resps)}
        if len(self.state_index) != ns or len(self.inv_index) != ni or len(self.resp_index) != nr:
            raise EncodeError("states, invs and resps must each be distinct values")

        def table(x, shape, dtype, what):
            arr = np.asarray(x)
            if arr.shape != shape or not np.issubdtype(arr.dtype, np.integer):
                raise EncodeError(f"{what}: an integer array of shape {shape}")
            if arr.size and (arr.min() < 0 or arr.max() > np.iinfo(dtype).max):
                raise EncodeError(f"{what}: entry out of range")
            return np.ascontiguousarray(arr.astype(dtype))

        sdt, pshape = np.dtype(self.STATE_DTYPE).type, self._post_shape(ns, ni, nr)
        self.on_inv = table(on_inv, (ns, ni), sdt, "on_inv")
        self.on_resp = table(on_resp, (ns, nr), sdt, "on_resp")
        self.post = table(post, pshape, np.uint32, "post")
        self.post_err = None if post_err is None else table(post_err, pshape, np.uint32, "post_err")
        if self.on_inv.max() >= ns or self.on_resp.max() >= ns:
            raise EncodeError("on_inv / on_resp: entry >= n_states")
        if not 0 <= int(init_state) < ns:
            raise EncodeError("init_state >= n_states")
        self.init_state = int(init_state)

    @classmethod
    def from_closures(cls, transition, postcondition, init_model, invs, resps, raises=ModelError):
        """Tabulate ``transition`` / ``postcondition`` (the reference's
        closures, src/Linearisability.hs:52-58) over the states reachable
        from ``init_model``: breadth-first, each state's successors under
        every ``("L", inv)`` in ``invs`` order and then every ``("R", resp)``
        in ``resps`` order, so state 0 is ``init_model`` and the numbering is
        reproducible.  A ``postcondition`` that raises ``raises`` becomes a
        post_err bit.  :class:`EncodeError` past the class's limits (256
        states and 32 symbols; :class:`WideTableModel`: 65,536 and 256)."""
        invs, resps = list(invs), list(resps)
        if len(invs) > cls.MAX_SYMBOLS or len(resps) > cls.MAX_SYMBOLS:
            raise EncodeError(f"{len(invs)} invocation / {len(resps)} response symbols > {cls.MAX_SYMBOLS}")
        states, index = [init_model], {init_model: 0}
        on_inv, on_resp = [], []
        k = 0
        while k < len(states):
            s = states[k]
            rows = []
            for evs in ([("L", x) for x in invs], [("R", x) for x in resps]):
                row = []
                for ev in evs:
                    t = transition(s, ev)
                    if t not in index:
                        if len(states) >= cls.MAX_STATES:
                            raise EncodeError(f"more than {cls.MAX_STATES} reachable states")
                        index[t] = len(states)
                        states.append(t)
                    row.append(index[t])
                rows.append(row)
            on_inv.append(rows[0])
            on_resp.append(rows[1])
            k += 1
        post = [[0] * len(invs) for _ in states]
        err = [[0] * len(invs) for _ in states]
        any_err = False
        for si, s in enumerate(states):
            for ii, inv in enumerate(invs):
                for ri, resp in enumerate(resps):
                    try:
                        if postcondition(s, inv, resp):
                            post[si][ii] |= 1 << ri
                    except raises:
                        err[si][ii] |= 1 << ri
                        any_err = True
        nr = len(resps)
        post = [[cls._post_entry(b, nr) for b in row] for row in post]
        err = [[cls._post_entry(b, nr) for b in row] for row in err] if any_err else None
        return cls(states, invs, resps, on_inv, on_resp, post, err, 0)

    @property
    def init_model(self):
        return self.states[self.init_state]

    def _state(self, m):
        try:
            return self.state_index[m]
        except (KeyError, TypeError):
            raise EncodeError(f"not a state of this table model: {m!r}") from None

    # bound methods: linearisable() finds the model through their __self__
    def transition(self, m, ev):
        kind, x = ev
        s = self._state(m)
        if kind == "L":
            return self.states[self.on_inv[s, self.encode_inv(x, None)[0]]]
        return self.states[self.on_resp[s, self.encode_resp(x)[0]]]

    def postcondition(self, m, inv, resp):
        s, i, r = self._state(m), self.encode_inv(inv, None)[0], self.encode_resp(resp)[0]
        if self.post_err is not None and self._post_bit(self.post_err[s, i], r):
            raise ModelError(f"postcondition raises: {self.show_model(m)}, {self.show_inv(inv)}, "
                             f"{self.show_resp(resp)}")
        return bool(self._post_bit(self.post[s, i], r))

    def encode_inv(self, inv, accounts):
        try:
            return self.inv_index[inv], 0, 0, 0
        except (KeyError, TypeError):
            raise EncodeError(f"unknown invocation symbol {inv!r}") from None

    def encode_resp(self, resp):
        try:
            return self.resp_index[resp], 0
        except (KeyError, TypeError):
            raise EncodeError(f"unknown response symbol {resp!r}") from None

    def decode_inv(self, code, a, b, val, accounts):
        return self.invs[code]

    def decode_resp(self, code, val):
        return self.resps[code]

    def pack_model0(self, model0, accounts):
        if model0 is None:
            return None
        return ctypes.c_uint32(self._state(model0))

    def c_struct(self):
        """The ``qsmd_table_model`` (``qsmd_wtable_model``) of this model
        (pointers into its arrays, which live as long as the model)."""
        return TableModelStruct(len(self.states), len(self.invs), len(self.resps), self.init_state,
                                self.on_inv.ctypes.data, self.on_resp.ctypes.data, self.post.ctypes.data,
                                None if self.post_err is None else self.post_err.ctypes.data)


# ---------------------------------------------------------------------------
# Wide table-driven models (include/qsmd.h QSMD_MODEL_WTABLE)
# ---------------------------------------------------------------------------

MODEL_WTABLE = 4
WTABLE_MAX_STATES = 65536
WTABLE_MAX_SYMBOLS = 256


class WideTableModel(TableModel):
    """A :class:`TableModel` beyond its limits: up to 65,536 states and 256
    invocation / 256 response symbols (``QSMD_MODEL_WTABLE``; the kernel reads
    the tables from device memory, so a model that fits a
    :class:`TableModel` is checked faster as one).  ``on_inv`` / ``on_resp``
    are ``uint16``; ``post`` / ``post_err`` have shape ``(n_states, n_inv,
    post_words)`` with ``post_words = ceil(n_resp / 32)``, response ``r`` being
    bit ``r & 31`` of word ``r >> 5``.  Everything else -- the step, the
    methods, :meth:`from_closures` and its numbering -- is
    :class:`TableModel`'s.  The device copy is held to
    ``QSMD_WTABLE_MAX_BYTES`` (64 MiB) by ``Context.set_wide_table``."""

    name = "wtable"
    model_id = MODEL_WTABLE
    MAX_STATES = WTABLE_MAX_STATES
    MAX_SYMBOLS = WTABLE_MAX_SYMBOLS
    STATE_DTYPE = "uint16"

    @staticmethod
    def _post_shape(ns, ni, nr):
        return (ns, ni, (nr + 31) // 32)

    @staticmethod
    def _post_entry(bits, nr):
        return [(bits >> (32 * k)) & 0xFFFFFFFF for k in range((nr + 31) // 32)]

    @staticmethod
    def _post_bit(entry, r):
        return (int(entry[r >> 5]) >> (r & 31)) & 1


# ---------------------------------------------------------------------------
# Keyed table models (include/qsmd.h QSMD_MODEL_KTABLE)
# ---------------------------------------------------------------------------

MODEL_KTABLE = 5
KTABLE_MAX_KEYS = 8


class _Invoked(tuple):
    """The product state between ``transition m (Left (key, inv))`` and
    ``transition m' (Right resp)`` (src/Linearisability.hs:64): a response
    names no key, so the intermediate value remembers the invocation's.  It
    compares and hashes as the plain tuple."""
    key = None


class KeyedTableModel(DeviceModel):
    """A map of small states: ``n_keys`` (1..8) independent copies of one
    ``component`` (a :class:`TableModel`, not a wide one), checked as the
    product model without tabulating it (``QSMD_MODEL_KTABLE``).

    Model values are tuples of ``n_keys`` component state values, invocation
    values are ``(key, inv)`` with ``inv`` one of the component's, responses
    are the component's.  A step from ``s`` with ``(k, i)`` and ``r`` checks
    the component's postcondition at ``s[k]`` and replaces ``s[k]`` by the
    component's next state; every other key is unchanged.  ``transition`` and
    ``postcondition`` are bound methods over those values, so
    ``linearisable(m.transition, m.postcondition, model0, history)`` finds
    ``m``."""

    name = "ktable"
    model_id = MODEL_KTABLE

    def __init__(self, component, n_keys):
        if not isinstance(component, TableModel) or isinstance(component, WideTableModel):
            raise EncodeError("the component of a keyed model is a TableModel (256 states, 32 symbols)")
        if isinstance(n_keys, bool) or not isinstance(n_keys, int) or not 1 <= n_keys <= KTABLE_MAX_KEYS:
            raise EncodeError(f"n_keys {n_keys!r}: a keyed model has 1..{KTABLE_MAX_KEYS} keys")
        self.component = component
        self.n_keys = n_keys
        self.resps = component.resps
        self.invs = [(k, i) for k in range(n_keys) for i in component.invs]

    @property
    def init_model(self):
        return (self.component.init_model,) * self.n_keys

    def _key(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < self.n_keys:
            raise EncodeError(f"key {k!r}: this keyed model has keys 0..{self.n_keys - 1}")
        return k

    def _split(self, inv):
        try:
            k, i = inv
        except (TypeError, ValueError):
            raise EncodeError(f"not a (key, inv) invocation: {inv!r}") from None
        return self._key(k), i

    def _model(self, m):
        if not isinstance(m, tuple) or len(m) != self.n_keys:
            raise EncodeError(f"not a state of this keyed model ({self.n_keys} component states): {m!r}")
        return m

    # bound methods: linearisable() finds the model through their __self__
    def transition(self, m, ev):
        kind, x = ev
        m = self._model(m)
        if kind == "L":
            k, i = self._split(x)
            out = _Invoked(m[:k] + (self.component.transition(m[k], ("L", i)),) + m[k + 1:])
            out.key = k
            return out
        k = getattr(m, "key", None)
        if k is None:       # (no invocation before it: nothing to apply the response to)
            return tuple(m)
        return m[:k] + (self.component.transition(m[k], ("R", x)),) + m[k + 1:]

    def postcondition(self, m, inv, resp):
        k, i = self._split(inv)
        return self.component.postcondition(self._model(m)[k], i, resp)

    def encode_inv(self, inv, accounts):
        k, i = self._split(inv)
        return self.component.encode_inv(i, None)[0], k, 0, 0

    def encode_resp(self, resp):
        return self.component.encode_resp(resp)

    def decode_inv(self, code, a, b, val, accounts):
        return (a, self.component.invs[code])

    def decode_resp(self, code, val):
        return self.component.resps[code]

    def pack_model0(self, model0, accounts):
        """``n_keys`` uint32 component states (a ctypes array), None for init_model."""
        if model0 is None:
            return None
        return (ctypes.c_uint32 * self.n_keys)(*[self.component._state(s) for s in self._model(model0)])

    def split_history(self, history, pending=False):
        """The per-key sub-histories the local mode searches (knob
        "ktable_local", include/qsmd.h): ``None`` when ``history`` is not
        *splittable*, else ``[(key, sub_history), ...]`` in ascending key
        order, keys with no operation left out.  ``pending=True`` is the
        split of the keyed pending call's local mode (knob "kpending_local"):
        a pid's events may end on an invocation, which is pending and belongs
        to its own key; everything else is refused as below.

        Splittable: at most 128 events, every invocation a ``(key, inv)`` of
        this model and every response one of the component's, and every pid's
        events alternating invocation, response, ... from an invocation to a
        response (no pending invocation, no lone response, no two operations
        of one pid in flight).  An operation is an invocation and its pid's
        next event; sub-history ``k`` is the events, unchanged and in history
        order, of the operations invoked on key ``k``."""
        history = list(history)
        if len(history) > 128:
            return None
        open_key = {}                   # pid -> the key of its operation in flight
        parts = {}
        for pid, (kind, x) in history:
            try:
                if kind == "L":
                    k = self.encode_inv(x, None)[1]
                else:
                    self.encode_resp(x)
            except EncodeError:
                return None
            if kind == "L":
                if pid in open_key:
                    return None
                open_key[pid] = k
            else:
                if pid not in open_key:
                    return None
                k = open_key.pop(pid)
            parts.setdefault(k, []).append((pid, (kind, x)))
        if open_key and not pending:
            return None
        return sorted(parts.items())

    def show_model(self, model):
        return "{" + ", ".join(f"{k}: {self.component.show_model(s)}" for k, s in enumerate(model)) + "}"

    def show_inv(self, inv):
        k, i = self._split(inv)
        return f"[{k}] {self.component.show_inv(i)}"

    def show_resp(self, resp):
        return self.component.show_resp(resp)


TICKET = TicketDispenser()
BANK = Bank()

BY_ID = {MODEL_TICKET: TICKET, MODEL_BANK: BANK}
BY_NAME = {"ticket": TICKET, "bank": BANK}
