"""Table-driven models on the host: qsmd.models.TableModel tabulates any
finite-state model's closures (include/qsmd.h QSMD_MODEL_TABLE); its
``transition`` / ``postcondition`` lookups must be the original closures as
far as the reference search can tell -- the same status, node count and path
from the literal oracle (oracle/linearise_lists.py) on generated histories."""

import ctypes
import os
import random
import re

import numpy as np
import pytest

import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, models
from qsmd.linearisability import _device_model, replay_witness, trace
from qsmd.models import EncodeError, TableModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ticket_model(K=16):
    t = tg.ticket_closures(K)

    def real(n, inv):                       # a dispenser that was reset before the history
        return (0, "Ok") if inv == "Reset" else (n + 1, ("Number", n + 1))
    t["real"] = real
    t["init_real"] = 0
    return t


def table_of(model):
    return TableModel.from_closures(model["transition"], model["postcondition"], model["init"],
                                    model["invs"], model["resps"], raises=OracleModelError)


MODELS = {"register": tg.REGISTER, "lock": tg.LOCK, "ticket": ticket_model()}


def histories(model, n):
    rng = random.Random(f"host/{model['name']}")
    out = []
    for k in range(n):
        c, ops, p = ((4, 16, 0.03), (3, 10, 0.1), (2, 10, 0.05))[k % 3]
        if model["name"].startswith("ticket"):
            m = dict(model, init=model["init_real"])
            ops = min(ops, 10)
            out.append(tg.gen_history(m, rng, c, ops, p))
        else:
            out.append(tg.gen_history(model, rng, c, ops, p))
    return out


@pytest.mark.parametrize("name", sorted(MODELS))
def test_tables_are_the_closures(name):
    """500 generated histories: the oracle with the table's lookups returns
    what it returns with the original closures (status, nodes, path)."""
    model = MODELS[name]
    m = table_of(model)

    def post(s, inv, resp):                 # the package's ModelError is the oracle's `raises`
        try:
            return m.postcondition(s, inv, resp)
        except models.ModelError as exc:
            raise OracleModelError(str(exc)) from None

    seen = set()
    for h in histories(model, 500):
        a = oracle_linearisable(model["transition"], model["postcondition"], model["init"], h, 2000)
        b = oracle_linearisable(m.transition, post, m.init_model, h, 2000)
        assert a == b
        seen.add(a[0])
    assert {"lin", "nonlin"} <= seen
    if name == "lock":
        assert "error" in seen and m.post_err is not None
    else:
        assert m.post_err is None


def test_shapes():
    reg = table_of(tg.REGISTER)
    assert (len(reg.states), len(reg.invs), len(reg.resps)) == (4, 21, 7)
    assert reg.states[0] == 0 and reg.init_model == 0 and sorted(reg.states) == [0, 1, 2, 3]
    assert reg.on_inv.dtype == np.uint8 and reg.on_inv.shape == (4, 21)
    assert reg.on_resp.dtype == np.uint8 and reg.on_resp.shape == (4, 7)
    assert reg.post.dtype == np.uint32 and reg.post.shape == (4, 21)
    # a response never moves the register
    assert all((reg.on_resp[s] == s).all() for s in range(4))
    t = table_of(tg.ticket_closures(10))
    assert len(t.states) == 13 and t.states[0] is None and tg.SINK in t.states   # Nothing, Just 0..10, sink
    assert t.model_id == 3 and models.MODEL_TABLE == 3
    assert set(models.BY_ID) == {1, 2} and set(models.BY_NAME) == {"ticket", "bank"}


def test_hand_written_table_equals_from_closures():
    """The lock by hand: states [False, True] (breadth-first from the initial
    state), invocations Lock / Unlock / IsLocked, responses Ok / Busy / Yes / No."""
    hand = TableModel(states=[False, True], invs=tg.LOCK_INVS, resps=tg.LOCK_RESPS,
                      on_inv=[[1, 0, 0], [1, 0, 1]], on_resp=[[0] * 4, [1] * 4],
                      post=[[0b0001, 0, 0b1000], [0b0010, 0b0001, 0b0100]],
                      post_err=[[0, 0b1111, 0], [0, 0, 0]], init_state=0)
    m = table_of(tg.LOCK)
    assert hand.states == m.states and hand.init_state == m.init_state
    for a in ("on_inv", "on_resp", "post", "post_err"):
        assert np.array_equal(getattr(hand, a), getattr(m, a)), a
    assert m.transition(False, ("L", "Lock")) is True and m.transition(True, ("R", "Ok")) is True
    assert m.postcondition(True, "Unlock", "Ok") and not m.postcondition(True, "Lock", "Ok")
    with pytest.raises(models.ModelError):
        m.postcondition(False, "Unlock", "Ok")


def test_encode_decode_round_trip():
    for model in MODELS.values():
        m = table_of(model)
        hs = histories(model, 40)
        batch = codec.encode(m, hs)
        assert not batch.encode_errors and (batch.hdr["model_id"] == 3).all()
        for i, h in enumerate(hs):
            assert codec.decode_history(batch, i) == h
        for k, x in enumerate(m.invs):
            assert m.encode_inv(x, None) == (k, 0, 0, 0) and m.decode_inv(k, 0, 0, 0, None) == x
        for k, x in enumerate(m.resps):
            assert m.encode_resp(x) == (k, 0) and m.decode_resp(k, 0) == x
        ev = batch.events
        assert (ev["a"] == 0).all() and (ev["b"] == 0).all() and (ev["val"] == 0).all()


def test_pack_model0_and_struct():
    m = table_of(tg.REGISTER)
    assert m.pack_model0(None, {}) is None
    p = m.pack_model0(2, {})
    assert isinstance(p, ctypes.c_uint32) and p.value == m.state_index[2]
    st = m.c_struct()
    assert (st.n_states, st.n_inv, st.n_resp, st.init_state) == (4, 21, 7, 0)
    assert st.post == m.post.ctypes.data and st.post_err is None
    assert ctypes.sizeof(st) == 16 + 4 * ctypes.sizeof(ctypes.c_void_p)
    with pytest.raises(EncodeError):
        m.pack_model0(7, {})


def test_encode_errors():
    m = table_of(tg.REGISTER)
    with pytest.raises(EncodeError):
        m.encode_inv(("Write", 9), None)
    with pytest.raises(EncodeError):
        m.encode_resp("Nope")
    with pytest.raises(EncodeError):
        m.transition(0, ("L", "Nope"))
    # in a batch: the history is marked, the others are encoded
    batch = codec.encode(m, [[(0, ("L", "Read")), (0, ("R", ("Val", 0)))], [(0, ("L", "Nope"))]])
    assert list(batch.encode_errors) == [1] and batch.hdr["model_id"][1] == codec.BAD_MODEL

    def counter(n):
        return (lambda s, ev: (s + 1) % n if ev[0] == "L" else s), (lambda s, i, r: True)

    tr, po = counter(256)
    assert len(TableModel.from_closures(tr, po, 0, ["inc"], ["ok"]).states) == 256
    tr, po = counter(257)
    with pytest.raises(EncodeError):
        TableModel.from_closures(tr, po, 0, ["inc"], ["ok"])
    tr, po = counter(2)
    assert len(TableModel.from_closures(tr, po, 0, list(range(32)), list(range(32))).invs) == 32
    with pytest.raises(EncodeError):
        TableModel.from_closures(tr, po, 0, list(range(33)), ["ok"])
    with pytest.raises(EncodeError):
        TableModel.from_closures(tr, po, 0, ["inc"], list(range(33)))
    with pytest.raises(EncodeError):            # explicit tables: an entry the kernel would index with
        TableModel([0, 1], ["i"], ["r"], [[2], [0]], [[0], [1]], [[1], [1]])
    with pytest.raises(EncodeError):
        TableModel([0, 1], ["i"], ["r"], [[1], [0]], [[0], [1]], [[1], [1]], init_state=2)


def test_linearisable_resolves_the_model():
    """`linearisable(m.transition, m.postcondition, ...)`: bound methods are
    new objects at every access, so the model is found through __self__."""
    m, other = table_of(tg.REGISTER), table_of(tg.LOCK)
    assert m.transition is not m.transition
    assert _device_model(m.transition, m.postcondition) is m
    assert _device_model(other.transition, other.postcondition) is other
    assert _device_model(models.TICKET.transition, models.TICKET.postcondition) is models.TICKET
    with pytest.raises(NotImplementedError):
        _device_model(m.transition, other.postcondition)
    with pytest.raises(NotImplementedError):
        _device_model(m.postcondition, m.transition)
    with pytest.raises(NotImplementedError):
        _device_model(tg.reg_transition, tg.reg_postcondition)


def test_trace_and_replay_witness():
    m = table_of(tg.REGISTER)
    h = [("a", ("L", ("Write", 2))), ("b", ("L", "Read")), ("a", ("R", "Ok")), ("b", ("R", ("Val", 2)))]
    assert replay_witness(m, h, [0, 1]) and not replay_witness(m, h, [1, 0])
    assert replay_witness(m, h[1:2] + h[3:], [0], model0=2) and not replay_witness(m, h[1:2] + h[3:], [0])
    text = trace(m.transition, 0, h)
    assert text == ("0\n  ==> ('Write', 2)  [a]\n2\n  ==> 'Read'  [b]\n"
                    "2\n  <== 'Ok'  [a]\n2\n  <== ('Val', 2)  [b]\n")


def test_header_is_additive():
    text = open(os.path.join(ROOT, "include", "qsmd.h")).read()
    assert re.search(r"#define\s+QSMD_ABI_VERSION\s+3u", text)
    for name, val in (("QSMD_MODEL_TABLE", "3u"), ("QSMD_TABLE_MAX_STATES", "256"),
                      ("QSMD_TABLE_MAX_INV", "32"), ("QSMD_TABLE_MAX_RESP", "32")):
        assert re.search(rf"#define\s+{name}\s+{val}\b", text), name
    assert "int qsmd_table_set(qsmd_ctx*" in text
