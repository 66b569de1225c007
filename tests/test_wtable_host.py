"""Wide table-driven models on the host: qsmd.models.WideTableModel
(include/qsmd.h QSMD_MODEL_WTABLE) -- up to 65,536 states and 256 symbols,
uint16 transitions, multi-word postcondition bitsets -- with TableModel's
methods and numbering."""

import ctypes
import os
import re

import numpy as np
import pytest

import tablegen as tg
import wtablegen as wg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec, models
from qsmd.linearisability import _device_model, replay_witness, trace
from qsmd.models import EncodeError, TableModel, WideTableModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counter(n):
    return (lambda s, ev: (s + 1) % n if ev[0] == "L" else s), (lambda s, i, r: True)


def test_kv_shapes():
    m = wg.wide_table("kv")
    assert isinstance(m, WideTableModel) and isinstance(m, TableModel)
    assert m.model_id == 4 and models.MODEL_WTABLE == 4 and models.MODEL_TABLE == 3
    assert (len(m.states), len(m.invs), len(m.resps)) == (1024, 105, 6)
    assert m.states[0] == wg.KV["init"] and m.init_state == 0 and m.init_model == (0,) * 5
    assert m.on_inv.dtype == np.uint16 and m.on_inv.shape == (1024, 105)
    assert m.on_resp.dtype == np.uint16 and m.on_resp.shape == (1024, 6)
    assert m.post.dtype == np.uint32 and m.post.shape == (1024, 105, 1) and m.post_err is None
    assert int(m.on_inv.max()) == 1023
    # the narrow model refuses it; the registries are the built-in models'
    with pytest.raises(EncodeError):
        TableModel.from_closures(wg.kv_transition, wg.kv_postcondition, wg.KV["init"], wg.KV_INVS, wg.KV_RESPS)
    assert set(models.BY_ID) == {1, 2} and set(models.BY_NAME) == {"ticket", "bank"}


def test_the_same_numbering_as_the_narrow_model():
    for c in (tg.REGISTER, tg.LOCK):
        n = TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                     raises=OracleModelError)
        w = wg.wide_table(c["name"])
        assert w.states == n.states and w.invs == n.invs and w.resps == n.resps
        assert np.array_equal(w.on_inv, n.on_inv) and np.array_equal(w.on_resp, n.on_resp)
        assert np.array_equal(w.post[:, :, 0], n.post)
        assert (w.post_err is None) == (n.post_err is None)
        if n.post_err is not None:
            assert np.array_equal(w.post_err[:, :, 0], n.post_err)


@pytest.mark.parametrize("name", ["wcounter", "big", "reg512"])
def test_numpy_tables_are_the_closures(name):
    m = wg.wide_table(name)
    assert wg.sampled_entries_equal_closures(name, 1000) == 1000
    if name == "wcounter":
        assert m.post.shape == (300, 256, 8) and m.post_err.shape == (300, 256, 8)
        assert m.postcondition(10, 50, 60) and not m.postcondition(10, 50, 61)      # word 1
        assert m.postcondition(200, 55, 255) and not m.postcondition(200, 55, 31)   # word 7
        with pytest.raises(models.ModelError):
            m.postcondition(127, 0, 200)
        assert m.transition(299, ("L", 1)) == 0
    if name == "big":
        assert len(m.states) == 65536 and m.post.shape == (65536, 2, 1)
        assert m.transition(65535, ("L", 1)) == 0 and int(m.on_inv.max()) == 65535


def test_tables_are_the_closures_for_the_oracle():
    """Generated histories: the oracle with the table's lookups returns what
    it returns with the closures (status, nodes, path)."""
    for name in ("kv", "wcounter"):
        c, m = wg.BY_NAME[name], wg.wide_table(name)

        def post(s, inv, resp):
            try:
                return m.postcondition(s, inv, resp)
            except models.ModelError as exc:
                raise OracleModelError(str(exc)) from None

        for h in tg.gen_batch(c, "3x10", 60, seed=5):
            assert (oracle_linearisable(c["transition"], c["postcondition"], c["init"], h, 2000) ==
                    oracle_linearisable(m.transition, post, m.init_model, h, 2000))


def test_limits():
    tr, po = counter(65536)
    m = WideTableModel.from_closures(tr, po, 0, ["inc"], ["ok"])
    assert len(m.states) == 65536 and m.on_inv[65535, 0] == 0
    tr, po = counter(65537)
    with pytest.raises(EncodeError):
        WideTableModel.from_closures(tr, po, 0, ["inc"], ["ok"])
    tr, po = counter(2)
    m = WideTableModel.from_closures(tr, po, 0, list(range(256)), list(range(256)))
    assert len(m.invs) == 256 and m.post.shape == (2, 256, 8) and (m.post == 0xFFFFFFFF).all()
    with pytest.raises(EncodeError):
        WideTableModel.from_closures(tr, po, 0, list(range(257)), ["ok"])
    with pytest.raises(EncodeError):
        WideTableModel.from_closures(tr, po, 0, ["inc"], list(range(257)))
    # explicit tables
    with pytest.raises(EncodeError):
        WideTableModel(list(range(65537)), ["i"], ["r"], np.zeros((65537, 1), int), np.zeros((65537, 1), int),
                       np.zeros((65537, 1, 1), int))
    with pytest.raises(EncodeError):            # an entry the kernel would index with
        WideTableModel([0, 1], ["i"], ["r"], [[2], [0]], [[0], [1]], [[[1]], [[1]]])
    with pytest.raises(EncodeError):
        WideTableModel([0, 1], ["i"], ["r"], [[1], [0]], [[0], [2]], [[[1]], [[1]]])
    with pytest.raises(EncodeError):
        WideTableModel([0, 1], ["i"], ["r"], [[1], [0]], [[0], [1]], [[[1]], [[1]]], init_state=2)
    with pytest.raises(EncodeError):            # post: (ns, ni, post_words), not the narrow (ns, ni)
        WideTableModel([0, 1], ["i"], ["r"], [[1], [0]], [[0], [1]], [[1], [1]])
    assert WideTableModel([0, 1], ["i"], ["r"], [[1], [0]], [[0], [1]], [[[1]], [[1]]], init_state=1).init_model == 1


def test_encode_decode_round_trip():
    for name in ("kv", "wcounter"):
        c, m = wg.BY_NAME[name], wg.wide_table(name)
        hs = tg.gen_batch(c, "4x16", 40, seed=2)
        batch = codec.encode(m, hs)
        assert not batch.encode_errors and (batch.hdr["model_id"] == 4).all()
        for i, h in enumerate(hs):
            assert codec.decode_history(batch, i) == h
        for k, x in enumerate(m.invs):
            assert m.encode_inv(x, None) == (k, 0, 0, 0) and m.decode_inv(k, 0, 0, 0, None) == x
        for k, x in enumerate(m.resps):
            assert m.encode_resp(x) == (k, 0) and m.decode_resp(k, 0) == x
        assert int(batch.events["code"].max()) > 31
    m = wg.wide_table("kv")
    with pytest.raises(EncodeError):
        m.encode_inv(("Write", 9, 0), None)
    batch = codec.encode(m, [[(0, ("L", ("Read", 0))), (0, ("R", ("Val", 0)))], [(0, ("L", "Nope"))]])
    assert list(batch.encode_errors) == [1] and batch.hdr["model_id"][1] == codec.BAD_MODEL


def test_pack_model0_and_struct():
    m = wg.wide_table("kv")
    assert m.pack_model0(None, {}) is None
    far = (3, 3, 3, 3, 3)
    p = m.pack_model0(far, {})
    assert isinstance(p, ctypes.c_uint32) and p.value == m.state_index[far] > 255
    with pytest.raises(EncodeError):
        m.pack_model0((4, 0, 0, 0, 0), {})
    st = m.c_struct()
    assert (st.n_states, st.n_inv, st.n_resp, st.init_state) == (1024, 105, 6, 0)
    assert st.on_inv == m.on_inv.ctypes.data and st.on_resp == m.on_resp.ctypes.data
    assert st.post == m.post.ctypes.data and st.post_err is None
    assert ctypes.sizeof(st) == 16 + 4 * ctypes.sizeof(ctypes.c_void_p)
    w = wg.wide_table("wcounter")
    assert w.c_struct().post_err == w.post_err.ctypes.data
    assert w.on_inv.flags["C_CONTIGUOUS"] and w.post.flags["C_CONTIGUOUS"]


def test_linearisable_resolves_wide_and_narrow_models_apart():
    c = tg.REGISTER
    narrow = TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"])
    wide, kv = wg.wide_table("register"), wg.wide_table("kv")
    for m in (narrow, wide, kv):
        assert _device_model(m.transition, m.postcondition) is m
    assert _device_model(wide.transition, wide.postcondition).model_id == 4
    assert _device_model(narrow.transition, narrow.postcondition).model_id == 3
    with pytest.raises(NotImplementedError):
        _device_model(wide.transition, narrow.postcondition)
    with pytest.raises(NotImplementedError):
        _device_model(kv.transition, wide.postcondition)
    with pytest.raises(NotImplementedError):
        _device_model(wg.kv_transition, wg.kv_postcondition)


def test_trace_and_replay_witness():
    m = wg.wide_table("kv")
    w, r = ("Write", 4, 2), ("Read", 4)
    h = [("a", ("L", w)), ("b", ("L", r)), ("a", ("R", "Ok")), ("b", ("R", ("Val", 2)))]
    assert replay_witness(m, h, [0, 1]) and not replay_witness(m, h, [1, 0])
    two = (0, 0, 0, 0, 2)
    assert replay_witness(m, h[1:2] + h[3:], [0], model0=two) and not replay_witness(m, h[1:2] + h[3:], [0])
    text = trace(m.transition, m.init_model, h)
    assert text == (f"{(0,) * 5!r}\n  ==> {w!r}  [a]\n{two!r}\n  ==> {r!r}  [b]\n"
                    f"{two!r}\n  <== 'Ok'  [a]\n{two!r}\n  <== ('Val', 2)  [b]\n")


def test_header_is_additive():
    text = open(os.path.join(ROOT, "include", "qsmd.h")).read()
    assert re.search(r"#define\s+QSMD_ABI_VERSION\s+3u", text)
    for name, val in (("QSMD_MODEL_WTABLE", "4u"), ("QSMD_WTABLE_MAX_STATES", "65536"),
                      ("QSMD_WTABLE_MAX_INV", "256"), ("QSMD_WTABLE_MAX_RESP", "256"),
                      ("QSMD_WTABLE_MAX_BYTES", r"\(64u << 20\)")):
        assert re.search(rf"#define\s+{name}\s+{val}(?!\w)", text), name
    assert "int qsmd_wtable_set(qsmd_ctx*" in text and "} qsmd_wtable_model;" in text
    assert re.search(r"const uint16_t\*\s+on_inv;", text) and re.search(r"const uint16_t\*\s+on_resp;", text)
