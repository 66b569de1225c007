"""Host half of the keyed table model (qsmd.models.KeyedTableModel,
QSMD_MODEL_KTABLE): its closures against the product closures of
tests/ktablegen.py, the oracle through both, the encoding, and the errors.
No GPU."""

import itertools
import random

import pytest

import ktablegen as kg
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd import KeyedTableModel, codec, models
from qsmd.linearisability import _device_model, replay_witness
from qsmd.models import EncodeError, TableModel, WideTableModel


def component(c):
    return TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                    raises=OracleModelError)


REG, LOCK = component(tg.REGISTER), component(tg.LOCK)


def step(transition, postcondition, s, inv, resp, raises):
    """(postcondition | 'raises', the state after the two transitions)."""
    try:
        ok = postcondition(s, inv, resp)
    except raises:
        ok = "raises"
    return ok, tuple(transition(transition(s, ("L", inv)), ("R", resp)))


def assert_same_step(m, p, s, inv, resp):
    a = step(m.transition, m.postcondition, s, inv, resp, models.ModelError)
    b = step(p["transition"], p["postcondition"], s, inv, resp, OracleModelError)
    assert a == b, (s, inv, resp, a, b)


def test_closures_equal_the_product_everywhere_on_two_registers():
    m, p = KeyedTableModel(REG, 2), kg.product(tg.REGISTER, 2)
    assert m.invs == p["invs"] and m.resps == p["resps"] and m.init_model == p["init"] and m.model_id == 5
    n = 0
    for s in itertools.product(tg.REG_VALUES, repeat=2):
        for inv in p["invs"]:
            for resp in p["resps"]:
                assert_same_step(m, p, s, inv, resp)
                n += 1
    assert n == 16 * 42 * 7


@pytest.mark.parametrize("name", ["register", "lock"])
def test_closures_equal_the_product_on_eight_keys(name):
    c, t = (tg.REGISTER, REG) if name == "register" else (tg.LOCK, LOCK)
    m, p = KeyedTableModel(t, 8), kg.product(c, 8)
    rng = random.Random(f"ktable-host/{name}")
    raised = 0
    for _ in range(1000):
        s = tuple(rng.choice(t.states) for _ in range(8))
        inv, resp = rng.choice(p["invs"]), rng.choice(p["resps"])
        assert_same_step(m, p, s, inv, resp)
        raised += step(m.transition, m.postcondition, s, inv, resp, models.ModelError)[0] == "raises"
    assert (raised > 0) == (name == "lock")


def test_the_oracle_through_the_bound_methods():
    m, p = KeyedTableModel(LOCK, 4), kg.product(tg.LOCK, 4)

    def post(s, inv, resp):
        try:
            return m.postcondition(s, inv, resp)
        except models.ModelError as e:
            raise OracleModelError(str(e)) from None

    hists = tg.gen_batch(p, "3x10", 200)
    seen = set()
    for h in hists:
        a = oracle_linearisable(m.transition, post, m.init_model, h, tg.MAX_NODES)
        b = oracle_linearisable(p["transition"], p["postcondition"], p["init"], h, tg.MAX_NODES)
        assert a == b
        seen.add(a[0])
        if a[0] == "lin":       # the oracle's path as a witness: invocation indices
            w, removed = [], set()
            for pid, inv, _ in a[2]:
                j = next(i for i, (q, e) in enumerate(h) if i not in removed and e == ("L", inv) and q == pid)
                r = next(i for i, (q, (k, _)) in enumerate(h) if i not in removed and k == "R" and q == pid)
                i0 = next(i for i, (q, (k, _)) in enumerate(h) if i not in removed and k == "L" and q == pid)
                w.append(j)
                removed |= {i0, r}
            assert replay_witness(m, h, w)
    assert {"lin", "nonlin", "error"} <= seen
    assert _device_model(m.transition, m.postcondition) is m
    with pytest.raises(NotImplementedError):
        _device_model(m.transition, KeyedTableModel(LOCK, 4).postcondition)


def test_encode_and_decode_round_trip():
    m = KeyedTableModel(REG, 8)
    p = kg.product(tg.REGISTER, 8)
    hists = tg.gen_batch(p, "4x16", 50)
    batch = codec.encode(m, hists)
    assert not batch.encode_errors and (batch.hdr["model_id"] == 5).all()
    for i, h in enumerate(hists):
        assert codec.decode_history(batch, i) == h
    ev = batch.events
    inv = (ev["kp"] & 0x80) == 0
    assert set(ev["a"][inv].tolist()) == set(range(8)) and (ev["a"][~inv] == 0).all()
    assert (ev["b"] == 0).all() and (ev["val"] == 0).all()
    assert m.encode_inv((7, ("Cas", 3, 3)), None) == (len(tg.REG_INVS) - 1, 7, 0, 0)
    assert m.decode_inv(20, 7, 0, 0, None) == (7, ("Cas", 3, 3))
    assert m.encode_resp("CasFail") == REG.encode_resp("CasFail")
    assert list(m.pack_model0((3, 0, 2, 1, 0, 0, 0, 1), {})) == [REG.state_index[v] for v in (3, 0, 2, 1, 0, 0, 0, 1)]
    assert m.pack_model0(None, {}) is None
    assert "3" in m.show_inv((3, "Read")) and m.show_resp("Ok") == REG.show_resp("Ok")
    assert m.show_model(m.init_model).count(":") == 8


def test_errors():
    m = KeyedTableModel(REG, 8)
    for bad in [(8, "Read"), (-1, "Read"), ("0", "Read"), "Read", (0, "Nope")]:
        with pytest.raises(EncodeError):
            m.encode_inv(bad, None)
    for n in (0, 9, True, 2.0):
        with pytest.raises(EncodeError):
            KeyedTableModel(REG, n)
    wide = WideTableModel.from_closures(tg.reg_transition, tg.reg_postcondition, 0, tg.REG_INVS, tg.REG_RESPS)
    with pytest.raises(EncodeError):
        KeyedTableModel(wide, 2)
    with pytest.raises(EncodeError):
        m.pack_model0((0,) * 7, {})
    with pytest.raises(EncodeError):
        m.pack_model0((0,) * 9, {})
    with pytest.raises(EncodeError):
        m.pack_model0((0, 0, 0, 4, 0, 0, 0, 0), {})
    # a history with a key out of range is an encode error of that history alone
    m4 = KeyedTableModel(REG, 4)
    good = [(0, ("L", (3, "Read"))), (0, ("R", ("Val", 0)))]
    bad = [(0, ("L", (4, "Read"))), (0, ("R", ("Val", 0)))]
    batch = codec.encode(m4, [good, bad, good])
    assert list(batch.encode_errors) == [1] and batch.hdr["model_id"].tolist() == [5, codec.BAD_MODEL, 5]


def test_the_setter_host_half_stand_alone(tmp_path):
    """tools/ktable_host_check.cpp: csrc/ktable_host.h (the validation, blob
    building and model0 packing of qsmd_ktable_set) built and run on its own,
    no device.  (Its header gives the sanitizer build.)"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "ktable_host_check")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I", os.path.join(root, "include"),
                    "-I", os.path.join(root, "quickcheck-state-machine-distributed_amd", "csrc"),
                    "-x", "hip", os.path.join(root, "tools", "ktable_host_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ktable host checks ok" in out.stdout, out.stdout[-2000:]
