"""CPU tests of the explain feature's host side: the restatement of its rule
(tests/explain_ref.py) against the literal oracle, `explanation_from_path`
(qsmd/linearisability.py) on hand-made and generated cases, and the header."""

import functools
import os
import re

import pytest

import explain_ref as xr
import ktablegen as kg
import tablegen as tg
from linearise_lists import ModelError as OracleModelError
from linearise_lists import linearisable as oracle_linearisable
from qsmd.linearisability import Explanation, explanation_from_path
from qsmd.models import KeyedTableModel, TableModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXN = tg.MAX_NODES
L, R = tg.L, tg.R
CLOSURES = {"register": tg.REGISTER, "lock": tg.LOCK}
# (shape, histories): tablegen's settings and explain_ref's shapes
CASES = [("tg/3x10", 200), ("tg/4x16", 200), ("tg/6x24", 100), ("3x24", 64), ("2x40", 32), ("3x40", 16),
         (xr.ANYSHAPE, 128)]


@functools.lru_cache(maxsize=None)
def table(name):
    c = CLOSURES[name]
    return TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                    raises=OracleModelError)


@functools.lru_cache(maxsize=None)
def case(name, shape, n):
    c = CLOSURES[name]
    hists = tg.gen_batch(c, shape[3:], n) if shape.startswith("tg/") else xr.histories(c, shape)
    assert len(hists) == n
    return hists, xr.explain_all(c, hists, MAXN)


@pytest.mark.parametrize("shape,n", CASES)
@pytest.mark.parametrize("name", sorted(CLOSURES))
def test_restatement_equals_the_literal_oracle(name, shape, n):
    """Status and nodes of every history, and the path of every `lin` one."""
    c = CLOSURES[name]
    hists, ref = case(name, shape, n)
    for h, (st, nd, path, _) in zip(hists, ref):
        st_o, nd_o, path_o = oracle_linearisable(c["transition"], c["postcondition"], c["init"], list(h), MAXN)
        assert (st, nd) == (st_o, nd_o)
        if st == "lin":
            assert path == path_o
        if st == "budget":
            assert nd == MAXN


def test_every_status_and_depth_0_failures_occur():
    seen, depth0 = set(), 0
    for name in CLOSURES:
        for shape, n in CASES:
            for st, _, path, _ in case(name, shape, n)[1]:
                seen.add(st)
                depth0 += st == "nonlin" and not path
    assert seen == {"lin", "nonlin", "error", "budget"} and depth0 > 0


def path_indices(hist, ops):
    """The invocation event indices a path of operations stands for: at each
    level the first remaining candidate invocation equal to the operation's
    (the search takes candidates in history order, and equal candidates of
    one pid are one and the same child)."""
    removed, out = set(), []
    for pid, inv, resp in ops:
        j = next(i for i, (p, (k, x)) in enumerate(hist) if i not in removed and k == "L" and p == pid and x == inv)
        r = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "R" and p == pid)
        assert hist[r][1][1] == resp
        i0 = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "L" and p == pid)
        out.append(j)
        removed |= {i0, r}
    return out


@pytest.mark.parametrize("shape,n", CASES)
@pytest.mark.parametrize("name", sorted(CLOSURES))
def test_explanations_of_the_restatement(name, shape, n):
    """Every path replays to the restatement's operations and model with every
    postcondition true; at the end of a `nonlin` path no candidate passes, of a
    `lin` path none has a response, and an `error` path has a raising one."""
    c, m = CLOSURES[name], table(name)
    hists, ref = case(name, shape, n)
    for h, (st, _, path, model) in zip(hists, ref):
        e = explanation_from_path(m, h, path_indices(h, path), st)
        assert e.prefix == path and e.model == model and e.status == st
        cur = c["init"]
        for pid, inv, resp in e.prefix:
            assert c["postcondition"](cur, inv, resp)
            cur = c["transition"](c["transition"](cur, L(inv)), R(resp))
        assert cur == model
        outcomes = [s[3] for s in e.stuck]
        if st == "nonlin":
            assert "passes" not in outcomes and "raises" not in outcomes
        elif st == "lin":
            assert set(outcomes) <= {"no response"}
        elif st == "error":
            assert "raises" in outcomes
        assert e.pretty().count("=/=>") == len(e.stuck)


# --------------------------------------------------------------- hand-made cases

def test_register_read_of_a_value_nobody_wrote():
    h = [(0, L(("Write", 1))), (0, R("Ok")), (1, L("Read")), (1, R(("Val", 2)))]
    assert xr.explain(tg.reg_transition, tg.reg_postcondition, 0, h)[:3] == ("nonlin", 2, [(0, ("Write", 1), "Ok")])
    e = explanation_from_path(table("register"), h, [0], "nonlin")
    assert isinstance(e, Explanation)
    assert e.prefix == [(0, ("Write", 1), "Ok")]
    assert e.model == 1
    assert e.stuck == [(1, "Read", ("Val", 2), "postcondition false")]
    text = e.pretty()
    assert text.splitlines()[-1].endswith("[1]: postcondition false") and "==> " in text and "<== " in text


def test_pending_invocation_reads_no_response():
    h = [(0, L(("Write", 1))), (0, R("Ok")), (2, L("Read")), (1, L("Read")), (1, R(("Val", 2)))]
    e = explanation_from_path(table("register"), h, [0], 0)
    assert e.status == "nonlin" and e.model == 1
    assert e.stuck == [(2, "Read", None, "no response"), (1, "Read", ("Val", 2), "postcondition false")]
    assert "no response" in e.pretty()


def test_lock_unlock_of_an_unlocked_lock_raises():
    h = [(0, L("Lock")), (0, R("Ok")), (0, L("Unlock")), (0, R("Ok")), (1, L("Unlock")), (1, R("Ok"))]
    st, nodes, path, model = xr.explain(tg.lock_transition, tg.lock_postcondition, False, h)
    assert (st, path, model) == ("error", [(0, "Lock", "Ok"), (0, "Unlock", "Ok")], False)
    e = explanation_from_path(table("lock"), h, [0, 2], "error")
    assert e.prefix == path and e.model is False
    assert e.stuck == [(1, "Unlock", "Ok", "raises")]


def test_shared_pid_path_follows_the_witness_replay_rule():
    """Two operations of pid 0 in flight: choosing the second invocation pairs
    it with the pid's first response and removes the pid's first invocation."""
    h = [(0, L(("Write", 1))), (0, L(("Write", 2))), (0, R("Ok")), (0, R("Ok")), (1, L("Read")), (1, R(("Val", 3)))]
    e = explanation_from_path(table("register"), h, [1], "budget")
    assert e.prefix == [(0, ("Write", 2), "Ok")] and e.model == 2
    # what remains: Write 2 (event 1), Ok (event 3) and, beyond that response, the Read
    assert e.stuck == [(0, ("Write", 2), "Ok", "passes")]


def test_keyed_model_and_bad_paths():
    m = KeyedTableModel(table("register"), 2)
    h = [(0, L((1, ("Write", 3)))), (0, R("Ok")), (1, L((0, "Read"))), (1, R(("Val", 3)))]
    p = kg.product(tg.REGISTER, 2)
    st, _, path, model = xr.explain(p["transition"], p["postcondition"], p["init"], h)
    assert (st, path, tuple(model)) == ("nonlin", [(0, (1, ("Write", 3)), "Ok")], (0, 3))
    e = explanation_from_path(m, h, [0], st)
    assert tuple(e.model) == (0, 3) and e.stuck == [(1, (0, "Read"), ("Val", 3), "postcondition false")]
    assert "[0] " in e.pretty()
    for bad in ([1], [0, 0], [7], [2, 2]):
        with pytest.raises(ValueError):
            explanation_from_path(m, h, bad, "nonlin")
    assert explanation_from_path(m, [], [], "lin").prefix == []


# ------------------------------------------------------------------- the header

def test_header_declares_the_explain_entry_points():
    hdr = open(os.path.join(ROOT, "include", "qsmd.h")).read()
    assert re.search(r"^#define QSMD_ABI_VERSION 3u$", hdr, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("qsmd_explain_batch", "qsmd_explain_batch_device"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
    body = re.search(r"typedef struct qsmd_explain \{(.*?)\} qsmd_explain;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("uint16_t", "depth"), ("uint16_t", "reserved"),
                                                  ("uint32_t", "reserved2"), ("uint64_t", "state")]
    from qsmd import device
    assert device.EXPLAIN_DTYPE.itemsize == 16 and device.EXPLAIN_DTYPE.fields["state"][1] == 8
