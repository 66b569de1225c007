"""The any-shape histories (tests/anyshape.py: ill-formed, shared pids, pending
invocations, stray and leading responses) against the CPU references alone:
the conditions the generator must meet for the GPU tests
(tests/test_gpu_table_anyshape.py) to mean anything, the agreement of every
CPU reference on every one of these histories, the Haskell binding's witness
check on their paths, and their encoding."""

import functools

import numpy as np
import pytest

import anyshape as an
import ktablememo as km
import tablegen as tg
import tablememo as tm
import wtablegen as wg
from hs_replay import hs_replay, successful_paths
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec
from qsmd.models import KeyedTableModel

MAXN = tg.MAX_NODES
MODELS = {"register": tg.REGISTER, "lock": tg.LOCK, "kv": wg.KV, "register^4": km.product("register", 4),
          "lock^8": km.product("lock", 8)}
KEYED = {"register^4": ("register", 4), "lock^8": ("lock", 8)}
STATUSES = {name: {"lin", "nonlin", "budget"} | ({"error"} if name.startswith("lock") else set())
            for name in MODELS}
SETTINGS = list(an.ALL_SETTINGS)


@functools.lru_cache(maxsize=None)
def case(name, setting):
    """The histories of one setting and the literal oracle's results
    (computed once, shared)."""
    m = MODELS[name]
    hists = an.batch(m, setting)
    return hists, [oracle_linearisable(m["transition"], m["postcondition"], m["init"], h, MAXN) for h in hists]


# ------------------------------------------------------- 1. census conditions

def test_the_generator_is_deterministic_and_within_the_encoding():
    for name in ("register", "lock^8"):
        for setting in SETTINGS:
            hists = an.batch(MODELS[name], setting, 50)
            assert hists == an.batch(MODELS[name], setting, 50)
            assert hists != an.batch(MODELS[name], setting, 50, seed="another")
            assert all(len(h) <= an.MAX_EVENTS for h in hists)
    assert max(len(h) for h in case("register", "2x62")[0]) > 64
    assert {len(h) for h in case("register", an.RANDOM)[0]} == set(range(17))


def test_exactly_and_census():
    L, R = tg.L, tg.R
    h = [(0, L("Read")), (1, L("Read")), (0, R(("Val", 0))), (1, R(("Val", 0)))]
    assert an.census(h) == set()
    assert an.exactly(h, 3) == h[:3] and an.census(an.exactly(h, 3)) == {"pending"}
    assert an.exactly(h, 6) == h + h[:2] and an.census(an.exactly(h, 6)) == {"pending"}
    assert an.exactly(h, 10) == h + h + h[:2]
    assert an.census([(0, L("Read")), (0, L("Read")), (0, R(("Val", 0)))]) == {"two_in_flight", "pending"}
    assert an.census([(0, R("Ok")), (0, L("Read"))]) == {"stray_resp", "resp_first", "pending"}
    assert an.census([(0, L("Read")), (0, R("Ok")), (0, R("Ok"))]) == {"stray_resp"}
    assert an.census([]) == set()
    with pytest.raises(ValueError):
        an.exactly([], 1)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_census_conditions(name):
    """Conditions on the generator, from the oracle alone.  More than pass
    1's default budget (256 nodes) is counted by at least 1 history in 10 of
    every bent setting, and of all the model's histories, the random family
    (at most 16 events: never over 256 nodes) included."""
    seen = set()
    long_runs = total = 0
    for setting in SETTINGS:
        hists, ref = case(name, setting)
        seen |= {r[0] for r in ref}
        over = sum(r[1] > 256 for r in ref)
        long_runs += over
        total += len(ref)
        if setting == an.RANDOM:
            continue
        cen = [an.census(h) for h in hists]
        for feature in an.FEATURES:
            assert 20 * sum(feature in c for c in cen) >= len(hists), (setting, feature)
        assert 2 * sum(r[0] != "budget" for r in ref) >= len(hists), setting
        assert 10 * over >= len(hists), (setting, over)
    assert seen == STATUSES[name]
    assert 10 * long_runs >= total, (long_runs, total)


# ---------------------------------------------- 2. the CPU references agree

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", ["register", "lock", "register^4", "lock^8"])
def test_cpu_references_agree(name, setting):
    m = MODELS[name]
    hists, ref = case(name, setting)
    for h, want in zip(hists, ref):
        assert tm.exact_count(m, h, MAXN) == want[:2], h
        for entries in (0, 2, 64):
            if name in KEYED:
                got = km.kmemo_dfs(*KEYED[name], h, entries, MAXN)
            else:
                got = tm.memo_dfs(m, h, entries, MAXN)
            assert got == want, (h, entries)


# ------------------------------------------------------ 3. the witness check

def path_to_witness(hist, path):
    """The invocation events a path of the oracle chose: at each step the
    first remaining invocation of takeInvocations' prefix with the step's pid
    and symbol (a later equal one has the same child)."""
    rest, out = list(range(len(hist))), []
    for pid, inv, _ in path:
        j = None
        for k in rest:
            if hist[k][1][0] != "L":
                break
            if hist[k] == (pid, ("L", inv)):
                j = k
                break
        assert j is not None
        out.append(j)
        rest.remove(next(k for k in rest if hist[k][0] == pid and hist[k][1][0] == "L"))     # filter1
        rest.remove(next(k for k in rest if hist[k][0] == pid and hist[k][1][0] == "R"))     # findResponse
    return out


def witness_to_path(hist, wit):
    """The operations a witness names: each chosen invocation with the first
    remaining response of its pid; the pid's first remaining invocation and
    that response leave (Lemma L1)."""
    removed, path = set(), []
    for j in wit:
        pid, (_, inv) = hist[j]
        r = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "R" and p == pid)
        i0 = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "L" and p == pid)
        path.append((pid, inv, hist[r][1][1]))
        removed |= {i0, r}
    return path


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_hs_replay_accepts_every_path(name, setting):
    m = MODELS[name]
    tr, post, init = m["transition"], m["postcondition"], m["init"]
    hists, ref = case(name, setting)
    n_lin = n_nonlin = 0
    for h, (st, _, path) in zip(hists, ref):
        if st == "lin":
            wit = path_to_witness(h, path)
            assert witness_to_path(h, wit) == path, h
            assert hs_replay(tr, post, init, h, wit), h
            n_lin += 1
        elif st == "nonlin" and n_nonlin < 50:
            assert successful_paths(tr, post, init, h) == [], h
            n_nonlin += 1
    assert n_lin > 0 and n_nonlin > 0


# -------------------------------------------------------------- 4. encoding

def device_models():
    return {"register": tm._table("register"), "lock": tm._table("lock"), "kv": wg.wide_table("kv"),
            "lock/wide": wg.wide_table("lock"), "register^4": KeyedTableModel(tm._table("register"), 4),
            "lock^8": KeyedTableModel(tm._table("lock"), 8)}


@pytest.mark.parametrize("name", ["register", "lock", "kv", "lock/wide", "register^4", "lock^8"])
def test_encoding(name):
    dm = device_models()[name]
    for setting in SETTINGS:
        hists = case(name.split("/")[0], setting)[0]
        batch = codec.encode(dm, hists)
        assert not batch.encode_errors
        assert [int(n) for n in batch.hdr["n_ev"]] == [len(h) for h in hists]
        assert (batch.hdr["model_id"] == dm.model_id).all()
        for i, h in enumerate(hists):
            first_use = list(dict.fromkeys(p for p, _ in h))
            assert batch.pid_maps[i] == {p: k for k, p in enumerate(first_use)}
            assert int(batch.hdr["n_pid"][i]) == len(first_use)
            o = int(batch.hdr["ev_off"][i])
            kp = batch.events["kp"][o:o + len(h)]
            assert np.array_equal(kp & 0x7F, [first_use.index(p) for p, _ in h])
            assert np.array_equal(kp >> 7, [e[0] == "R" for _, e in h])
            if setting == "6x14" and i < 50:
                assert codec.decode_history(batch, i) == h
