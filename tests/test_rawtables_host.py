"""The raw-table inputs (tests/rawtables.py) on the host.

1. The inputs have teeth: conditions on the *reference alone*
   (oracle/linearise_lists.py, tests/pending_ref.py run with rawtables'
   closures), asserted for every shape before anything is sent to a GPU --
   every status is reached, the deep shapes pass pass 1's budget, and
   replacing ``on_resp`` by identity rows changes (status, nodes) on at least
   half of the histories: these inputs see the fourth table.
2. The Python mirror (qsmd.models.TableModel / WideTableModel /
   KeyedTableModel, replay_witness, split_history) against the raw arrays."""

import random

import numpy as np
import pytest

import ktablelocal_ref as kref
import pending_ref as pr
import rawtables as rt
from linearise_lists import linearisable as oracle_linearisable
from qsmd import codec
from qsmd.linearisability import replay_witness
from qsmd.models import EncodeError, KeyedTableModel, ModelError, TableModel, WideTableModel

SINGLE = [n for n in list(rt.NARROW) + list(rt.WIDE) if n != "c_odd"]
SHAPES = SINGLE + list(rt.KEYED)                    # every shape with check batches of its own
PENDING = [n for n in SHAPES if n not in rt.WIDE]   # the shapes with a pending entry


def has_err(name):
    return rt.spec(rt.KEYED[name][0] if name in rt.KEYED else name).p_err is not None


def union(name):
    """The reference's results over the union of a shape's check batches."""
    return [r for s in rt.BATCHES for r in rt.check_case(name, s)[1]]


# ------------------------------------------------------------ 1. the inputs have teeth

def test_the_tables_are_what_the_issue_describes():
    for name in SINGLE:
        sp, t = rt.spec(name), rt.tables_of(name)
        assert t.on_inv.shape == (sp.ns, sp.ni) and t.on_resp.shape == (sp.ns, sp.nr)
        assert 0 <= t.on_inv.min() and t.on_inv.max() < sp.ns and 0 <= t.on_resp.min() and t.on_resp.max() < sp.ns
        if sp.ns > 1:                                   # no identity fourth table
            assert (t.on_resp != np.arange(sp.ns)[:, None]).mean() > 0.4
        pw = (sp.nr + 31) // 32
        assert t.wide_post.shape == t.wide_err.shape == (sp.ns, sp.ni, pw)
        assert (t.post_words is None) == (sp.nr > 32)
        low = (1 << (sp.nr - 32 * (pw - 1))) - 1        # the last word's bits below n_resp
        for words, cube, high in ((t.wide_post, t.post, sp.high == "post"), (t.wide_err, t.err, sp.high == "err")):
            above = words[:, :, -1] & np.uint32(~low & 0xFFFFFFFF)
            assert (above == np.uint32(~low & 0xFFFFFFFF)).all() if high else not above.any()
            for r in {0, sp.nr - 1, min(31, sp.nr - 1), min(32, sp.nr - 1)}:
                assert np.array_equal((words[:, :, r >> 5] >> np.uint32(r & 31)) & 1, cube[:, :, r])
        if sp.nr <= 32:
            assert np.array_equal(t.post_words, t.wide_post[:, :, 0])
    # several allowed responses per (state, invocation), post_err overlapping post
    t = rt.tables_of("n_max")
    assert ((t.post & ~t.err).sum(axis=2) > 1).mean() > 0.9 and (t.post & t.err).any()


@pytest.mark.parametrize("name", SHAPES)
def test_every_status_is_reached(name):
    ref = union(name)
    n = len(ref)
    assert n == sum(rt.BATCHES.values())
    count = lambda st: sum(1 for r in ref if r[0] == st)        # noqa: E731
    if name == "n_one":
        assert count("lin") == n
        return
    assert 10 * count("lin") >= n and 10 * count("nonlin") >= n
    if has_err(name):
        assert count("error") >= 3
    else:
        assert count("error") == 0
    if name in rt.DEEP:
        assert count("budget") >= 1 and sum(1 for r in ref if r[1] > 256) >= 10
        assert all(r[1] == rt.MAX_NODES for r in ref if r[0] == "budget")


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "n_one"])
def test_the_fourth_table_decides(name):
    """With on_resp replaced by identity rows the reference's (status, nodes)
    changes on at least half of the histories; ignoring post_err changes at
    least one where there is one."""
    ref = union(name)
    ident = [r for s in rt.BATCHES for r in rt.variant_ref(name, s, "identity_resp")]
    changed = sum(1 for a, b in zip(ref, ident) if a[:2] != b[:2])
    assert 2 * changed >= len(ref), (changed, len(ref))
    if has_err(name):
        plain = [r for s in rt.BATCHES for r in rt.variant_ref(name, s, "ignore_err")]
        assert any(a[:2] != b[:2] for a, b in zip(ref, plain))


def next_state(name, s, inv, r):
    """The component state after (inv, r) from s, on the raw arrays."""
    t = rt.tables_of(rt.KEYED[name][0] if name in rt.KEYED else name)
    if name in rt.KEYED:
        k, i = inv
        return k, int(t.on_resp[t.on_inv[s[k], i], r])
    return int(t.on_resp[t.on_inv[s, inv], r])


@pytest.mark.parametrize("name", PENDING)
def test_crashed_batches_assume_responses(name):
    symbols, nexts = set(), set()
    for setting in rt.BATCHES:
        hists, ref = rt.crash_case(name, setting)
        assert sum(1 for h in hists if pr.pending_invocations(h)) > len(hists) // 3
        with_assumed = [r for r in ref if r[0] == "lin" and any(op[3] for op in r[2])]
        assert len(with_assumed) >= 10, (setting, len(with_assumed))
        c = rt.closures(name)
        for _, _, path in with_assumed:
            s = c["init"]
            for pid, inv, r, assumed in path:
                if assumed:
                    symbols.add(r)
                    nexts.add(next_state(name, s, inv, r))
                s = c["transition"](c["transition"](s, ("L", inv)), ("R", r))
    if name != "n_one":
        assert len(symbols) >= 2 and len(nexts) >= 2


@pytest.mark.parametrize("name", ["n_r32", "w_3w", "k_odd"])
def test_anyshape_census(name):
    import anyshape as an
    feats = set()
    for setting in rt.ANY_SETTINGS:
        feats |= set().union(*(an.census(h) for h in rt.anyshape_case(name, setting)[0]))
    assert feats == set(an.FEATURES)


@pytest.mark.parametrize("name", ["n_1inv", "n_r2"])
def test_pending_walks_have_several_allowed_symbols_and_high_bits(name):
    m, sp = rt.model(name), rt.spec(name)
    assert sp.high == "post"
    h, states = rt.pending_walk(name, 128)
    assert rt.pending_walk(name, 40)[0] == h[:40]
    s = sp.init
    for d, (_, (_, i)) in enumerate(h):
        assert s == states[d]
        word = int(m.post[s, i])
        assert word >> sp.nr == (1 << (32 - sp.nr)) - 1                 # the allowed word carries the high bits
        a = word & ~int(m.post_err[s, i]) & ((1 << sp.nr) - 1)
        assert a == rt.allowed_bits(name, s, i) and bin(a).count("1") >= 2
        s = int(m.on_resp[m.on_inv[s, i], (a & -a).bit_length() - 1])


# ------------------------------------------------- 2. the Python mirror on the raw arrays

def samples(name):
    """(s, i, r) triples: random ones, the corners (state ns-1, bit 31, the
    last bit of a wide word, the last response), and entries with both the
    post and the err bit set."""
    sp, t = rt.spec(name), rt.tables_of(name)
    rng = random.Random(f"rawtables/samples/{name}")
    out = {(rng.randrange(sp.ns), rng.randrange(sp.ni), rng.randrange(sp.nr)) for _ in range(300)}
    for r in {0, sp.nr - 1, min(31, sp.nr - 1), min(32, sp.nr - 1), min(63, sp.nr - 1), 32 * ((sp.nr - 1) // 32)}:
        out |= {(sp.ns - 1, sp.ni - 1, r), (0, 0, r), (sp.ns - 1, rng.randrange(sp.ni), r)}
    both = np.argwhere(t.post & t.err)
    out |= {tuple(int(x) for x in b) for b in both[:50]}
    return sorted(out), len(both)


@pytest.mark.parametrize("name", SINGLE + list(rt.TWINS))
def test_table_models_read_the_raw_arrays(name):
    m, sp, t = rt.model(name), rt.spec(name), rt.tables_of(name)
    assert type(m) is (WideTableModel if name in rt.WIDE or name in rt.TWINS else TableModel)
    assert (m.post_err is None) == (sp.p_err is None) and m.init_model == sp.init
    triples, n_both = samples(name)
    if name in ("n_max", "n_r32", "w_3w", "n_r2"):
        assert n_both > 0
    for s, i, r in triples:
        assert m.transition(s, ("L", i)) == int(t.on_inv[s, i])
        assert m.transition(s, ("R", r)) == int(t.on_resp[s, r])
        if t.err[s, i, r]:                          # ModelError wins over a post bit
            with pytest.raises(ModelError):
                m.postcondition(s, i, r)
        else:
            assert m.postcondition(s, i, r) is bool(t.post[s, i, r])
    # a response code at or above n_resp stays an EncodeError, whatever the high bits say
    for bad in (sp.nr, sp.nr + 31, -1):
        with pytest.raises(EncodeError):
            m.postcondition(0, 0, bad)
        with pytest.raises(EncodeError):
            m.transition(0, ("R", bad))
    batch = codec.encode(m, [[(0, ("L", 0)), (0, ("R", sp.nr))], [(0, ("L", sp.ni)), (0, ("R", 0))]])
    assert set(batch.encode_errors) == {0, 1}


@pytest.mark.parametrize("name", list(rt.KEYED))
def test_keyed_model_reads_the_raw_arrays(name):
    comp, K, model0 = rt.KEYED[name]
    m, t, sp = rt.model(name), rt.tables_of(comp), rt.spec(comp)
    assert isinstance(m, KeyedTableModel) and m.n_keys == K and m.component is rt.model(comp)
    rng = random.Random(f"rawtables/keyed/{name}")
    for _ in range(300):
        s = tuple(rng.randrange(sp.ns) for _ in range(K))
        k, i, r = rng.randrange(K), rng.randrange(sp.ni), rng.randrange(sp.nr)
        if rng.random() < 0.2:
            s = s[:k] + (sp.ns - 1,) + s[k + 1:]
        mid = m.transition(s, ("L", (k, i)))
        assert tuple(mid) == s[:k] + (int(t.on_inv[s[k], i]),) + s[k + 1:]
        assert m.transition(mid, ("R", r)) == s[:k] + (int(t.on_resp[t.on_inv[s[k], i], r]),) + s[k + 1:]
        if t.err[s[k], i, r]:
            with pytest.raises(ModelError):
                m.postcondition(s, (k, i), r)
        else:
            assert m.postcondition(s, (k, i), r) is bool(t.post[s[k], i, r])
    with pytest.raises(EncodeError):
        m.postcondition((0,) * K, (0, 0), sp.nr)


def witness_of_path(hist, path):
    """The device's witness layout for a reference path: per operation the
    index of its pid's first remaining invocation (Lemma L1); an observed
    operation also removes the pid's first remaining response."""
    removed, wit, assumed = set(), [], []
    for op in path:
        pid, resp_assumed = op[0], (op[3] if len(op) > 3 else False)
        i0 = next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "L" and p == pid)
        removed.add(i0)
        wit.append(i0)
        if resp_assumed:
            assumed.append(op[2])           # (the symbols are their own indices)
        else:
            removed.add(next(i for i, (p, (k, _)) in enumerate(hist) if i not in removed and k == "R" and p == pid))
            assumed.append(None)
    return wit, assumed


@pytest.mark.parametrize("name", SHAPES + list(rt.TWINS))
def test_the_oracle_on_the_models_methods_and_replay_witness(name):
    """The literal oracle run with the model's own transition / postcondition
    returns what it returns with the closures, and the reference's paths
    replay (one wrong response at a level does not)."""
    m, c = rt.model(name), rt.closures(name)
    hists, ref = rt.check_case(rt.TWINS.get(name, name), "3x10")
    model0 = rt.model0_of(name)
    init = m.init_model if model0 is None else model0
    assert init == c["init"]
    lin = 0
    for h, want in list(zip(hists, ref))[:120]:
        try:
            got = oracle_linearisable(m.transition, m.postcondition, init, h, rt.MAX_NODES)
        except ModelError:          # (the package's ModelError is not the oracle's)
            got = ("error", None, [])
        assert got[0] == want[0] and (got[0] == "error" or got[1:] == want[1:])
        if want[0] == "lin":
            wit, _ = witness_of_path(h, want[2])
            assert replay_witness(m, h, wit, model0)
            lin += 1
    assert lin >= 10 or name == "n_r2"


@pytest.mark.parametrize("name", PENDING)
def test_replay_witness_with_assumed_responses(name):
    m = rt.model(name)
    model0 = rt.model0_of(name)
    nr = len(m.resps)
    done = rejected = 0
    for setting in ("3x10", "4x16"):
        hists, ref = rt.crash_case(name, setting)
        for h, (st, _, path) in zip(hists, ref):
            if st != "lin" or not any(op[3] for op in path):
                continue
            wit, assumed = witness_of_path(h, path)
            assert replay_witness(m, h, wit, model0, assumed=assumed)
            done += 1
            # another symbol at the first assumed level: a code at or above n_resp never replays (whatever
            # the table's high bits say), one the closures do not allow there does not either
            d = next(k for k, a in enumerate(assumed) if a is not None)
            assert not replay_witness(m, h, wit, model0, assumed=assumed[:d] + [nr] + assumed[d + 1:])
            other = (assumed[d] + 1) % nr
            if other != assumed[d] and not allowed_by_the_closures(name, path, d, other):
                assert not replay_witness(m, h, wit, model0, assumed=assumed[:d] + [other] + assumed[d + 1:])
                rejected += 1
    assert done >= 20 and (rejected > 0 or name == "n_one")


def allowed_by_the_closures(name, path, d, other):
    """Whether the closures allow symbol `other` at level d of `path`."""
    c = rt.closures(name)
    s = c["init"]
    for op in path[:d]:
        s = c["transition"](c["transition"](s, ("L", op[1])), ("R", op[2]))
    return other in pr.allowed(c, s, path[d][1])


@pytest.mark.parametrize("name", list(rt.KEYED))
def test_split_history_is_the_restatements_split(name):
    comp, K, _ = rt.KEYED[name]
    m, c = rt.model(name), rt.closures(comp)
    import anyshape as an
    hists = rt.histories(name, "4x16") + an.batch(rt.closures(name), "6x16", 60) + \
        an.batch(rt.closures(name), an.RANDOM, 100)
    split = 0
    for h in hists:
        want = kref.split(c, K, h)
        assert m.split_history(h) == want
        split += want is not None
    assert rt.BATCHES["4x16"] <= split < len(hists)
