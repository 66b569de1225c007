"""The raw-table inputs (tests/rawtables.py) on the host.

1. The inputs have teeth: conditions on the *reference alone*
   (oracle/linearise_lists.py, tests/pending_ref.py run with rawtables'
   closures), asserted for every shape before anything is sent to a GPU --
   every status is reached, the deep shapes pass pass 1's budget, and
   replacing ``on_resp`` by identity rows changes (status, nodes) on at least
   half of the histories: these inputs see the fourth table.
2. The Python mirror (qsmd.models.TableModel / WideTableModel /
   KeyedTableModel, replay_witness, split_history) against the raw arrays.
3. The same for the keyed pending call's local mode (knob "kpending_local",
   tests/kpendinglocal_ref.py): the conditions on the restatement that keep
   tests/test_gpu_rawtables_kpending_local.py from passing vacuously, the
   local verdicts against the product's, and split_history(pending=True)."""

import collections

import random

import numpy as np
import pytest

import anyshape as an
import kpendinglocal_ref as klr
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
    return rt.spec(rt.keyed_spec(name)[0] if rt.keyed_spec(name) else name).p_err is not None


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


# ------------------------------------- 3. the keyed pending call's local mode on raw tables

LOCAL = list(rt.LOCAL_SHAPES)
TWO_KEYS = ["k2_deep", "k2_r32"]
WALKS = ["k8_1inv", "k8_r2"]
ALL_KEYED = list(rt.KEYED) + list(rt.KEYED_LOCAL)
# what the restatement counts on the frozen batches, over all settings (DESIGN.md §10l records them; the GPU
# module prints its pass-2 counts beside the first): parts beyond pass 1's 256 nodes at MAX_NODES; at LOW_NODES
# the histories a `budget` part decides, those where one lies behind a lower failing key, those whose summed
# nodes pass LOW_NODES; the product's `budget` histories the local mode decides at MAX_NODES
PARTS_BEYOND_256 = {"k2_deep": 1, "k2_r32": 5}
LOW = {"k2_deep": (18, 1, 24), "k2_r32": (27, 5, 45)}
PRODUCT_BUDGET_DECIDED = {"k_max": 30, "k_deep": 13, "k_odd": 11, "k2_deep": 2, "k2_r32": 9}


def test_the_local_shapes_are_apart_from_the_keyed_ones():
    assert not set(rt.KEYED) & set(rt.KEYED_LOCAL) and not set(rt.KEYED_LOCAL) & set(SHAPES)
    assert set(rt.LOCAL_SHAPES) <= set(ALL_KEYED) and set(TWO_KEYS + WALKS) == set(rt.KEYED_LOCAL)
    for name, (comp, K, model0) in rt.KEYED_LOCAL.items():
        m, c = rt.model(name), rt.closures(name)
        assert isinstance(m, KeyedTableModel) and m.n_keys == K and m.component is rt.model(comp)
        assert rt.model0_of(name) == model0 and c["name"] == name
        assert c["init"] == rt.inits_of(name) == (model0 or (rt.spec(comp).init,) * K)
    # k8_r2 starts every state of n_r2 somewhere, and not every key at 0
    assert set(rt.inits_of("k8_r2")) == set(range(rt.spec("n_r2").ns)) and len(rt.inits_of("k8_r2")) == 8
    assert rt.inits_of("k_max") == (255, 0, 17, 255, 128, 3, 254, 1)
    assert 0 < rt.LOW_NODES < 256 < rt.MAX_NODES


def part_state(comp, s, inv, r):
    t = rt.tables_of(comp)
    return int(t.on_resp[t.on_inv[s, inv], r])


@pytest.mark.parametrize("name", LOCAL)
def test_local_crashed_batches_have_teeth(name):
    comp, K, model0 = rt.keyed_spec(name)
    c, init = rt.closures(comp), rt.inits_of(name)
    changed = changed_err = total = assumed_parts = invocations_only = 0
    symbols, nexts = set(), set()
    for setting, n in rt.BATCHES.items():
        hists, parts, combined, paths = rt.local_crash_case(name, setting)
        assert len(hists) == n and all(p is not None for p in parts)          # every history is splittable
        assert combined == [klr.check(c, K, h, rt.MAX_NODES, model0) for h in hists]
        assert sum(1 for h in hists if pr.pending_invocations(h)) > n // 3
        if not (name in TWO_KEYS and setting == "3x10"):
            assert sum(1 for p in parts if len(p) > 1) > n // 2
        subs = [sub for h in hists for _, sub in klr.split(c, K, h)]
        # (k_odd's frozen 6x24 batch -- 3 keys, 24 operations -- has no such part: the condition is the shape's)
        invocations_only += sum(1 for sub in subs if all(e[1][0] == "L" for e in sub))
        ident = rt.local_crash_case(name, setting, rt.MAX_NODES, "identity_resp")[2]
        changed += sum(1 for a, b in zip(combined, ident) if a != b)
        plain = rt.local_crash_case(name, setting, rt.MAX_NODES, "ignore_err")[2]
        changed_err += sum(1 for a, b in zip(combined, plain) if a != b)
        total += n
        # parts that are linearisable only through an assumed response
        for p, pa in zip(parts, paths):
            for (k, st, _), path in zip(p, pa):
                if st != "lin" or not any(op[3] for op in path):
                    continue
                assumed_parts += 1
                s = init[k]
                for _, inv, r, assumed in path:
                    nxt = part_state(comp, s, inv, r)
                    if assumed:
                        symbols.add(r)
                        nexts.add(nxt)
                    s = nxt
    print(name, "changed by identity_resp:", changed, "by ignore_err:", changed_err, "of", total,
          "parts with an assumed response:", assumed_parts, "parts of invocations only:", invocations_only)
    assert invocations_only >= 1
    assert 2 * changed >= total
    assert has_err(name) and changed_err >= 1
    assert assumed_parts >= 10 and len(symbols) >= 2 and len(nexts) >= 2


@pytest.mark.parametrize("name", LOCAL)
def test_local_verdicts_against_the_products(name):
    """Locality on raw tables: `lin` is `lin` on both sides wherever the
    product decides, and a disagreement is the product's `budget` or a swap
    within {error, nonlin}; the local mode decides some of those `budget`."""
    pairs = collections.Counter()
    for setting in rt.BATCHES:
        hists, ref = rt.crash_case(name, setting)
        hists2, _, combined, _ = rt.local_crash_case(name, setting)
        assert hists2 is hists
        pairs.update((r[0], c[0]) for r, c in zip(ref, combined))
    print(name, "(product, per key):", dict(pairs))
    for (whole, local), n in pairs.items():
        if whole != "budget":
            assert (whole == "lin") == (local == "lin"), (whole, local, n)
        assert whole == local or whole == "budget" or {whole, local} == {"error", "nonlin"}, (whole, local, n)
    decided = sum(n for (whole, local), n in pairs.items() if whole == "budget" and local != "budget")
    assert decided >= 1 and decided == PRODUCT_BUDGET_DECIDED[name]


def test_a_product_error_that_is_lin_key_by_key():
    """The third kind of disagreement, which the frozen batches do not hold
    (rawtables.LOCAL_CRASH_SALT): the product search raises where no key's own
    search does."""
    h = rt.ERROR_LIN_KAT
    assert pr.linearisable_pending(rt.closures("k2_r32"), h, rt.MAX_NODES)[:2] == ("error", 20)
    assert rt.local_parts("k2_r32", h, rt.MAX_NODES)[0] == [(0, "lin", 9), (1, "lin", 11)]
    assert klr.check(rt.closures("n_r32"), 2, h, rt.MAX_NODES) == ("lin", 20)
    # without post_err both are `lin`: the raise is all that differs
    c = rt.closures("k2_r32", ignore_err=True)
    assert pr.linearisable_pending(c, h, rt.MAX_NODES)[0] == "lin"


@pytest.mark.parametrize("name", TWO_KEYS)
def test_two_key_parts_pass_pass_1_and_reach_a_low_max_nodes(name):
    beyond = sum(1 for s in rt.BATCHES for p in rt.local_crash_case(name, s)[1] for _, _, nd in p if nd > 256)
    print(name, "parts beyond 256 nodes at", rt.MAX_NODES, ":", beyond)
    assert beyond >= 1 and beyond == PARTS_BEYOND_256[name]
    assert not any(st == "budget" for s in rt.BATCHES for p in rt.local_crash_case(name, s)[1] for _, st, _ in p)
    low = rt.LOW_NODES
    decides = behind = over = 0
    for setting in rt.BATCHES:
        _, parts, combined, _ = rt.local_crash_case(name, setting, low)
        for p, (status, nodes) in zip(parts, combined):
            sts = [st for _, st, _ in p]
            assert all(nd == low for _, st, nd in p if st == "budget")
            assert all(nd <= low for _, _, nd in p) and nodes == sum(nd for _, _, nd in p)
            if status == "budget":              # the lowest part that is not lin is a `budget` one
                assert all(st == "lin" for st in sts[:sts.index("budget")])
                decides += 1
            elif "budget" in sts:               # a `budget` part behind a lower failing key: the lower key's status
                assert status in ("nonlin", "error") and sts.index(status) < sts.index("budget")
                behind += 1
            over += nodes > low
    print(name, "at max_nodes", low, "- budget decides:", decides, "budget behind a lower key:", behind,
          "summed nodes beyond it:", over)
    assert decides >= 3 and behind >= 1 and over >= 1
    assert (decides, behind, over) == LOW[name]


@pytest.mark.parametrize("name", WALKS)
def test_keyed_walks(name):
    comp, K, _ = rt.keyed_spec(name)
    m, sp, init = rt.model(comp), rt.spec(comp), rt.inits_of(name)
    assert sp.high == "post" and K == 8
    h, ends = rt.keyed_walk(name, rt.WALK_PER_KEY)
    assert len(h) == 128 and len({pid for pid, _ in h}) == 128 and max(pid for pid, _ in h) == 127
    assert [x[0] for _, (_, x) in h[:K]] == list(range(K))          # round-robin over the keys
    for k in range(K):
        s = init[k]
        mine = [(pid, x[1]) for pid, (kind, x) in h if kind == "L" and x[0] == k]
        assert [pid for pid, _ in mine] == list(range(k * rt.WALK_PER_KEY, (k + 1) * rt.WALK_PER_KEY))
        for _, i in mine:
            word = int(m.post[s, i])
            assert word >> sp.nr == (1 << (32 - sp.nr)) - 1         # bits at and above n_resp
            a = word & ~int(m.post_err[s, i]) & ((1 << sp.nr) - 1)
            assert a == rt.allowed_bits(comp, s, i) and bin(a).count("1") >= 2
            s = part_state(comp, s, i, (a & -a).bit_length() - 1)
        assert s == ends[k]
    hists, parts, combined, product = rt.walk_case(name)
    assert hists[0] == h and parts[0] == [(k, "lin", rt.WALK_PER_KEY) for k in range(K)] and combined[0] == ("lin", 128)
    assert product[0][:2] == ("lin", 128)
    # the short walk: one completed operation the end state of the highest key does not allow
    short, k, (i, r) = rt.failing_walk(name)
    walk, ends = rt.keyed_walk(name, rt.SHORT_WALK)
    assert hists[1] == short and short[:-2] == walk and k == K - 1
    assert short[-2:] == [(K * rt.SHORT_WALK, ("L", (k, i))), (K * rt.SHORT_WALK, ("R", r))]
    assert not (rt.allowed_bits(comp, ends[k], i) >> r) & 1 and not rt.tables_of(comp).err[ends[k], i, r]
    assert [(key, st) for key, st, _ in parts[1]] == [(q, "lin") for q in range(K - 1)] + [(k, "nonlin")]
    assert all(nd == rt.SHORT_WALK for _, _, nd in parts[1][:-1]) and rt.SHORT_WALK < parts[1][-1][2] < rt.MAX_NODES
    assert combined[1] == ("nonlin", (K - 1) * rt.SHORT_WALK + parts[1][-1][2])
    print(name, "the failing key's part:", parts[1][-1], "the product:", product[1][:2])


def test_empty_allowed_words():
    """Rule 2 where the allowed word is empty only after the `& symbols` cut
    and post_err: a lone pending invocation there is `lin` with 0 nodes."""
    assert not rt.empty_allowed("n_1inv") and not rt.empty_allowed("c_odd")
    pairs = rt.empty_allowed("n_r2")
    m, t = rt.model("n_r2"), rt.tables_of("n_r2")
    assert len(pairs) >= 10
    for s, i in pairs:
        word = int(m.post[s, i])
        assert word and not word & ~int(m.post_err[s, i]) & 3 and not (t.post[s, i] & ~t.err[s, i]).any()
    assert any(int(m.post[s, i]) & int(m.post_err[s, i]) & 3 for s, i in pairs)     # some bit post_err removes
    cases = rt.empty_allowed_histories("k8_r2")
    assert not rt.empty_allowed_histories("k8_1inv")
    init, c = rt.inits_of("k8_r2"), rt.closures("n_r2")
    assert {s for s, _ in pairs} == {s for s, _, _, _ in cases} and any(s != 0 for s, _, _, _ in cases)
    hists, parts, combined, product = rt.walk_case("k8_r2")
    assert len(hists) == 2 + 3 * len(cases)
    for n, (s, i, k, (h1, h2, h3)) in enumerate(cases):
        assert init[k] == s and h1 == [(0, ("L", (k, i)))] and h2[:1] == h3[:1] == h1
        assert hists[2 + 3 * n:5 + 3 * n] == [h1, h2, h3]
        p1, p2, p3 = parts[2 + 3 * n:5 + 3 * n]
        assert p1 == [(k, "lin", 0)] and klr.check(c, 8, h1, rt.MAX_NODES, init) == ("lin", 0)
        k2 = h2[1][1][1][0]
        assert k2 != k and sorted(p2) == sorted([(k, "lin", 0), (k2, "lin", 1)])
        assert combined[3 + 3 * n] == ("lin", 1)
        assert h3[1][1][1][0] == k and [key for key, _, _ in p3] == [k]
        assert combined[4 + 3 * n] == klr.check(c, 8, h3, rt.MAX_NODES, init)
    assert {c[0] for c in combined[2:]} == {"lin"} and {c[1] for c in combined[4::3]} >= {1, 2}


def split_inputs(name):
    c = rt.closures(name)
    hists = [h for s in rt.BATCHES for h in rt.crashed(name, s)]
    rng = random.Random(f"rawtables/split/{name}")
    for setting, n in (("6x16", 60), (an.RANDOM, 100)):
        some = an.batch(c, setting, n)
        hists += some + [pr.crash(h, rng, rt.CRASH) for h in some]
    return hists


@pytest.mark.parametrize("name", ALL_KEYED)
def test_split_history_pending_is_the_restatements_split(name):
    comp, K, _ = rt.keyed_spec(name)
    m, c, sp = rt.model(name), rt.closures(comp), rt.spec(comp)
    reasons = collections.Counter()
    differs = 0
    for h in split_inputs(name):
        want = klr.split(c, K, h)
        reason = klr.refusal(c, K, h)
        assert (want is None) == (reason is not None)
        assert m.split_history(h, pending=True) == want, h
        reasons[reason] += 1
        plain = kref.split(c, K, h)                             # the default split is unchanged
        assert m.split_history(h) == plain and m.split_history(h, pending=False) == plain, h
        differs += plain != want
    print(name, dict(reasons))
    # the reasons an encodable history of at most 128 events can show, and splits of both kinds
    assert reasons[None] >= sum(rt.BATCHES.values()) and reasons["lone_response"] and reasons["two_in_flight"]
    assert differs > sum(rt.BATCHES.values()) // 3 and set(reasons) <= {None, "lone_response", "two_in_flight"}
    # the others, made by hand
    long = an.exactly(rt.histories(name, "6x24")[0], 129)
    by_hand = {"too_long": long, "symbol": [(0, ("L", (0, 0))), (0, ("R", sp.nr))],
               "key": [(0, ("L", (K, 0))), (0, ("R", 0))]}
    assert set(by_hand) | {"lone_response", "two_in_flight"} == set(klr.REASONS)
    for reason, h in by_hand.items():
        assert klr.refusal(c, K, h) == reason and klr.split(c, K, h) is None
        assert m.split_history(h, pending=True) is None and m.split_history(h) is None
    assert klr.split(c, K, long[:128]) is not None and m.split_history(long[:128], pending=True) is not None


@pytest.mark.parametrize("name", ["k_deep", "k_odd", "k_max"])
def test_complete_histories_are_the_check_calls_local_mode(name):
    comp, K, model0 = rt.keyed_spec(name)
    c = rt.closures(comp)
    for setting in rt.BATCHES:
        for h in rt.histories(name, setting):
            assert not pr.pending_invocations(h)
            assert klr.check(c, K, h, rt.MAX_NODES, model0) == kref.check(c, K, h, rt.MAX_NODES, model0)
