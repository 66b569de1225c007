"""The CPU references of the keyed path's state memo (tests/ktablememo.py):
the literal mirror of ``TableLane::check_step<KeyedModel, MEMO>`` against the exact count on the
product closures for every deep row the GPU tests run
(tests/test_gpu_ktable_memo.py), the run-time cap of those rows, the teeth of
the inputs (a memo keyed on part of the state gets them wrong), and the sizing
arithmetic of the memo's tables built and run on its own.  No GPU."""

import os
import random
import shutil
import subprocess

import pytest

import ktablememo as km
import tablegen as tg
from linearise_lists import linearisable as oracle_linearisable

KEYS_0_3, KEYS_4_7 = 0x00000000FFFFFFFF, 0xFFFFFFFF00000000


@pytest.mark.parametrize("name", sorted(km.KDEEP))
def test_deep_constants(name):
    comp, K, hist, events, status, nodes, states = km.KDEEP[name]
    assert len(hist) == events
    pids = {p for p, _ in hist}
    assert pids == set(range(len(pids)))
    stats = {}
    assert km.exact(name, 0, stats) == (status, nodes)
    assert stats["states"] == states


@pytest.mark.parametrize("name", sorted(km.KDEEP))
def test_mirror_equals_the_exact_count(name):
    status, nodes = km.KDEEP[name][4:6]
    st, nd, path, iters, hits = km.mirror(name, 4096)
    print(name, 4096, st, nd, iters, hits)
    assert (st, nd) == (status, nodes)
    assert hits > 0 and iters <= km.ITERATION_CAP
    assert (path != []) == (status == "lin")


@pytest.mark.parametrize("entries,name", [(e, n) for e in sorted(km.LOSSY) for n in km.LOSSY[e]])
def test_mirror_with_lossy_tables(entries, name):
    status, nodes = km.KDEEP[name][4:6]
    st, nd, _, iters, hits = km.mirror(name, entries)
    print(name, entries, st, nd, iters, hits)
    assert (st, nd) == (status, nodes)
    assert hits > 0 and iters <= km.ITERATION_CAP      # the run-time cap of the GPU test


@pytest.mark.parametrize("name,max_nodes,want", km.BUDGET_CASES)
def test_budget_inside_a_hit(name, max_nodes, want):
    assert km.exact(name, max_nodes) == want
    st, nd, _, iters, hits = km.mirror(name, 4096, max_nodes)
    assert (st, nd) == want and hits > 0 and iters <= km.ITERATION_CAP
    if want[0] == "budget":
        assert nd == max_nodes


def test_small_rows_equal_the_oracle_and_the_plain_search():
    for name in ("kreads_2_3x2", "klin_deep_2_3_2", "klock_deep_3_3_2"):
        comp, K, hist, _, status, nodes, _ = km.KDEEP[name]
        p = km.product(comp, K)
        st, nd, path = oracle_linearisable(p["transition"], p["postcondition"], p["init"], hist)
        assert (st, nd) == (status, nodes)
        plain = km.kmemo_dfs(comp, K, hist, 0)
        assert plain == (st, nd, path)
        for entries in (2, 16, 4096):
            assert km.mirror(name, entries)[:3] == plain
    assert km.mirror("klin_deep_2_3_2", 4096)[2] != []


@pytest.mark.parametrize("comp", ["register", "lock"])
def test_mirror_equals_the_oracle_on_generated_histories(comp):
    p = km.product(comp, 3)
    rng = random.Random(f"kmemo-host/{comp}")
    seen = set()
    for k in range(60):
        c, ops, bug = ((4, 12, 0.05), (3, 10, 0.1), (2, 8, 0.05))[k % 3]
        h = tg.gen_history(p, rng, c, ops, bug)
        for max_nodes in (0, 50):
            ref = oracle_linearisable(p["transition"], p["postcondition"], p["init"], h, max_nodes)
            seen.add(ref[0])
            for entries in (0, 2, 64):
                assert km.kmemo_dfs(comp, 3, h, entries, max_nodes) == ref, (h, max_nodes, entries)
    assert {"lin", "nonlin", "budget"} <= seen


def weakened(name, mask):
    comp, K, hist = km.KDEEP[name][:3]
    return km.kmemo_dfs(comp, K, hist, 4096, state_mask=mask)[:2]


def test_the_inputs_keep_their_teeth():
    """A memo whose key holds only part of the state gets these rows wrong."""
    for name in ("kreads_8_4x4_k7373", "kreads_8_4x8_k76543210", "kreads_8_4x12", "klin_deep_8_4_8"):
        assert weakened(name, KEYS_0_3) != km.KDEEP[name][4:6], name
    for name in ("kreads_8_4x8_k76543210", "kreads_8_4x12", "klin_deep_5_4_4", "klin_deep_8_4_2", "klin_deep_8_4_8"):
        assert weakened(name, KEYS_4_7) != km.KDEEP[name][4:6], name
    assert weakened("klin_deep_8_4_2", 0)[0] == "nonlin"


def test_the_memo_sizing_stand_alone(tmp_path):
    """tools/ktable_memo_host_check.cpp: csrc/ktable_host.h's ktable_memo_ok /
    ktable_memo_plan built under AddressSanitizer and UBSan and run as a
    program of its own, no device."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "ktable_memo_host_check")
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(root, "include"),
                    "-I", os.path.join(root, "quickcheck-state-machine-distributed_amd", "csrc"),
                    "-x", "hip", os.path.join(root, "tools", "ktable_memo_host_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ktable memo host checks ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
