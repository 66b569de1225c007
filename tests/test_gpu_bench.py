"""bench.py end to end on one GPU at a small size: --full with its extra
configs (BASELINE configs 1, 3, 4, 5 at their own sizes) and their oracle
checks, the one JSON line the driver parses, with the fields it and the
judge read; a plain run, which times the steps and nothing else, and the
outputs it writes with --dump-outputs."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_bench_one_gpu_with_extra_configs():
    cmd = [sys.executable, "bench.py", "--full", "--steps", "4", "--warmup", "2", "--n-hist", "20000",
           "--rotate", "3", "--no-cpu-baseline", "--roof-calls", "3"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280,
                       env=dict(os.environ, PYTHONUNBUFFERED="1"))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["value"] > 0 and d["higher_is_better"]
    assert d["verdicts"]["checked"] + d["verdicts"]["budget"] <= 4 * 20000
    r = d["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(r)
    assert set(r["kernels"]) >= {"stage0"}
    ex = d["extra"]["configs"]
    for k in ("config1", "config3", "config5"):
        assert ex[k]["mismatches_vs_oracle"] == 0 and ex[k]["histories_per_sec"] > 0
    assert ex["config4"]["verdict_matches_oracle"]


def test_bench_plain_run_dumps_last_step(tmp_path):
    """A plain run: the headline's fields and none of the legs behind --full;
    --dump-outputs writes the last timed step's status, node count and
    totals, which are the oracle's for that step's batch (step 4 of 5 over 3
    resident batches: batch 1, histories [n, 2n) of the seeded stream)."""
    import oracle_c
    from qsmd import codec, gen, models
    n, steps = 20000, 5
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--n-hist", str(n),
           "--rotate", "3", "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=200,
                       env=dict(os.environ, PYTHONUNBUFFERED="1"))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["value"] > 0 and d["higher_is_better"]
    assert d["unit"] == "histories/s" and d["dtype"] == "int32" and d["metric"]
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 / n - 1) < 1e-9
    assert d["verdicts"]["checked"] + d["verdicts"]["budget"] == steps * n
    assert not {"roofline", "extra", "mismatches_vs_oracle"} & set(d) and d["cpu_baseline"] is None
    assert sorted(os.listdir(tmp_path / "out")) == ["nodes.npy", "status.npy", "totals.npy"]
    st, nd, tot = (np.load(tmp_path / "out" / f"{k}.npy") for k in ("status", "nodes", "totals"))
    assert st.dtype == np.float32 and nd.dtype == np.float64 and tot.dtype == np.float64
    hdr, ev, _ = gen.generate_config("bank_4x16", ((steps - 1) % 3) * n, n)
    st_o, nd_o, _ = oracle_c.check_batch(models.MODEL_BANK, hdr, ev, threads=4, max_nodes=0)
    assert np.array_equal(st, st_o.astype(np.float32)) and np.array_equal(nd, nd_o.astype(np.float64))
    assert tot.shape == (8,) and tot[0] == n and tot[1] == (st_o == codec.STATUS_LIN).sum() and tot[7] == nd_o.sum()


@pytest.mark.parametrize("plant", [None, 0.6])
def test_bench_early_exit_leg(plant):
    """The early-exit leg on one GPU: config 3 (its first failure is its
    second history: one round decides) and config 2's stream with one
    failure planted at 60 % of the batch (the geometric rounds up to it, a
    MIN per round): the decision's latency, the histories searched, and the
    statuses against the oracle cut (every history up to the first failure
    the oracle's, every later one SKIPPED)."""
    n = 60000
    cmd = [sys.executable, "bench.py", "--full", "--early-exit", "--steps", "2", "--warmup", "1", "--n-hist", str(n)]
    if plant is not None:
        cmd += ["--plant", str(plant)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=200,
                       env=dict(os.environ, PYTHONUNBUFFERED="1"))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    ee = d["early_exit"]
    assert d["ms_to_decision"] == ee["ms_to_decision"] > 0
    assert d["value"] == ee["histories_searched_per_sec"] > 0
    assert ee["mismatches_vs_oracle"] == 0
    assert ee["searched"] + ee["skipped"] == n
    if plant is None:
        assert ee["workload"] == "bank_4x16_bugs" and ee["rounds"] == 1 and ee["first_fail"] < 4096
    else:
        at = int(plant * n)
        assert ee["workload"] == "bank_4x16" and ee["planted_at"] == at == ee["first_fail"]
        assert ee["rounds"] > 2 and ee["searched"] >= at + 1
        assert ee["totals"]["nonlinearisable"] + ee["totals"]["model_errors"] == 1
