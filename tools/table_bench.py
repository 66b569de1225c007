"""Throughput of the table-driven model (csrc/table.hip, QSMD_MODEL_TABLE).

Workload: the register model (Write / Read / Cas on values 0..3) on the
4 clients x 16 operations generator of tests/tablegen.py with p_bug 0.03:
65,536 distinct histories tiled to 1M, device-resident, one check call at a
time.  Per pass-1 budget ("table_budget"; `default` = the library's, 0 = a
single pass): 5 warm-up calls, 20 timed calls (HIP events on the stream),
the median ms per call, histories/s, nodes/s and pass 2's share of the batch.
One JSON line per budget and memo size ("table_memo", --memo: entries per
lane slot of pass 2's state memo, 0 = off), the sizes crossed with every
budget.  --rounds R repeats the whole cross R times (interleaved).

--wide both runs every configuration as QSMD_MODEL_TABLE and then as
QSMD_MODEL_WTABLE (csrc/wtable.hip: the tables in device memory) on the same
batch with only hdr.model_id changed, the two interleaved: what a model that
fits the narrow table pays on the wide path.  --wide 1 runs the wide path
alone.  --model kv is the 5-key, 4-value store of tests/wtablegen.py (1,024
states, 105 invocations), which only the wide path holds.

--generated: the batch is --n DISTINCT histories generated on the device
(csrc/tgen.hip, Context.gen_table_device) from (seed, index) over the same
tables: 4 clients x 16 operations, executed at the invocation as
tests/tablegen.py's are, one response bug in 39 % of the histories (its 3 %
per operation over 16).  No tiling and no host-to-device copy.  With an
explicit --distinct D the first D generated histories are tiled to --n on the
device instead, which isolates what tiling does to the measurement.  Without
the flag the tool does exactly what it did before it had one.

--keyed K: the keyed path (csrc/ktable.hip, QSMD_MODEL_KTABLE).  K = 1 runs
the register batch above as QSMD_MODEL_TABLE and as KeyedTableModel(register,
1), the same histories, interleaved: what the keyed step costs.  K > 1 runs
4x16 histories of the register on K keys (tests/ktablegen.py's product
generator) as QSMD_MODEL_KTABLE and, re-encoded, as QSMD_MODEL_WTABLE on the
flat product (4^K states, 21 K invocations; K <= 4 tabulates in seconds),
interleaved: what factoring buys.  Not with --wide or --model kv.
--keyed K --generated: the model-5 line alone, on --n DISTINCT keyed
histories generated on the device (csrc/ktgen.hip, Context.gen_ktable_device)
with --generated's settings, unit weights; --distinct D tiles the first D as
above.  No flat product is tabulated, so any K in 1..8 runs.
--memo sizes the keyed path's memo through its own knob ("ktable_memo") on
the model-5 lines and "table_memo" on the others; every line carries the hits.
--local 0,1 (with --keyed): the model-5 lines with the keyed path's local mode
off and on (knob "ktable_local", csrc/ksplit.hip: every splittable history
checked key by key), crossed with the budgets and memo sizes; a line carries
"ktable_local" and the histories that were split.  --clients C --ops K --p-bug P
shape the --generated batch (default 4, 16 and 0.39: P is the probability that
a history gets its one response bug, 1 - 0.97^K for 3 % per operation).

--explain: every configuration is also timed as an explain call
(qsmd_explain_batch_device: the check's search with the deepest linearised path
of every history recorded, always without a memo and on the product), the two
interleaved; a line carries "call": "check" or "explain".

--pending: every configuration is also timed as qsmd_check_pending_batch_device
(csrc/tpending.hip: pending invocations may take effect) on the same, complete
batch -- what the wider stack and the extra branch cost where nothing is
pending -- and on the same histories with clients crashed (tests/pending_ref.py
crash, probability 0.3 per client), the three interleaved; a line carries
"call": "check" or "pending" and "batch": "complete" or "crash 0.3".  With
--memo the pending lines run with the pending call's own knob ("pending_memo",
DESIGN.md §10j) at that size and carry "pending_memo" and "pending_memo_hits".  The
register batch of the default run, or with --keyed K the keyed batch above as
QSMD_MODEL_KTABLE alone (no flat product): the keyed check call against
qsmd_check_kpending_batch_device (csrc/kpending.hip), which has
no memo -- --memo sizes the check lines only.  --keyed K --pending --local adds
the keyed pending call's own local mode (knob "kpending_local", DESIGN.md §10l:
every history splittable with pending invocations checked key by key) on the
complete and on the crashed batch, five calls interleaved; a pending line
carries "kpending_local" and "kpending_local_last", and "ktable_local" stays 0.
With --pending, --clients C --ops K shape the host generator's batch (3 % per
operation as before).

    python tools/table_bench.py [--budgets default,0] [--memo 0,64,256,1024,4096] [--distinct 65536] [--n 1048576]
                                [--wide 0|1|both] [--model register|kv] [--generated] [--seed S] [--keyed K]
                                [--local [0,1]] [--clients C] [--ops K] [--p-bug P] [--explain] [--pending]
"""

import argparse
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("quickcheck-state-machine-distributed_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import tablegen as tg  # noqa: E402
from qsmd import codec, device, gen  # noqa: E402
from qsmd.models import KeyedTableModel, TableModel, WideTableModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budgets", default="default,0")
    ap.add_argument("--memo", default="0")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--distinct", type=int, default=None)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--max-nodes", type=int, default=tg.MAX_NODES)
    ap.add_argument("--wide", default="0", choices=["0", "1", "both"])
    ap.add_argument("--model", default="register", choices=["register", "kv"])
    ap.add_argument("--generated", action="store_true")
    ap.add_argument("--seed", type=int, default=0x7AB1E)
    ap.add_argument("--keyed", type=int, default=0)
    ap.add_argument("--local", nargs="?", const="1", default="0")
    ap.add_argument("--clients", type=int, default=4)
    ap.add_argument("--ops", type=int, default=16)
    ap.add_argument("--p-bug", type=float, default=0.39)
    ap.add_argument("--explain", action="store_true")
    ap.add_argument("--pending", action="store_true")
    args = ap.parse_args()
    if args.pending and (args.generated or args.wide != "0" or args.model != "register" or args.explain):
        ap.error("--pending runs the register batch of the default run (or of --keyed K) alone")
    if args.pending and args.keyed and args.local not in ("0", "1"):
        ap.error("--pending --local: the keyed pending call's local mode beside the product route (no value)")
    if args.local != "0" and not args.keyed:
        ap.error("--local is the keyed path's (--keyed K)")
    if ((args.clients, args.ops) != (4, 16) and not (args.generated or args.pending)) or \
            (args.p_bug != 0.39 and not args.generated):
        ap.error("--clients / --ops shape the --generated or the --pending batch, --p-bug the --generated one")
    kpending_local = args.pending and args.keyed and args.local == "1"
    if args.pending:
        args.local = "0"                    # (the check lines stay on the product)
    if args.keyed and (args.wide != "0" or args.model != "register"):
        ap.error("--keyed runs the register model alone")
    tiled = args.distinct is not None or not args.generated
    if args.distinct is None:
        args.distinct = 65536 if tiled else args.n
    import torch

    if args.model == "kv":
        import wtablegen as wg
        model, args.wide = wg.KV, "1"
    else:
        model = tg.REGISTER
    ids = {"0": [3], "1": [4], "both": [3, 4]}[args.wide]
    closures = (model["transition"], model["postcondition"], model["init"], model["invs"], model["resps"])
    m = (TableModel if 3 in ids else WideTableModel).from_closures(*closures)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = device.Context(0, time_limit_ms=60000)
    if 3 in ids:
        ctx.set_table(m)
    if 4 in ids:
        ctx.set_wide_table(m if isinstance(m, WideTableModel) else WideTableModel.from_closures(*closures))
    encoders = {mid: m for mid in ids}      # model id -> the model that encodes the batch for it
    if args.keyed:
        import ktablegen as kg
        km = KeyedTableModel(m, args.keyed)
        ctx.set_keyed_table(km)
        if args.generated or args.pending:
            ids, encoders = [5], {5: km}
            if args.keyed > 1 and not args.generated:
                model = kg.product(model, args.keyed)
        elif args.keyed == 1:
            ids, encoders = [3, 5], {3: m, 5: km}
        else:
            model = kg.product(model, args.keyed)
            flat = WideTableModel.from_closures(model["transition"], model["postcondition"], model["init"],
                                                model["invs"], model["resps"])
            ctx.set_wide_table(flat)
            ids, encoders = [5, 4], {5: km, 4: flat}
    reps = (args.n + args.distinct - 1) // args.distinct
    n = reps * args.distinct
    d_hdrs, d_evs = {}, {}
    if args.generated:
        per = 2 * args.ops
        sched = dict(n_clients=args.clients, n_ops=args.ops, prefix_ops=0, lin_policy=gen.LIN_AT_INVOKE,
                     pid_mode=gen.PID_PER_CLIENT, p_bug=args.p_bug, seed=args.seed)
        gp, kgp = gen.table_params(**sched), gen.ktable_params(**sched)
        d_ev = torch.empty(n * per * 8, dtype=torch.uint8, device=dev)
        for mid in ids:                     # the same stream from either table: only hdr.model_id differs
            h = torch.empty(n * 16, dtype=torch.uint8, device=dev)
            if mid == 5:
                ctx.gen_ktable_device(kgp, 0, args.distinct, h.data_ptr(), d_ev.data_ptr(), None, stream=stream)
            else:
                ctx.gen_table_device(gp, 0, args.distinct, h.data_ptr(), d_ev.data_ptr(), None, stream=stream,
                                     wide=mid == 4)
            torch.cuda.synchronize()
            if reps > 1:                    # tile on the device: ev_off moves on by one tile's events
                first = h[:args.distinct * 16].view(torch.int32).view(args.distinct, 4)
                tiles = first.repeat(reps, 1)
                tiles[:, 0] += torch.arange(reps, device=dev, dtype=torch.int32).repeat_interleave(
                    args.distinct) * (args.distinct * per)
                h = tiles.view(torch.uint8).reshape(-1)
            d_hdrs[mid] = h
        if reps > 1:
            d_ev = d_ev[:args.distinct * per * 8].repeat(reps)
        d_evs[ids[0]] = d_ev
        n_events = n * per
        name = args.model + (f"^{args.keyed}" if args.keyed else "")
        what = (f"{name} {args.clients}x{args.ops} generated on the device (seed {args.seed:#x}, p_bug {args.p_bug}), " +
                (f"{args.distinct} distinct tiled to {n}" if reps > 1 else f"{n} distinct"))
    else:
        rng = random.Random("table_bench")
        hists = [tg.gen_history(model, rng, args.clients, args.ops, 0.03) for _ in range(args.distinct)]
        def encoded(mid, hs):               # the histories in a model's encoding
            if args.keyed == 1 and mid == 5:        # the one key
                hs = [[(p, (k, (0, x) if k == "L" else x)) for p, (k, x) in h] for h in hs]
            return codec.encode(encoders[mid], hs)

        for mid in ids:                     # the same histories, in each model's encoding
            batch = encoded(mid, hists)
            assert not batch.encode_errors
            per = len(batch.events)
            hdr = np.tile(batch.hdr, reps)
            hdr["ev_off"] = (hdr["ev_off"].astype(np.int64) + np.repeat(np.arange(reps, dtype=np.int64) * per,
                                                                         args.distinct)).astype(np.uint32)
            hdr["model_id"] = mid
            d_hdrs[mid] = torch.from_numpy(hdr.view(np.uint8).copy()).to(dev)
            if args.keyed or not d_evs:     # (without --keyed the events are the same for every id: one copy)
                d_evs[mid] = torch.from_numpy(np.tile(batch.events, reps).view(np.uint8)).to(dev)
        n_events = per * reps
        if args.pending:                    # the same histories with clients crashed, tiled alike
            import pending_ref
            crash_rng = random.Random("table_bench/crash")
            batch = encoded(ids[0], [pending_ref.crash(h, crash_rng, 0.3) for h in hists])
            assert not batch.encode_errors
            per_c = len(batch.events)
            hdr = np.tile(batch.hdr, reps)
            hdr["ev_off"] = (hdr["ev_off"].astype(np.int64) + np.repeat(np.arange(reps, dtype=np.int64) * per_c,
                                                                         args.distinct)).astype(np.uint32)
            hdr["model_id"] = ids[0]
            d_hdr_c = torch.from_numpy(hdr.view(np.uint8).copy()).to(dev)
            d_ev_c = torch.from_numpy(np.tile(batch.events, reps).view(np.uint8)).to(dev)
            n_events_c = per_c * reps
        what = (f"{model['name']} {args.clients}x{args.ops} p_bug 0.03, {args.distinct} distinct tiled to {n}, "
                "device-resident")
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nd = torch.empty(n, dtype=torch.int64, device=dev)
    d_tot = torch.zeros(8, dtype=torch.int64, device=dev)
    if args.explain:
        d_path = torch.empty(n_events, dtype=torch.uint8, device=dev)
        d_rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    default = ctx.get_param("table_budget")
    cross = [(b, int(e), mid, int(loc), call) for _ in range(args.rounds) for b in args.budgets.split(",")
             for e in args.memo.split(",") for mid in ids for loc in (args.local.split(",") if mid == 5 else "0")
             for call in (("check", "explain") if args.explain else
                          ("check", "pending", "pending/crash") +
                          (("pending+local", "pending/crash+local") if kpending_local else ())
                          if args.pending else ("check",))]
    for b, entries, mid, local, call in cross:
        d_hdr, d_ev = d_hdrs[mid], d_evs.get(mid, next(iter(d_evs.values())))
        budget = default if b == "default" else int(b)
        ctx.set_param("table_budget", budget)
        # (the keyed path's memo has its own knob; each knob is set for its own path alone)
        ctx.set_param("table_memo", 0 if mid == 5 else entries)
        ctx.set_param("ktable_memo", entries if mid == 5 and call == "check" else 0)
        ctx.set_param("ktable_local", local)
        # (the pending call's memo is its own knob too: "table_memo" does not reach it)
        ctx.set_param("pending_memo", entries if call.startswith("pending") and mid != 5 else 0)
        klocal = call.endswith("+local")    # the keyed pending call's own local mode
        call = call.split("+")[0]
        if kpending_local:
            ctx.set_param("kpending_local", int(klocal))
        ms = []
        for k in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if call == "explain":
                ctx.explain_device(mid, d_hdr.data_ptr(), n, d_ev.data_ptr(), n_events, d_st.data_ptr(),
                                   d_path.data_ptr(), d_rec.data_ptr(), d_nd.data_ptr(), d_tot.data_ptr(),
                                   max_nodes=args.max_nodes, stream=stream)
            elif call.startswith("pending"):
                hp, ep, ne = ((d_hdr_c, d_ev_c, n_events_c) if call == "pending/crash" else (d_hdr, d_ev, n_events))
                if mid == 5:
                    ctx.check_kpending_device(hp.data_ptr(), n, ep.data_ptr(), ne, d_st.data_ptr(), d_nd.data_ptr(),
                                              None, d_tot.data_ptr(), max_nodes=args.max_nodes, stream=stream)
                else:
                    ctx.check_pending_device(mid, hp.data_ptr(), n, ep.data_ptr(), ne, d_st.data_ptr(),
                                             d_nd.data_ptr(), None, d_tot.data_ptr(), max_nodes=args.max_nodes,
                                             stream=stream)
            else:
                ctx.check_device(mid, d_hdr.data_ptr(), n, d_ev.data_ptr(), n_events, d_st.data_ptr(),
                                 d_nd.data_ptr(), None, d_tot.data_ptr(), max_nodes=args.max_nodes, stream=stream)
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        tot = d_tot.cpu().numpy()
        med = statistics.median(ms)
        print(json.dumps({
            "model_id": mid, "call": call.split("/")[0],
            **({"batch": "crash 0.3" if call == "pending/crash" else "complete"} if args.pending else {}),
            "workload": what,
            "table_budget": budget, "is_default": budget == default, "table_memo": entries,
            "memo_knob": "ktable_memo" if mid == 5 else "table_memo", "table_memo_hits": ctx.table_memo_hits(), "calls": args.calls,
            **({"pending_memo": entries, "pending_memo_hits": ctx.pending_memo_hits()}
               if call.startswith("pending") and mid != 5 else {}),
            "ktable_local": local, "ktable_local_last": ctx.ktable_local_last() if mid == 5 else 0,
            **({"kpending_local": int(klocal), "kpending_local_last": ctx.kpending_local_last()}
               if kpending_local and call.startswith("pending") else {}),
            "ms_per_call_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "histories_per_s": round(n / med * 1e3), "nodes_per_s": round(int(tot[7]) / med * 1e3),
            "nodes_per_call": int(tot[7]), "pass2_histories": ctx.table_pass2(),
            "pass2_share": round(ctx.table_pass2() / n, 5),
            "lin": int(tot[1]), "nonlin": int(tot[2]), "budget": int(tot[5]),
            "max_nodes": args.max_nodes}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
