"""The table-model generator alone (csrc/tgen.hip, Context.gen_table_device).

Workload: 4 clients x 16 operations, linearisation points inside the window,
per-client pids, --n histories (default 1,048,576), from the register table
(model 3, tests/tablegen.py) and from the kv table (model 4,
tests/wtablegen.py).  Per model, one JSON line:

  device   --warmup + --calls launches, each timed by HIP events on the
           stream; the median ms per launch, histories/s, and the bytes the
           launch must write (256 B of events + 16 B of header + 1 flag byte a
           history) per second;
  fill     the same with a device fill of the events buffer in place of the
           launch: what plain stores of those bytes achieve on this box;
  host     qsmd.gen.generate_table with --threads threads (wall clock, median
           of --host-calls) and the host-to-device copy of its three arrays
           (pageable memory, wall clock with a device synchronisation): what a
           caller paid before the kernel existed.

--keyed K[,K...] adds, after the models' lines and in the same run, one line
per K: the register on K keys (model 5) through the keyed launch
(csrc/ktgen.hip, Context.gen_ktable_device), the host leg being
qsmd.gen.generate_ktable.  "over_model3" is its median over the model-3
register launch's of this run (when "register" is among --models).

    python tools/tgen_bench.py [--n 1048576] [--models register,kv] [--keyed 1,4,8] [--threads 16] [--p-bug 0.0]
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("quickcheck-state-machine-distributed_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import tablegen as tg  # noqa: E402
import wtablegen as wg  # noqa: E402
from qsmd import device, gen  # noqa: E402
from qsmd.models import KeyedTableModel, TableModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--models", default="register,kv")
    ap.add_argument("--keyed", default="", help="key counts for the keyed register lines, e.g. 1,4,8")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--p-bug", type=float, default=0.0)
    ap.add_argument("--lin", type=int, default=gen.LIN_IN_WINDOW)
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda:0")
    n, per = args.n, 32
    d_hdr = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    d_ev = torch.empty(n * per * 8, dtype=torch.uint8, device=dev)
    d_fl = torch.empty(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    out_bytes = n * (per * 8 + 16 + 1)

    def timed(fn):
        ms = []
        for k in range(args.warmup + args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    def register():
        c = tg.REGISTER
        return TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"])

    ctx = device.Context(0)
    sched = dict(n_clients=4, n_ops=16, prefix_ops=4, lin_policy=args.lin, pid_mode=gen.PID_PER_CLIENT,
                 p_bug=args.p_bug, seed=0x5EED)
    runs = [(name, 0) for name in args.models.split(",") if name]
    runs += [("register", int(k)) for k in args.keyed.split(",") if k]
    model3_ms = None
    for name, keys in runs:
        if keys:
            m = KeyedTableModel(register(), keys)
            ctx.set_keyed_table(m)
            p = gen.ktable_params(**sched)
            launch = lambda: ctx.gen_ktable_device(p, 0, n, d_hdr.data_ptr(), d_ev.data_ptr(),  # noqa: E731
                                                   d_fl.data_ptr(), stream=stream)
            host = lambda: gen.generate_ktable(p, m, 0, n, threads=args.threads)  # noqa: E731
        else:
            if name == "kv":
                m, wide = wg.wide_table("kv"), True
                ctx.set_wide_table(m)
            else:
                m, wide = register(), False
                ctx.set_table(m)
            p = gen.table_params(**sched)
            launch = lambda: ctx.gen_table_device(p, 0, n, d_hdr.data_ptr(), d_ev.data_ptr(),  # noqa: E731
                                                  d_fl.data_ptr(), stream=stream, wide=wide)
            host = lambda: gen.generate_table(p, m, 0, n, threads=args.threads)  # noqa: E731
        ms = timed(launch)
        fill = timed(lambda: d_ev.fill_(0xA5))
        host_s, copy_s = [], []
        for _ in range(args.host_calls):
            t0 = time.perf_counter()
            hdr, ev, fl = host()
            t1 = time.perf_counter()
            for a in (hdr, ev, fl):
                torch.from_numpy(a.view("uint8")).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host_s.append(t1 - t0)
            copy_s.append(t2 - t1)
        med, fmed = statistics.median(ms), statistics.median(fill)
        host_ms = statistics.median(host_s) * 1e3 if host_s else None      # --host-calls 0: the device alone
        copy_ms = statistics.median(copy_s) * 1e3 if copy_s else None
        if not keys and name == "register":
            model3_ms = med
        line = {
            "model": f"{name}^{keys}" if keys else name, "model_id": m.model_id, "n": n, "n_inv": len(m.invs),
            "n_states": len((m.component if keys else m).states),
            "workload": f"4x16 prefix 4, lin_policy {args.lin}, per-client pids, p_bug {args.p_bug}",
            "device_ms_median": round(med, 4), "device_ms_min": round(min(ms), 4), "device_ms_max": round(max(ms), 4),
            "histories_per_s": round(n / med * 1e3), "out_bytes": out_bytes,
            "out_GBps": round(out_bytes / med / 1e6, 1),
            "fill_ms_median": round(fmed, 4), "fill_GBps": round(n * per * 8 / fmed / 1e6, 1),
            "host_threads": args.threads, "host_gen_ms_median": host_ms and round(host_ms, 2),
            "h2d_ms_median": copy_ms and round(copy_ms, 2),
            "host_total_over_device": host_ms and round((host_ms + copy_ms) / med, 1),
        }
        if keys:
            line["keys"] = keys
            line["over_model3"] = model3_ms and round(med / model3_ms, 3)
        print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
