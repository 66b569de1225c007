"""The deep keyed histories of tests/ktablememo.py (KDEEP), one call each
through the host entry with the keyed path's state memo ("ktable_memo",
csrc/ktable.hip): wall ms of the call, the memo's hits, and
the verdict and node count against the known answer.  One JSON line per row
and memo size; the first call of a size (which allocates and clears the
tables) is made on a short history and not reported.

    python tools/ktable_memo_rows.py [--memo 4096] [--repeat 3] [--time-limit-ms 5000]
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("quickcheck-state-machine-distributed_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import ktablememo as km  # noqa: E402
import tablegen as tg  # noqa: E402
from linearise_lists import ModelError as OracleModelError  # noqa: E402
from qsmd import codec, device  # noqa: E402
from qsmd.models import KeyedTableModel, TableModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--memo", default="4096")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--time-limit-ms", type=int, default=5000)
    args = ap.parse_args()
    ctx = device.Context(0, time_limit_ms=args.time_limit_ms)
    models, warmed = {}, set()
    for name, c in (("register", tg.REGISTER), ("lock", tg.LOCK)):
        t = TableModel.from_closures(c["transition"], c["postcondition"], c["init"], c["invs"], c["resps"],
                                     raises=OracleModelError)
        models[name] = KeyedTableModel(t, 8)
    for entries in (int(e) for e in args.memo.split(",")):
        ctx.set_param("ktable_memo", entries)
        for name in sorted(km.KDEEP):
            comp, K, hist, events, status, nodes, states = km.KDEEP[name]
            m = models[comp]
            if ctx.keyed_table is not m:
                ctx.set_keyed_table(m)
            if (entries, comp) not in warmed:
                warmed.add((entries, comp))
                warm = codec.encode(m, [km.KDEEP["klin_deep_2_3_2" if comp == "register" else "klock_deep_8_4_4"][2]])
                ctx.check_arrays(5, warm.hdr, warm.events, None, device.QSMD_FLAG_EXHAUSTIVE, 0)
            batch = codec.encode(m, [hist])
            ms = []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                st, nd, _, _ = ctx.check_arrays(5, batch.hdr, batch.events, None, device.QSMD_FLAG_EXHAUSTIVE, 0)
                ms.append((time.perf_counter() - t0) * 1e3)
            got = (codec.STATUS_NAMES[int(st[0])], int(nd[0]))
            print(json.dumps({"row": name, "keys": K, "events": events, "ktable_memo": entries,
                              "status": got[0], "nodes": got[1], "as_known": got == (status, nodes),
                              "distinct_states": states, "hits": ctx.table_memo_hits(),
                              "timed_out": bool(ctx.timed_out()),
                              "wall_ms": [round(x, 3) for x in ms], "wall_ms_min": round(min(ms), 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
