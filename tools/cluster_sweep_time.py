#!/usr/bin/env python3
"""Development timing (not part of the product): pg_cluster_sweep on C3 batch
A's device-resident edge table (-c 2) over host.sweep_thresholds(max_weight),
beside the same number of pg_cluster_cc calls, one per threshold: how the
figures were had before the sweep.  Both are synchronous (they return after
their last kernel), so each is bracketed on the host with perf_counter: one
warm-up, then the median of --reps runs.  The curve of both is compared
(clusters per threshold).  Prints one JSON line; writes nothing.

Per-kernel split: run it under `rocprofv3 --kernel-trace --stats -- python
tools/cluster_sweep_time.py --reps 2` and read the k_sw_* / k_cc_* / rocprim rows.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--input", default="c3a", help="a tests/scale_util.py input name")
    args = ap.parse_args()
    import numpy as np
    from scale_util import make_input
    from pangenome_amd import host
    from pangenome_amd._lib import Context
    fasta = np.frombuffer(make_input(args.input), np.uint8)
    ctx = Context(27, 0)
    ctx.build_host(fasta, True)
    ctx.build_rdbg()
    n_edges = ctx.edges_count(None, False)

    def timed(f):
        f()                                            # warm-up (buffers, rocPRIM scratch)
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            f()
            ms.append(1e3 * (time.perf_counter() - t))
        return round(statistics.median(ms), 3), [round(x, 3) for x in ms]

    res = {"input": args.input, "n_edges": int(n_edges), "reps": args.reps}
    res["cluster_weights_ms"], res["cluster_weights_all"] = timed(ctx.cluster_weights)
    n_nodes, max_weight = ctx.cluster_weights()
    thr = host.sweep_thresholds(max_weight)
    res.update(n_nodes=int(n_nodes), max_weight=int(max_weight), n_thr=len(thr))
    out = {}
    res["cluster_sweep_ms"], res["cluster_sweep_all"] = timed(lambda: out.update(t=ctx.cluster_sweep(thr)))
    table = {k: [int(x) for x in v] for k, v in out["t"].items()}
    res["table"] = table
    res["auto"] = host.sweep_choice(out["t"])

    def one_by_one():
        out["cc"] = [ctx.cluster_cc(None, None, w)[0] for w in thr]
    res["cluster_cc_each_ms"], res["cluster_cc_each_all"] = timed(one_by_one)
    assert out["cc"] == table["clusters"], (out["cc"], table["clusters"])
    res["cluster_cc_one_ms"] = round(res["cluster_cc_each_ms"] / len(thr), 3)
    res["sweep_over_one_cc"] = round(res["cluster_sweep_ms"] / res["cluster_cc_one_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
