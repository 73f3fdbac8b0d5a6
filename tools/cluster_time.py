#!/usr/bin/env python3
"""Development timing (not part of the product): pg_cluster_cc on C3 batch
A's device-resident edge table (-c 2) against pg_labels_from_edges on the
same table, the step the `-a cc` path replaces (it does the same node sorts).
Both calls are synchronous (they return after their last kernel), so each is
bracketed on the host with perf_counter: one warm-up, then the median of
--reps runs.  Prints one JSON line; writes nothing.

Per-kernel split: run it under `rocprofv3 --kernel-trace --stats -- python
tools/cluster_time.py --reps 2` and read the k_cc_* / k_text_*<MclLine> / rocprim rows.
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
    ap.add_argument("-w", type=int, nargs="*", default=[1, 4])
    args = ap.parse_args()
    import numpy as np
    from scale_util import make_input
    from pangenome_amd._lib import Context
    fasta = np.frombuffer(make_input(args.input), np.uint8)
    ctx = Context(27, 0)
    ctx.build_host(fasta, True)
    ctx.build_rdbg()
    n_edges = ctx.edges_count(None, False)
    z = np.zeros(0, np.int64)

    def timed(f):
        f()                                            # warm-up (buffers, rocPRIM scratch)
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            f()
            ms.append(1e3 * (time.perf_counter() - t))
        return round(statistics.median(ms), 3), [round(x, 3) for x in ms]

    res = {"input": args.input, "n_edges": int(n_edges), "reps": args.reps}
    res["labels_from_edges_ms"], res["labels_from_edges_all"] = timed(lambda: ctx.labels_from_edges(None, z, z, z, 0))
    res["n_nodes"] = int(ctx.n_labels)
    for w in args.w:
        out = {}
        med, allms = timed(lambda: out.update(r=ctx.cluster_cc(None, None, w)))
        res["cluster_cc_w%d_ms" % w], res["cluster_cc_w%d_all" % w] = med, allms
        res["cluster_cc_w%d_clusters" % w] = int(out["r"][0])
        assert out["r"][1] == res["n_nodes"]
        t = time.perf_counter()
        nbytes = len(ctx.clusters_text())
        res["clusters_text_w%d_ms" % w] = round(1e3 * (time.perf_counter() - t), 3)
        res["mcl_bytes_w%d" % w] = nbytes
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
