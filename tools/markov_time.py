#!/usr/bin/env python3
"""Development timing (not part of the product): pg_cluster_markov at the
command line's settings (-w 1, -I 1.5, select 64, 200 iterations at most) on
C3 batch A's device-resident edge table (-c 2), and pg_cluster_cc at W = 1 on
the same edges in the same process as the yardstick.  The calls are
synchronous, so each is bracketed on the host with perf_counter: one warm-up,
then the median of --reps runs.  A call with max_iter = 0 (node ids, weights,
initial matrix, components, text) gives the part that is not iterations.
Prints one JSON line and writes it to --out (profiles/markov_time_c3.json).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "markov_time_c3.json"))
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

    res = {"input": args.input, "n_edges": int(n_edges), "reps": args.reps, "min_weight": 1, "inflation2": 3,
           "select": host.MK_SELECT, "max_iter": host.MK_MAX_ITER}
    out = {}
    res["cluster_cc_w1_ms"], res["cluster_cc_w1_all"] = timed(lambda: out.update(cc=ctx.cluster_cc(None, None, 1)))
    res["cluster_cc_w1_clusters"] = int(out["cc"][0])
    res["markov_setup_ms"], res["markov_setup_all"] = timed(
        lambda: ctx.cluster_markov(None, None, 1, 3, host.MK_SELECT, 0))
    res["markov_ms"], res["markov_all"] = timed(
        lambda: out.update(mk=ctx.cluster_markov(None, None, 1, 3, host.MK_SELECT, host.MK_MAX_ITER)))
    n_clusters, n_nodes, n_iter, chaos = out["mk"]
    nu, _, cols_wave, cols_mid, cols_block = ctx.cluster_markov_stats()
    lines = ctx.labels()[2]
    res.update(n_nodes=int(n_nodes), iterations=int(n_iter), chaos=int(chaos), clusters=int(n_clusters),
               largest=int(np.bincount(lines).max()) if len(lines) else 0,
               ms_per_iteration=round((res["markov_ms"] - res["markov_setup_ms"]) / max(1, n_iter), 3),
               columns_wave_class=int(cols_wave), columns_mid_class=int(cols_mid), columns_block_class=int(cols_block),
               share_wave_class=round(cols_wave / max(1, cols_wave + cols_mid + cols_block), 6),
               share_mid_class=round(cols_mid / max(1, cols_wave + cols_mid + cols_block), 6),
               share_block_class=round(cols_block / max(1, cols_wave + cols_mid + cols_block), 6))
    text = json.dumps(res)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
