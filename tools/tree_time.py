#!/usr/bin/env python3
"""Development timing (not part of the product): pg_tree_nj on random Hamming
matrices (--labels labels, each in a genome with probability 0.4) of --sizes
leaves, uploaded from the host.  Per size one warm-up, then --reps calls:
pg_tree_time's HIP-event span over the joins (median, range, every sample),
the host-clock bracket of the whole call, cells = the sum of m^2 over the
joins and 8 x cells / the median as bytes per second (the arg-min of a dense
m x m matrix; the kernels read less, the upper triangle of an uncompacted
n x n).  --host-size: host.tree_nj's wall time at that size on the same
machine, and whether the device gives the same tables.  Prints one JSON line
per size; writes nothing.
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

HBM_PEAK = 8.0e12                  # bytes per second, the MI355X's HBM3E (6.29e12 measured by a float4 copy)


def stat(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
            "all": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--labels", type=int, default=4000)
    ap.add_argument("--host-size", type=int, default=1024, help="0 skips host.tree_nj")
    args = ap.parse_args()
    import numpy as np
    from pangenome_amd import _lib, host
    from tree_util import hamming
    ctx = _lib.Context(27, 0)
    for n in args.sizes:
        d = hamming(n, labels=args.labels, seed=5)
        ctx.tree_nj(d)                                       # warm-up (code objects, buffers)
        ev, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            ctx.tree_nj(d)
            wall.append(1e3 * (time.perf_counter() - t))
            ms, cells = ctx.tree_time()
            ev.append(ms)
        med = statistics.median(ev)
        res = {"n": n, "labels": args.labels, "joins": max(n - 3, 0), "cells": cells, "pg_tree_time_ms": stat(ev),
               "pg_tree_nj_wall_ms": stat(wall), "us_per_join": round(1e3 * med / max(n - 3, 1), 3),
               "argmin_bytes_per_s": round(8 * cells / (med * 1e-3)), "hbm_peak_bytes_per_s": HBM_PEAK,
               "share_of_hbm_peak": round(8 * cells / (med * 1e-3) / HBM_PEAK, 4)}
        if n == args.host_size:
            t = time.perf_counter()
            joins, root = host.tree_nj(d)
            res["host_tree_nj_ms"] = round(1e3 * (time.perf_counter() - t), 1)
            got, (child, ln) = ctx.tree_joins(), ctx.tree_root()
            res["same"] = bool(all(np.array_equal(got[k], joins[k]) for k in joins) and
                               np.array_equal(child, root[0]) and np.array_equal(ln, root[1]))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
