#!/usr/bin/env python3
"""Development timing (not part of the product): pg_tree_bootstrap on a
synthetic presence table (--labels coin-flip rows over --genomes genomes,
uploaded from the host), --replicates replicates, three ways:
  default    PG_TUNE_BOOT_FORM 0: a workgroup per replicate
  form3      PG_TUNE_BOOT_FORM 3: pg_tree_nj's per-join launches per replicate
  yardstick  the route without pg_tree_bootstrap: the replicate matrices made
             on the host (host.tree_bootstrap's float64 products, timed once)
             and sent through pg_tree_nj one after another (timed --reps times)
Per way one warm-up, then --reps calls on the host clock around the whole call
(median, range, every sample); for the two forms also pg_tree_bootstrap_time's
HIP-event spans of the last call.  The forms' supports and joins are compared.
Prints one JSON line per size; --out also writes them to a file.
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


def stat(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
            "all": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="*", default=[100])
    ap.add_argument("--labels", type=int, default=100000)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--yardstick-genomes", type=int, nargs="*", default=[100], help="sizes at which the yardstick runs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    from pangenome_amd import _lib, host, synth
    from boot_util import coin_table, table_dist
    seed, R = synth.DEFAULT_SEED, args.replicates
    ctx = _lib.Context(27, 0)
    lines = []
    for G in args.genomes:
        bits = coin_table(args.labels, G, seed=5)
        d = table_dist(bits, G)
        ctx.tree_nj(d, G)
        res = {"genomes": G, "labels": args.labels, "replicates": R, "joins_per_tree": max(G - 3, 0),
               "command": " ".join(["python"] + sys.argv)}
        got = {}
        for name, form in (("default", 0), ("form3", 3)):
            ctx.tune(_lib.PG_TUNE_BOOT_FORM, form)
            ctx.tree_bootstrap(R, seed, bits=bits, n_groups=G)           # warm-up (code objects, buffers)
            wall = []
            for _ in range(args.reps):
                t = time.perf_counter()
                ctx.tree_bootstrap(R, seed, bits=bits, n_groups=G)
                wall.append(1e3 * (time.perf_counter() - t))
            ms_dist, ms_nj, ms_sup, cells = ctx.tree_bootstrap_time()
            ran, batches = ctx.tree_bootstrap_form()
            got[name] = (ctx.tree_support()[0], ctx.tree_bootstrap_joins())
            res[name] = {"form_ran": ran, "batches": batches, "wall_ms": stat(wall),
                         "event_ms": {"dist": round(ms_dist, 3), "nj": round(ms_nj, 3), "support": round(ms_sup, 3)},
                         "cells": cells}
        ctx.tune(_lib.PG_TUNE_BOOT_FORM, 0)
        res["forms_agree"] = bool(np.array_equal(got["default"][0], got["form3"][0]) and
                                  all(np.array_equal(a, b) for a, b in zip(got["default"][1], got["form3"][1])))
        if G in args.yardstick_genomes:
            t = time.perf_counter()
            mats = host.tree_bootstrap(bits, G, ctx.tree_joins(), R, seed, rep_dist=True)["rep_dist"]
            host_ms = 1e3 * (time.perf_counter() - t)                    # (includes the host's own trees)
            for m in mats[:2]:
                ctx.tree_nj(m, G)
            wall = []
            for _ in range(args.reps):
                t = time.perf_counter()
                for m in mats:
                    ctx.tree_nj(m, G)
                    ctx.tree_joins()
                wall.append(1e3 * (time.perf_counter() - t))
            res["yardstick"] = {"pg_tree_nj_loop_wall_ms": stat(wall),
                                "host_matrices_and_spec_ms_once": round(host_ms, 1)}
            ctx.tree_nj(d, G)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
