#!/usr/bin/env python3
"""Development timing (not part of the product): pg_kmer_colors on a synthetic
pangenome from synth (--genomes x --length bases at the C3 mutation model:
0.1 % SNP, 0.01 % indel; one genome per record), k = 27, both strands.  The
table is built once (pg_build_host); then one warm-up and --reps calls: the
whole call on the host clock and pg_kmer_colors_time's HIP-event spans (the
index and the tables, the colouring pass alone), the windows per second of the
colouring pass, then pg_kmer_compare over 3 orders the same way.  As a
yardstick for lookups without writes: pg_edges on the same input and table
(whole calls on the host clock: the walk's count and write passes, which make
the same lookups, plus its edge table).  Prints one JSON object; writes
nothing.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
            "all": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=100)
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    import numpy as np
    from pangenome_amd import _lib, host, synth
    G = args.genomes
    fa = np.frombuffer(synth.pangenome(G, args.length), np.uint8)
    ctx = _lib.Context(27, 0)
    st = ctx.build_host(fa, True)
    R = ctx.n_records
    assert R == G
    grp = np.arange(R, dtype=np.int32)
    counts = ctx.kmer_colors(grp, G, None, True)             # warm-up (code objects, buffers)
    wall, idx, col = [], [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        assert ctx.kmer_colors(grp, G, None, True) == counts
        wall.append(1e3 * (time.perf_counter() - t))
        a, b, _, nwin = ctx.kmer_colors_time()
        idx.append(a)
        col.append(b)
    orders = host.compare_orders(G, 3)
    ctx.kmer_compare(orders)
    cmp_wall, cmp_ev = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        ctx.kmer_compare(orders)
        cmp_wall.append(1e3 * (time.perf_counter() - t))
        cmp_ev.append(ctx.kmer_colors_time()[2])
    by_g = ctx.kmer_colors_spectrum()["kmers_by_g"]
    ctx.kmer_colors_drop()
    ctx.build_rdbg()
    ctx.edges_count(None, True)
    edges = []
    for _ in range(args.reps):
        t = time.perf_counter()
        n_edges = ctx.edges_count(None, True)
        edges.append(1e3 * (time.perf_counter() - t))
    med = statistics.median(col)
    print(json.dumps({
        "commit": args.commit, "where": "one MI355X", "input": "synth.pangenome(%d, %d): %d x %.1f Mbp, 0.1%% SNP, 0.01%% indel"
        % (G, args.length, G, args.length / 1e6), "k": 27, "rc0": 1, "genomes": G, "words_per_key": (G + 63) // 64,
        "n_bases": int(st.n_bases), "n_keys": counts[0], "n_windows": counts[1], "n_missing": counts[2],
        "n_uncoloured": counts[3], "keys_in_every_genome": int(by_g[G]), "keys_in_one_genome": int(by_g[1]),
        "layout": "key-major rows in the table's sweep order, brought into key order after the pass (the one form built)",
        "pg_kmer_colors_wall_ms": stat(wall), "ms_index": stat(idx), "ms_colour": stat(col),
        "windows_per_second_colour_pass": round(nwin / (med * 1e-3)),
        "pg_kmer_compare_3_orders_wall_ms": stat(cmp_wall), "ms_compare": stat(cmp_ev),
        "yardstick_pg_edges_wall_ms": stat(edges), "yardstick_n_edges": int(n_edges),
        "yardstick_note": "pg_edges whole call, rc1 = 1: count pass + write pass (each the same lookups as one colouring pass, "
                          "no writes to the keys) + the edge table", "reps": args.reps}))


if __name__ == "__main__":
    main()
