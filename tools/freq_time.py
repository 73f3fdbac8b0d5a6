#!/usr/bin/env python3
"""Development timing (not part of the product): pg_freq on C3 batch A's
device-resident rows (-c 2, one genome per record), next to pg_rows of the
same process - the pass that produces the data - at `-a cc -w 1` (one hot
label) and `-w 4` (many labels), and with that clustering's even labels
folded into one (a hot label between small ones, on the device like the
others).  The wave-aggregated accumulate pass and the
plain one (PG_TUNE_FREQ_FORM 0 / 1) alternate call by call on the same rows;
both must give the same text.  Every call is synchronous (it returns after
its last kernel), so each is bracketed on the host with perf_counter: one
warm-up per form, then --reps alternating rounds; median and range of each.
Prints one JSON line; writes nothing.

Per-kernel split: run it under `rocprofv3 --kernel-trace --stats -- python
tools/freq_time.py --reps 2` and read the k_fr_* and k_row_scan rows.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stat(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--input", default="c3a", help="a tests/scale_util.py input name")
    ap.add_argument("-w", type=int, nargs="*", default=[1, 4])
    args = ap.parse_args()
    import numpy as np
    from scale_util import make_input
    from pangenome_amd import _lib
    fasta = np.frombuffer(make_input(args.input), np.uint8)
    ctx = _lib.Context(27, 0)
    ctx.build_host(fasta, True)
    ctx.build_rdbg()
    n_edges = ctx.edges_count(None, False)
    R = ctx.n_records
    rec_group = np.arange(R, dtype=np.int32)
    res = {"input": args.input, "n_edges": int(n_edges), "n_records": int(R), "reps": args.reps}

    def clock(f):
        t = time.perf_counter()
        f()
        return 1e3 * (time.perf_counter() - t)
    def measure(extra):
        ctx.rows_count(None, False)                    # warm-up
        rows_ms = [clock(lambda: ctx.rows_count(None, False)) for _ in range(args.reps)]
        n_rows = ctx.rows_count(None, False)
        forms = {0: [], 1: []}
        sha = {}
        for form in (0, 1):                            # warm-up (buffers, rocPRIM scratch) and the result
            ctx.tune(_lib.PG_TUNE_FREQ_FORM, form)
            counts = ctx.freq(rec_group, R)
            sha[form] = hashlib.sha256(ctx.freq_text()).hexdigest()
        for _ in range(args.reps):
            for form in (0, 1):
                ctx.tune(_lib.PG_TUNE_FREQ_FORM, form)
                forms[form].append(clock(lambda: ctx.freq(rec_group, R)))
        ctx.tune(_lib.PG_TUNE_FREQ_FORM, 0)
        t = ctx.freq_table()
        return dict(extra, n_rows=int(n_rows), n_labels=int(counts[0]), n_used=int(counts[1]),
                    largest_label_rows=int(t["rows"].max()) if counts[0] else 0, pg_rows_ms=stat(rows_ms),
                    pg_freq_aggregated_ms=stat(forms[0]), pg_freq_plain_ms=stat(forms[1]),
                    same_text=sha[0] == sha[1], text_sha256=sha[0])
    for w in args.w:
        n_clusters, _ = ctx.cluster_cc(None, None, w)
        res["w%d" % w] = measure({"n_clusters": int(n_clusters)})
    # one hot label between small ones (a giant component at a middling weight
    # cut): the last clustering's even labels folded into label 0.  A row ends
    # where the label changes, so the hot label holds at most every other row.
    keys, vals, ids = ctx.labels()
    ctx.set_labels(keys, vals, np.where(ids % 2 == 0, 0, ids))
    res["hot"] = measure({"labels_folded": "even -> 0"})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
