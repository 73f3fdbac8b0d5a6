#!/usr/bin/env python3
"""Development timing (not part of the product): pg_rdbg_export on the
HBM-resident C3 graph (batch c3a, 100 x 5 Mbp, k = 27) in both forms of
PG_TUNE_RDBG_KEYS - 0: the build counts the members and the export sweeps the
table for their keys; 1: the build writes the keys and the export gathers them.

    python tools/rdbg_export_time.py [--calls 9]

Per form: one build, one warm-up export, then the median (min-max) of --calls
exports, each the whole call (sweep or gather, device sort, copy back); the
keys of the two forms are compared.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--genomes", type=int, default=100)
    args = ap.parse_args()
    import torch
    from pangenome_amd import _lib, kmer, synth
    tmp = tempfile.mkdtemp(prefix="rdbg_export_")
    p = os.path.join(tmp, "c3a.fa")
    synth.write_pangenome(p, args.genomes, 5_000_000, first_index=0, workers=16)
    d = torch.from_numpy(np.array(kmer.seq2bytes(p))).to("cuda:0")
    os.unlink(p)
    os.rmdir(tmp)
    out, keys = {}, {}
    for form in (0, 1):
        ctx = _lib.Context(27, 0)
        ctx.tune(_lib.PG_TUNE_RDBG_KEYS, form)
        st = ctx.build_device(d.data_ptr(), d.numel(), True, keepalive=d)
        keys[form] = ctx.rdbg()
        ms = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.rdbg()
            ms.append(1e3 * (time.perf_counter() - t0))
        out["form%d" % form] = dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3),
                                    max_ms=round(max(ms), 3), n_rdbg=int(st.n_rdbg), buckets=int(st.table_capacity),
                                    calls_ms=[round(x, 3) for x in ms])
        ctx.close()
    out["same_keys"] = bool(np.array_equal(keys[0], keys[1]))
    print(json.dumps({"rdbg_export_time": out}))


if __name__ == "__main__":
    main()
