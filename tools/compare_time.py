#!/usr/bin/env python3
"""Development timing (not part of the product): pg_freq_compare next to its
numpy specification host.freq_compare at two shapes - the frequency table of
C3 batch A (-c 2, `-a cc -w 4`, one genome per record: G = 100) where pg_freq
left it on the device, over `-p 100`'s orders, and a synthetic table of
--labels labels x --genomes genomes at --density with 100 orders, uploaded
from the host.  Every call is synchronous (it returns after its last kernel),
so each is bracketed on the host with perf_counter: one warm-up, then --reps
calls; median and range.  The two must give the same arrays.  Prints one JSON
line per shape; writes nothing.

Per-kernel split: run it under `rocprofv3 --kernel-trace --stats -- python
tools/compare_time.py --reps 2 --host-reps 0` and read the k_cmp_* rows.
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
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)} if ms else None


def clock(f):
    t = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--orders", type=int, default=100)
    ap.add_argument("--input", default="c3a", help="a tests/scale_util.py input name ('' skips the shape)")
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--labels", type=int, default=1_000_000, help="0 skips the synthetic shape")
    ap.add_argument("--density", type=float, default=0.4)
    args = ap.parse_args()
    import numpy as np
    from pangenome_amd import _lib, host
    ctx = _lib.Context(27, 0)

    def measure(res, G, orders, bits, on_device):
        """bits: the host table; on_device: the device call takes the context's own table"""
        call = (lambda: ctx.freq_compare(orders)) if on_device else \
            (lambda: ctx.freq_compare(orders, bits=bits, n_groups=G))
        call()                                           # warm-up (buffers)
        dev = [clock(call) for _ in range(args.reps)]
        shared, (pan, core) = ctx.freq_shared(), ctx.freq_curves()
        got = []
        hst = [clock(lambda: got.append(host.freq_compare(bits, G, orders))) for _ in range(args.host_reps)]
        res.update(n_labels=int(bits.shape[0]), n_genomes=G, n_orders=int(orders.shape[0]),
                   bits_from="device table" if on_device else "host", pg_freq_compare_ms=stat(dev),
                   host_freq_compare_ms=stat(hst), pan_last=int(pan[0, -1]), core_last=int(core[0, -1]),
                   same=all(np.array_equal(a, b) for a, b in zip((shared, pan, core), got[0])) if got else None)
        print(json.dumps(res), flush=True)

    if args.input:
        from scale_util import make_input
        fasta = np.frombuffer(make_input(args.input), np.uint8)
        ctx.build_host(fasta, True)
        ctx.build_rdbg()
        ctx.edges_count(None, False)
        ctx.cluster_cc(None, None, 4)
        ctx.rows_count(None, False)
        R = ctx.n_records
        ctx.freq(np.arange(R, dtype=np.int32), R)
        measure({"shape": "%s -a cc -w 4 -g record" % args.input}, R, host.compare_orders(R, args.orders),
                ctx.freq_table()["bits"], True)
    if args.labels:
        G, n = args.genomes, args.labels
        rng = np.random.default_rng(1)
        bits = np.zeros((n, (G + 63) // 64), np.uint64)
        cut = int(round(256 * args.density))
        for lo in range(0, n, 1 << 16):
            hi = min(lo + (1 << 16), n)
            m = np.zeros((hi - lo, bits.shape[1] * 64), np.uint8)
            m[:, :G] = rng.integers(0, 256, (hi - lo, G), dtype=np.uint8) < cut
            bits[lo:hi] = np.packbits(m, axis=1, bitorder="little").view(np.uint64)
        measure({"shape": "synthetic, density %.2f" % (cut / 256)}, G, host.compare_orders(G, args.orders), bits, False)


if __name__ == "__main__":
    main()
