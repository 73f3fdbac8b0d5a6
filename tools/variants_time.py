#!/usr/bin/env python3
"""Development timing (not part of the product): the decoder kernel inside
pg_region_variants next to the one inside pg_region_seqs, on a synthetic input
on which both decode exactly the same letters in the same process.

The input: --records records of --bases random bases, half of them genome 0
and half genome 1.  Genome 0 carries --alleles segments, four per site, each
with an inner label of its own and a span of 0 .. --max-len bases (both
strands, every alignment); genome 1 joins every site's flanks directly and is
the reference.  The flank rows have length 0, so pg_region_seqs' longest row
per label is the inner row: its letters are the alleles' letters, one for one.

Both kernels are timed by the library with HIP events on its stream
(pg_region_seqs_time, pg_region_variants_time); the byte model is the same,
0.25 bytes read and 1 written per base.  One warm-up of each, then --reps
rounds alternating the two calls; median, range and every round.  The two text
calls (the allele FASTA and the VCF body, each ending in a stream synchronise)
and the whole pg_region_variants call are bracketed on the host.

--seqs-only: pg_region_seqs alone - what a tree without pg_region_variants
can run, so that the same file times the decoder before and after its move
into the shared header.  Prints one JSON line; with --out, writes it there.
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
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
            "rounds": [round(x, 4) for x in ms]}


def make_input(np, n_records, n_bases, n_alleles, max_len, seed):
    """(fasta bytes, rows [n, 5], rec_group)."""
    rng = np.random.default_rng(seed)
    half = n_records // 2
    recs = []
    for r in range(n_records):
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_bases)]
        lines = np.concatenate([seq.reshape(-1, 100), np.full((n_bases // 100, 1), 10, np.uint8)], axis=1)
        recs.append(b">r%d\n" % r + lines.tobytes())
    t = np.arange(n_alleles, dtype=np.int64)
    site, rec, fw = t // 4, t % half, t % 2 == 1
    length = rng.integers(0, max_len + 1, n_alleles)
    p = 1 + rng.integers(0, n_bases - max_len - 2, n_alleles)
    q = p + length
    a, c, x = 10 + 2 * site, 11 + 2 * site, 10 + 2 * (n_alleles // 4 + 1) + t
    one, zero = np.ones_like(t), np.zeros_like(t)
    # per allele: its a row, its inner row, its c row and an unused row that ends the run
    quad = np.stack([np.stack([rec, np.where(fw, p, q), np.where(fw, p, q), np.where(fw, 1, -1), a], axis=1),
                     np.stack([rec, np.where(fw, p, q), np.where(fw, q, p), np.where(fw, 1, -1), x], axis=1),
                     np.stack([rec, np.where(fw, q, p), np.where(fw, q, p), np.where(fw, 1, -1), c], axis=1),
                     np.stack([zero, zero, zero, one, -one], axis=1)], axis=1).reshape(-1, 5)
    s = np.arange(n_alleles // 4, dtype=np.int64)
    at = 1 + (s * 7919) % (n_bases - 2)
    rs = half + s % (n_records - half)
    one, zero = np.ones_like(s), np.zeros_like(s)
    ref = np.stack([np.stack([rs, at, at, one, 10 + 2 * s], axis=1), np.stack([rs, at, at, one, 11 + 2 * s], axis=1),
                    np.stack([zero, zero, zero, one, -one], axis=1)], axis=1).reshape(-1, 5)
    rec_group = (np.arange(n_records) >= half).astype(np.int32)
    return b"".join(recs), np.ascontiguousarray(np.concatenate([quad, ref])), rec_group


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--bases", type=int, default=4_000_000)
    ap.add_argument("--alleles", type=int, default=200_000)
    ap.add_argument("--max-len", type=int, default=600)
    ap.add_argument("--seqs-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    from pangenome_amd import _lib
    fasta, rows, rec_group = make_input(np, args.records, args.bases, args.alleles, args.max_len, 2026)
    ctx = _lib.Context(27, 0)
    ctx.parse_host(np.frombuffer(fasta, np.uint8))
    names = [b"r%d" % r for r in range(args.records)]
    res = {"records": args.records, "bases_per_record": args.bases, "rows": int(rows.shape[0]), "reps": args.reps,
           "bytes_per_base": 1.25}

    def clock(f):
        t = time.perf_counter()
        r = f()
        return 1e3 * (time.perf_counter() - t), r

    def seqs():
        n_regions, n_bases, _ = ctx.region_seqs(rec_group, 2, rows=rows)
        ms, chunks = ctx.region_seqs_time()
        return ms, n_bases, chunks

    def variants():
        _, n_bases, _, _ = ctx.region_variants(rec_group, 2, None, rows=rows)
        ms, chunks = ctx.region_variants_time()
        return ms, n_bases, chunks
    steps = {"region_seqs": seqs}
    if not args.seqs_only:
        na = ctx.region_bubbles(rec_group, 2, 2, rows=rows)[3]
        res["alleles"] = int(na)
        steps["region_variants"] = variants
    samples = {k: [] for k in steps}
    for it in range(1 + args.reps):
        for k, f in steps.items():
            ms, n_bases, chunks = f()
            if it:
                samples[k].append(ms)
            else:
                res[k + "_letters"], res[k + "_chunks"] = int(n_bases), int(chunks)
    for k, v in samples.items():
        res[k + "_decode_ms"] = stat(v)
        res[k + "_letters_per_s"] = round(res[k + "_letters"] / (statistics.median(v) * 1e-3))
        res[k + "_GB_per_s"] = round(1.25 * res[k + "_letters"] / (statistics.median(v) * 1e-3) / 1e9, 1)
    if not args.seqs_only:
        res["equal_letters"] = res["region_seqs_letters"] == res["region_variants_letters"]
        whole = {"region_variants_no_ref": lambda: ctx.region_variants(rec_group, 2, None, rows=rows),
                 "region_variants_ref": lambda: ctx.region_variants(rec_group, 2, 1, rows=rows),
                 "alleles_fasta_text": lambda: len(ctx.region_alleles_fasta_text(names)),
                 "vcf_text": lambda: len(ctx.region_vcf_text(names))}
        calls = {k: [] for k in whole}
        for it in range(1 + min(args.reps, 7)):
            for k, f in whole.items():
                ms, r = clock(f)
                if it:
                    calls[k].append(ms)
                else:
                    res[k + "_result"] = list(r) if isinstance(r, tuple) else int(r)
        res["host_clock_ms"] = {k: stat(v) for k, v in calls.items()}
        res["decode_ms_with_ref"] = round(ctx.region_variants_time()[0], 4)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
