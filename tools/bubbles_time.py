"""tools/bubbles_time.py [genomes] [out.json]: pg_region_bubbles + its text at min_genomes = genomes / 2 and = genomes
beside pg_region_sites + its text on the rows of the C3-shaped run (synth.pangenome at the bench's C3 parameters,
-c 3 -a cc -w 4), same process: warm-up, repeated, median, and every round.  Host clock around calls that end in a
stream synchronise.  pg_region_sites is the yardstick: pg_sites.hip is what it was before pg_bubbles.hip."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pangenome_amd import synth                           # noqa: E402
from pangenome_amd._lib import Context                    # noqa: E402

genomes = int(sys.argv[1]) if len(sys.argv) > 1 else 100
t0 = time.time()
fa = synth.pangenome(genomes, 5_000_000, snp=1e-3, indel=1e-4)
buf = np.frombuffer(fa, np.uint8)
print("synth %.1f s, %d bytes" % (time.time() - t0, buf.shape[0]), flush=True)
ctx = Context(27, 0)
ctx.parse_host(buf)
ctx.build_dbg(None, 0, True)
ctx.build_rdbg()
ctx.edges_count(None, True)
ctx.cluster_cc(None, None, 4)
n_rows = ctx.rows_count(None, True)
R = len(ctx.records()["hdr_start"])
grp = np.arange(R, dtype=np.int32)
print("rows %d records %d (%.1f s so far)" % (n_rows, R, time.time() - t0), flush=True)


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


out = {"rows": int(n_rows), "records": R, "ms": {}}
steps = {"region_sites": lambda: ctx.region_sites(grp, R), "region_sites_text": ctx.region_sites_text}
for m in (max(1, R // 2), R):
    steps["region_bubbles_m%d" % m] = lambda m=m: ctx.region_bubbles(grp, R, m)
    steps["region_bubbles_m%d_text" % m] = ctx.region_bubbles_text
samples = {k: [] for k in steps}
for it in range(2 + 7):                                   # 2 warm-up rounds, 7 timed, the steps alternating
    for k, f in steps.items():
        ms, r = timed(f)
        if it >= 2:
            samples[k].append(ms)
        if it == 0:
            out[k + "_result"] = list(r) if isinstance(r, tuple) else len(r)
            if k.startswith("region_bubbles") and not k.endswith("_text"):
                al = ctx.region_bubbles_alleles()
                out[k + "_inner"] = {"labels": int(al["allele_regions"].sum()),
                                     "longest": int(al["allele_regions"].max()) if len(al["allele_regions"]) else 0,
                                     "alleles_2_regions": int((al["allele_regions"] >= 2).sum())}
for k, v in samples.items():
    out["ms"][k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                    "rounds": [round(x, 3) for x in v]}
ms = out["ms"]
for k in steps:
    if k.startswith("region_bubbles") and not k.endswith("_text"):
        out[k + "_over_sites"] = round(ms[k]["median"] / ms["region_sites"]["median"], 2)
out["device_bytes_peak"] = int(ctx.lib.pg_device_bytes(1))
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
ctx.close()
