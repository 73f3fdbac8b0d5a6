"""tools/regionseq_time.py [bases]: the decoder kernel of pg_region_seqs on one region over a whole synthetic
record (synth.base_genome, default 2^28 bases), on the - strand and on the + strand, beside a device-to-device
copy of the same number of output bytes; same process, warm-up, the three alternating, median.  Kernel times
are HIP events (pg_region_seqs_time; torch events around the copy)."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pangenome_amd import synth                           # noqa: E402
from pangenome_amd._lib import Context                    # noqa: E402
import torch                                              # noqa: E402

L = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 28
letters = np.frombuffer(b"ACGT", np.uint8)[synth.base_genome(L)]
buf = np.concatenate([np.frombuffer(b">g0\n", np.uint8), letters, np.frombuffer(b"\n", np.uint8)])
ctx = Context(27, 0)
ctx.parse_host(buf)
assert ctx.records()["seq_len"].tolist() == [L]
grp = np.zeros(1, np.int32)
rows = {"reverse": np.array([[0, L, 0, -1, 0]], np.int64), "forward": np.array([[0, 0, L, 1, 0]], np.int64)}
src = torch.empty(L, dtype=torch.uint8, device="cuda")
dst = torch.empty(L, dtype=torch.uint8, device="cuda")
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def decode(which):
    assert ctx.region_seqs(grp, 1, rows=rows[which]) == (1, L, 0)
    ms, chunks = ctx.region_seqs_time()
    assert chunks == (L + 15) // 16
    return ms


def copy():
    ev[0].record()
    dst.copy_(src)
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


steps = {"reverse": lambda: decode("reverse"), "forward": lambda: decode("forward"), "copy": copy}
samples = {k: [] for k in steps}
for it in range(2 + 7):                                   # 2 warm-up rounds, 7 timed, the steps alternating
    for k, f in steps.items():
        ms = f()
        if it >= 2:
            samples[k].append(ms)
# the last decode was the forward one: its letters are the input's
assert ctx.region_seqs_bases() == letters.tobytes()
out = {"bases": L, "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                              "max": round(max(v), 4)} for k, v in samples.items()}}
decode_bytes = L + L / 4 + L / 16                         # 1 B written, 0.25 B of p2 and 1/16 B of e16 read per base
copy_bytes = 2 * L                                        # 1 B read and 1 B written per byte
out["decode_bytes"], out["copy_bytes"] = int(decode_bytes), copy_bytes
for k in ("reverse", "forward"):
    out[k + "_gbytes_per_s"] = round(decode_bytes / out["ms"][k]["median"] / 1e6, 1)
    out[k + "_output_rate_of_copy"] = round(out["ms"]["copy"]["median"] / out["ms"][k]["median"], 3)
out["copy_gbytes_per_s"] = round(copy_bytes / out["ms"]["copy"]["median"] / 1e6, 1)
print(json.dumps(out))
ctx.close()
