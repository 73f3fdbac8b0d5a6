"""Inputs and checks of test_gpu_cover_geo.py: small pangenome-shaped records
around the sizes at which the coverage pass's per-group geometry (k_tiles'
GroupGeo descriptors) changes shape."""
import json
import os

import numpy as np

from pangenome_amd import synth

TILE = 4096                       # windows per coverage tile (pg_dbg.hip)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cover_geo", "identical.json")

# (records, length) of the inputs whose followers are exact copies of the lead
IDENTICAL = [(2, 4095), (2, 2 * TILE + 5), (5, TILE), (5, TILE + 27), (9, 2 * TILE + 5), (9, 3 * TILE - 1)]


def drifting(lengths, seed, snp=2e-3, indel=1e-3):
    """One record per length: variants of one base genome with indels dense
    enough that tiles drift against the references, cut to the length."""
    base = synth.base_genome(max(lengths) + max(lengths) // 8 + 512, seed)
    out = []
    for i, n in enumerate(lengths):
        v = synth.variant(base, i, snp, indel, seed)
        assert v.shape[0] >= n, (v.shape[0], n)
        out.append(synth.ACGT[v[:n]].copy())
    return out


def copies(n_rec, length, seed):
    """n_rec records, all the same random sequence."""
    seq = synth.ACGT[synth.base_genome(length, seed)]
    return [seq.copy() for _ in range(n_rec)]


def fasta_of(seqs, width=61):
    parts = []
    for i, s in enumerate(seqs):
        b = s.tobytes()
        parts.append(b">r%d\n" % i + b"".join(b[j:j + width] + b"\n" for j in range(0, len(b), width)))
    return b"".join(parts)


def check(ctx, ref, what=""):
    """The context's dBG (sorted keys and masks) and rdBG keys are the oracle's."""
    keys, masks = ctx.dbg()
    rk, rm = ref.dbg()
    assert np.array_equal(keys, rk) and np.array_equal(masks, rm), what
    assert np.array_equal(ctx.rdbg(), ref.rdbg()), what


def identical_stats(n_rec, length, k=27):
    """(n_records_a, n_work_items) of a build of copies(n_rec, length).  The
    last member's lanes read a few packed words and exception bytes past the
    end of the stream, so in device memory recycled from earlier builds of the
    process the counts move by a few segments (before the descriptors as
    well); new buffers are zero-filled for this build, as in a fresh process."""
    from pangenome_amd._lib import Context, PG_TUNE_POISON
    ctx = Context(k)
    try:
        ctx.tune(PG_TUNE_POISON, 0)
        ctx.set_fasta(fasta_of(copies(n_rec, length, 900 + n_rec)))
        ctx.parse()
        st = ctx.build(None, 0, True)
        return int(st.n_records_a), int(st.n_work_items)
    finally:
        ctx.tune(PG_TUNE_POISON, -1)
        ctx.close()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
