"""The rdBG's count and its keys, in both forms of PG_TUNE_RDBG_KEYS: 0 (the
default: the range pass counts the members, pg_rdbg_export sweeps the table
for their keys) and 1 (the range pass writes the keys as it counts them).

Every case compares ctx.rdbg() bit for bit with the CPU oracle's rdBG of the
same input (both sorted) and the build's n_rdbg with its length.  The base
input is tests/ksweep_util.py's: a 20 kbp lead, five followers and a tail of
records of 0 to k + 3 bases, which give the n<k sentinel and the short
records' own emission.

What each size is for:
  k = 27   2^25 buckets in 8192 partitions, 16 per persistent block: a lane's
           count carries across its block's partitions, and the export sweeps
           a nearly empty 0.5 GB table.
  k = 13   2^17 buckets in 32 partitions, fewer than blocks: the blocks
           without a partition report 0; second words are common.
  k = 13 at bucket shifts 1, 2 and 8: members in the LDS overflow set and the
           HBM overflow table (the set holds h + 1, the table's slots c + 1).
           At shift 8 (2^9 buckets for 34 k keys, 8 to a partition) the sets
           spill and stages B/C run again with more buckets, and the count
           must be the last run's alone.  (Shifts 2 and 3 leave this input's
           64 partitions within their 512 overflow slots: no re-run, measured.)
  k = 5    as many bucket bits as key bits and a 0-bit quotient, almost every
           key a member: the export's run reservation at high density.
  k = 4, 10 with repeats of ACGT and AACCGGTT spliced into the lead: keys
           that are their own reverse complement, whose two orientations both
           sit in field A.
"""
import ctypes as C

import numpy as np
import pytest

import ksweep_util as ku
from pangenome_amd import synth

pytestmark = pytest.mark.gpu

FORMS = (0, 1)
PG_ERANGE = -34
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _shared():
    """The inputs and the oracle's rdBGs, computed once and freed with the module."""
    yield
    _cache.clear()


def palindrome_fasta(k):
    """sweep_fasta(k) with runs of ACGT and of AACCGGTT spliced into the lead
    (every k-base window inside a run of a unit whose length divides k, or of
    ACGT at even k, is its own reverse complement)."""
    base = synth.base_genome(ku.GENOME, ku.SEED)
    code = {c: i for i, c in enumerate(b"ACGT")}
    acgt = np.array([code[c] for c in b"ACGT" * 16], np.uint8)
    aaccggtt = np.array([code[c] for c in b"AACCGGTT" * 8], np.uint8)
    lead = np.concatenate([base[:5000], acgt, base[5000:12345], aaccggtt, base[12345:], acgt[:37]])
    parts = [synth.to_fasta_lines(b"lead", lead, width=ku.WIDTH)]
    for i in range(ku.FOLLOWERS):
        parts.append(synth.to_fasta_lines(b"f%d" % i, synth.variant(base, i, snp=0.01, indel=1e-3, seed=ku.SEED),
                                          width=ku.WIDTH))
    return b"".join(parts) + ku._tail(k, ku.SEED)


INPUTS = {
    "sweep": ku.sweep_fasta,
    "palindromes": palindrome_fasta,
    "empty": lambda k: b"",
    "short": lambda k: b">s\n" + b"ACGTTGCA"[:max(0, k - 1)] + b"\n",
}


def fasta_of(name, k):
    if ("fasta", name, k) not in _cache:
        _cache["fasta", name, k] = INPUTS[name](k)
    return _cache["fasta", name, k]


def ref_of(oracle, name, k):
    """The oracle's sorted rdBG of input `name` at k and -c 2."""
    if ("ref", name, k) not in _cache:
        r = np.sort(oracle.OracleRun(fasta_of(name, k), k, 2).rdbg())
        r.setflags(write=False)
        _cache["ref", name, k] = r
    return _cache["ref", name, k]


def check(ctx, st, ref, what):
    got = ctx.rdbg()
    assert st.n_rdbg == ref.shape[0], (what, st.n_rdbg, ref.shape[0])
    assert got.dtype == np.uint64 and np.array_equal(got, ref), what


def context(k, form, shift=0):
    from pangenome_amd._lib import Context, PG_TUNE_BUCKET_SHIFT, PG_TUNE_RDBG_KEYS
    ctx = Context(k)
    ctx.tune(PG_TUNE_RDBG_KEYS, form)
    ctx.tune(PG_TUNE_BUCKET_SHIFT, shift)
    return ctx


def build(ctx, fasta):
    ctx.set_fasta(fasta)
    ctx.parse()
    return ctx.build(None, 0, True)


def is_own_rc(keys, k):
    """which base-5 keys of k ACGT digits (alpha: A0 G1 C2 T3) equal their reverse complement"""
    d = np.stack([(keys // np.uint64(5 ** j)) % np.uint64(5) for j in range(k)])
    return ((d < 4).all(axis=0)) & ((d + d[::-1] == 3).all(axis=0))


# ------------------------------------------------------------ the base input
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k,shift", [(27, 0), (13, 0), (13, 1), (13, 2), (13, 8), (5, 0)])
def test_base_input(oracle_mod, k, shift, form):
    ref = ref_of(oracle_mod, "sweep", k)
    ctx = context(k, form, shift)
    try:
        st = build(ctx, fasta_of("sweep", k))
        reruns = (int(st.build_flags) >> 8) & 255
        print("k=%d shift=%d form=%d: buckets %d n_dbg %d n_rdbg %d B/C re-runs %d"
              % (k, shift, form, st.table_capacity, st.n_dbg, st.n_rdbg, reruns))
        check(ctx, st, ref, (k, shift, form))
        if shift == 8:
            assert reruns >= 1                      # the LDS overflow set spilled: the count is the last run's
        if k == 5:
            assert ref.shape[0] > 9 * 4 ** k // 10  # dense: nearly every ACGT key is a member
    finally:
        ctx.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", (4, 10))
def test_palindromes(oracle_mod, k, form):
    ref = ref_of(oracle_mod, "palindromes", k)
    own = is_own_rc(ref[ref != ku.SENTINEL], k)
    assert own.any()                                # members that are their own reverse complement
    ctx = context(k, form)
    try:
        check(ctx, build(ctx, fasta_of("palindromes", k)), ref, (k, form))
    finally:
        ctx.close()


# ------------------------------------------------------------------ the paths
@pytest.mark.parametrize("form", FORMS)
def test_dump_load_build_rdbg(oracle_mod, form):
    """The graph staged from another context's dump (pg_dbg_dump, pg_dbg_load)
    and built with every record unflagged, then pg_build_rdbg."""
    k = 13
    fasta, ref = fasta_of("sweep", k), ref_of(oracle_mod, "sweep", k)
    src, ctx = context(k, form), context(k, form)
    try:
        build(src, fasta)
        _, _, keys, vals, cnts = src.dbg_dump()
        sel = cnts > 0
        ctx.set_fasta(fasta)
        R, _ = ctx.parse()
        ctx.dbg_load(keys[sel], vals[sel], cnts[sel])
        ctx.build_dbg(np.zeros(R, np.uint8), 0, True)
        check(ctx, ctx.build_rdbg(), ref, form)
    finally:
        src.close()
        ctx.close()


@pytest.mark.parametrize("form", FORMS)
def test_route_finish(oracle_mod, form):
    """Stage A held for one owner (pg_route_stage_a), then pg_route_finish."""
    k = 13
    ref = ref_of(oracle_mod, "sweep", k)
    ctx = context(k, form)
    try:
        ctx.set_fasta(fasta_of("sweep", k))
        ctx.parse()
        counts, sent = ctx.route_stage_a(None, 0, True, 1)
        assert sent and int(counts[0]) > 0
        check(ctx, ctx.route_finish(), ref, form)
    finally:
        ctx.close()


@pytest.mark.parametrize("form", FORMS)
def test_export_twice_and_short_buffer(oracle_mod, form):
    """Two exports in a row give the same keys; a buffer one key too small is
    refused with PG_ERANGE and *n still says how many there are."""
    from pangenome_amd._lib import ptr
    k = 13
    ref = ref_of(oracle_mod, "sweep", k)
    ctx = context(k, form)
    try:
        st = build(ctx, fasta_of("sweep", k))
        check(ctx, st, ref, (form, "first"))
        check(ctx, st, ref, (form, "second"))
        n = C.c_uint64()
        small = np.zeros(ref.shape[0] - 1, np.uint64)
        assert ctx.lib.pg_rdbg_export(ctx.h, ptr(small), small.shape[0], C.byref(n)) == PG_ERANGE
        assert n.value == ref.shape[0] and not small.any()
        check(ctx, st, ref, (form, "after the refusal"))
    finally:
        ctx.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,want", [("empty", 0), ("short", 1)])
def test_nothing_to_export(oracle_mod, name, want, form):
    """An empty input has no key; a single record shorter than k has the n<k
    sentinel alone (no kernel runs for either export)."""
    k = 13
    ref = ref_of(oracle_mod, name, k)
    assert ref.shape[0] == want and (want == 0 or ref[0] == ku.SENTINEL)
    ctx = context(k, form)
    try:
        ctx.parse_host(fasta_of(name, k))
        check(ctx, ctx.build(None, 0, True), ref, (name, form))
    finally:
        ctx.close()
