"""The packed coverage pass's geometry comes from k_tiles' per-group
descriptors (GroupGeo) and the host's per-XCD chunk bounds: builds through
the public API on the smallest shapes at which that geometry changes form,
against the oracle (dBG keys and masks, rdBG keys), and - for inputs whose
followers are exact copies of the lead, where wrong geometry would leave the
graph right and only cover fewer windows - the stage A record and work item
counts recorded from the commit before the descriptors.
"""
import numpy as np
import pytest

from cover_geo_util import IDENTICAL, TILE, check, copies, drifting, fasta_of, golden, identical_stats

pytestmark = pytest.mark.gpu


_REFS = {}


def ref_of(oracle_mod, fasta, k=27):
    """The oracle's run of an input, made once and shared."""
    key = (hash(fasta), len(fasta), k)
    if key not in _REFS:
        _REFS[key] = oracle_mod.OracleRun(fasta, k, 2)
    return _REFS[key]


def build_and_check(oracle_mod, fasta, k=27, tunes=(), what=""):
    from pangenome_amd._lib import Context
    ref = ref_of(oracle_mod, fasta, k)
    ctx = Context(k)
    try:
        for t, v in tunes:
            ctx.tune(t, v)
        ctx.set_fasta(fasta)
        ctx.parse()
        st = ctx.build(None, 0, True)
        check(ctx, ref, what)
        return st
    finally:
        ctx.close()


@pytest.mark.parametrize("k", [27, 13, 5])
@pytest.mark.parametrize("length", ["TILE - 1", "TILE", "TILE + k", "2 * TILE + 5", "TILE + k - 2", "2 * TILE + k - 2"])
def test_record_lengths_around_the_tile(oracle_mod, k, length):
    """Five records of one length: the references' span clipped at the record
    end, a partial last stripe, anchors past the record end (TILE + k - 2 and
    2 TILE + k - 2 bases are one window below one and two tiles)."""
    n = eval(length, {"TILE": TILE, "k": k})
    build_and_check(oracle_mod, fasta_of(drifting([n] * 5, 100 + n)), k)


@pytest.mark.parametrize("lengths", [
    [2 * TILE + 200, 2 * TILE + 300] + [3 * TILE - 100] * 4,      # the references shorter than their followers
    [4 * TILE - 9, 4 * TILE - 500, TILE + 700, TILE + 40, TILE - 3, 3 * TILE],   # and longer
])
def test_reference_length(oracle_mod, lengths):
    build_and_check(oracle_mod, fasta_of(drifting(lengths, 7 + len(lengths))))


@pytest.mark.parametrize("n_rec", [1, 2, 3, 5, 6, 10])
def test_record_counts(oracle_mod, n_rec):
    """A lead alone, a follower without a second reference, one full group, a
    group with three empty slots, several groups per stripe."""
    build_and_check(oracle_mod, fasta_of(drifting([2 * TILE + 300 - 7 * i for i in range(n_rec)], 40 + n_rec)))


@pytest.mark.parametrize("k", [27, 13, 5])
def test_record_starts_mod_16(oracle_mod, k):
    """16 records whose lengths are 1 mod 16: their starts in the compacted
    stream take every residue mod 16 (the members' word index and shift)."""
    lengths = [TILE + 16 * (9 - (i % 5)) + 1 for i in range(16)]
    assert sorted(int(x) % 16 for x in np.cumsum([0] + lengths[:-1])) == list(range(16))
    build_and_check(oracle_mod, fasta_of(drifting(lengths, 16 + k)), k)


@pytest.mark.parametrize("k", [27, 5])
def test_non_acgt_bases(oracle_mod, k):
    """An N inside the lead's and the second reference's staged spans and
    inside a member's words: the two exception paths."""
    seqs = drifting([2 * TILE + 77] * 6, 55)
    seqs[0][TILE + 300] = ord("N")                    # the lead, second stripe
    seqs[1][100:103] = ord("n")                       # the second reference, first stripe
    seqs[3][TILE - 8:TILE + 9] = ord("N")             # a member, across the stripe boundary
    seqs[5][2 * TILE + 70] = ord("R")                 # a member's last words
    build_and_check(oracle_mod, fasta_of(seqs), k)


def _chunk_fasta(n_rec, length, seed):
    return fasta_of(drifting([length - 13 * i for i in range(n_rec)], seed))


@pytest.mark.parametrize("chunks", [2, 3, 6])
@pytest.mark.parametrize("head,tail", [(1, 16), (7, 7), (16, 1)])
@pytest.mark.parametrize("n_rec,length", [(13, 5 * TILE + 100), (3, 2 * TILE - 40)])
def test_forced_chunks(oracle_mod, chunks, head, tail, n_rec, length):
    """The tile list forced into chunks of uneven weight over a few groups
    (13 records of five stripes: 4 groups per stripe with the lead's, 20-odd
    in all, not a multiple of 8; 3 records of two stripes: fewer groups than
    XCDs, so some XCDs and some chunks get none)."""
    from pangenome_amd._lib import PG_TUNE_K3_CHUNKS, PG_TUNE_K3_HEAD, PG_TUNE_K3_TAIL
    build_and_check(oracle_mod, _chunk_fasta(n_rec, length, 300 + n_rec),
                    tunes=((PG_TUNE_K3_CHUNKS, chunks), (PG_TUNE_K3_HEAD, head), (PG_TUNE_K3_TAIL, tail)))


@pytest.mark.parametrize("h2d", [4096, 20000])
def test_build_host_incremental(oracle_mod, h2d):
    """pg_build_host with a small upload chunk: stage A in incremental parts,
    k_tiles per part, the followers of later parts against the first part's
    references."""
    from pangenome_amd._lib import Context, PG_TUNE_H2D_CHUNK
    fasta = _chunk_fasta(13, 5 * TILE + 100, 313)
    ref = ref_of(oracle_mod, fasta)
    ctx = Context(27)
    try:
        ctx.tune(PG_TUNE_H2D_CHUNK, h2d)
        for what in ("cold", "warm"):
            ctx.build_host(fasta, True)
            check(ctx, ref, what)
    finally:
        ctx.close()


def test_held_stage_a(oracle_mod):
    """pg_route_stage_a + pg_route_finish: stage A held for one owner."""
    from pangenome_amd._lib import Context
    fasta = _chunk_fasta(13, 5 * TILE + 100, 313)
    ref = ref_of(oracle_mod, fasta)
    ctx = Context(27)
    try:
        ctx.set_fasta(fasta)
        ctx.parse()
        counts, _ = ctx.route_stage_a(None, 0, True, 1)
        assert int(counts[0]) > 0
        ctx.route_finish()
        check(ctx, ref)
    finally:
        ctx.close()


@pytest.mark.parametrize("n_rec,length", IDENTICAL)
def test_no_coverage_lost(oracle_mod, n_rec, length):
    """Followers that are exact copies of the lead: the stage A records and
    the work items left by the coverage pass are fixed by the input, and equal
    the counts of the commit before the descriptors (c21c24a: its library ran
    cover_geo_util.identical_stats three times per case, in a fresh process;
    the three agreed on every case, so none is dropped, and that library also
    passes this test behind the others of this file:
    tests/golden/cover_geo/identical.json)."""
    want = golden()["%dx%d" % (n_rec, length)]
    assert list(identical_stats(n_rec, length)) == want
    build_and_check(oracle_mod, fasta_of(copies(n_rec, length, 900 + n_rec)))
