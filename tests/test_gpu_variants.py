"""The bubbles' alleles as sequences and the VCF on the device
(pg_region_variants, pangenome_amd/csrc/pg_variants.hip).

Every case compares, exactly, the four returned counts, the allele table, the
bases, the placed table, the allele FASTA and the VCF body with an independent
list-based reference (tests/variants_util.py).  The synthetic shapes are the
smallest at which each mechanism can go wrong: spans at every lo % 16 with
lengths around one, two and sixteen packed words on both strands behind a short
record, N and lower case at the padding base and at the span borders, a span
at the stream's last base under poisoned buffers, every placement rule, two
and three presence words, two-digit allele numbers, a site of 300 alleles and
an inner path of 300 regions, and more letters than the decoder's grid takes
in one round."""
import ctypes as C
import hashlib
import io
import os

import numpy as np
import pytest

from freq_util import fasta_names, rows5_of, rows_of
from golden_util import Fixture
from seq_util import fasta_records, make_fasta, parse
from test_variants_host import HAND_FASTA, HAND_GROUPS, HAND_PLACED, HAND_ROWS, HAND_SEQS, HAND_VCF
from variants_util import (assert_files, assert_same, check_device, check_vcf, device_state, golden, reference_variants,
                           summary)

pytestmark = pytest.mark.gpu

STRIDE = 2048 * 256 * 16                                 # letters the decoder's capped grid takes in one round
BREAK = [0, 0, 0, 1, -1]                                 # an unused row: it ends the run


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def km():
    from pangenome_amd import kmer
    return kmer


def acgt(n, seed):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def seg(rec, strand, p, length, inner, a=1, c=2, w=3):
    """The rows of one segment whose span is [p, p + length) of record rec,
    then an unused row: flank rows of w bases on either side, as the row pass
    gives them (start > end on the reverse strand, which is walked downward);
    the inner rows carry the labels of `inner` (their coordinates do not
    matter to the span)."""
    q = p + length
    if strand == 1:
        return [[rec, p - w, p, 1, a]] + [[rec, p, q, 1, x] for x in inner] + [[rec, q, q + w, 1, c], BREAK]
    return [[rec, q + w, q, -1, a]] + [[rec, q, p, -1, x] for x in inner] + [[rec, p, p - w, -1, c], BREAK]


# ------------------------------------------------------------ 1. empty cases
def test_empty(ctx):
    names, seqs = parse(ctx, make_fasta([acgt(40, 1), acgt(40, 2)]))
    # no rows; rows without a site; a site and PG_NO_REF
    for rows in (np.zeros((0, 5), np.int64), seg(0, 1, 10, 5, [7]) + seg(1, 1, 10, 5, [7])):
        for ref_group in (None, 0):
            ref, fasta, vcf = check_device(ctx, rows, [0, 1], 2, 2, names, seqs, ref_group)
            assert (fasta, vcf, ctx.region_variants_bases()) == (b"", b"", b"")
            assert (ref["n_alleles"], ref["n_placed"], ref["n_unplaced"]) == (0, 0, 0)
    rows = seg(0, 1, 10, 5, [7]) + seg(1, 1, 10, 0, [])
    ref, fasta, vcf = check_device(ctx, rows, [0, 1], 2, 2, names, seqs, None)
    assert (ref["n_alleles"], ref["n_bases"], ref["n_placed"], ref["n_unplaced"]) == (2, 5, 0, 1)
    assert vcf == b"" and fasta.count(b">") == 2 and ctx.region_variants_time()[1] == 1
    assert check_device(ctx, rows, [0, 1], 2, 2, names, seqs, 1)[0]["n_placed"] == 1


# ------------------------------------------------------------ 2. the hand case
def test_hand_case(ctx):
    """tests/test_variants_host.py's case, compared with the texts typed out
    there: REF is empty, short and long as the reference genome changes."""
    names, seqs = parse(ctx, make_fasta(HAND_SEQS))
    for ref_group in (0, 1, 2):
        ref, fasta, vcf = check_device(ctx, HAND_ROWS, HAND_GROUPS, 3, 3, names, seqs, ref_group)
        assert fasta == HAND_FASTA and vcf == HAND_VCF[ref_group]
        placed = ctx.region_variants_placed()
        assert (placed["ref_row"][0], placed["ref_allele"][0], placed["ref_len"][0]) == HAND_PLACED[ref_group]
        assert ctx.region_variants_bases() == b"CTCCNTG"
    assert check_device(ctx, HAND_ROWS, HAND_GROUPS, 3, 3, names, seqs, None)[1:] == (HAND_FASTA, b"")


# ------------------------------------------------------------ 3. span alignment
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257)


def test_span_alignment(ctx):
    """A 1,000-base record behind a 5-base one: an allele for every lo % 16,
    every length around one, two and sixteen words and both strands, all of
    one site; record 2 is the reference and joins the flanks directly."""
    names, seqs = parse(ctx, make_fasta([acgt(5, 3), acgt(1000, 4), acgt(60, 5)]))
    rows, x = [], 10
    for strand in (1, -1):
        for length in LENGTHS:
            for lo16 in range(16):
                rows += seg(1, strand, 16 + lo16 + 16 * (x % 40), length, [x])
                x += 1
    rows += seg(2, 1, 30, 0, [])
    assert x - 10 == 352 and max(max(r[1], r[2]) for r in rows) <= 1000
    ref, _, vcf = check_device(ctx, rows, [0, 0, 1], 2, 2, names, seqs, 1)
    assert ref["len"][:352] == [n for _ in (1, -1) for n in LENGTHS for _ in range(16)]
    assert ref["n_placed"] == 1 and vcf.split(b"\t")[4].count(b",") == 351
    check_vcf(ref, vcf, names, seqs)


# ------------------------------------------------------------ 4. exceptions, the end of the stream
def test_exceptions(ctx):
    """N, n, R and lower case at the padding base, at both borders of a span
    and inside it, on both strands; the reference's own letters carry them too."""
    recs = [bytearray(acgt(120, 20 + i)) for i in range(3)]
    for rec in recs:
        for p, ch in zip((15, 16, 17, 31, 32, 47, 63, 64, 80), b"NnRacgtN$"):
            rec[p] = ch
    names, seqs = parse(ctx, make_fasta([b"ACG"] + [bytes(r) for r in recs]))
    rows, x = [], 10
    for rec in (1, 2, 3):
        for strand in (1, -1):
            for p, length in ((16, 1), (16, 16), (17, 15), (15, 3), (18, 13), (32, 16), (30, 40), (48, 16), (64, 17),
                              (81, 20)):
                rows += seg(rec, strand, p, length, [x] if rec < 3 else [5])
                x += 1
    # record 3 carries one allele ([5]) at ten places on either strand: its earliest + segment is the reference
    ref, _, vcf = check_device(ctx, rows, [-1, 0, 0, 1], 2, 2, names, seqs, 1)
    assert sum(ref["amb"]) > 40 and ref["n_placed"] == 1 and ref["pos0"] == [16]
    assert vcf.split(b"\t")[3] == b"NN" and vcf.split(b"\t")[4].startswith(b"NN,NNN")
    check_vcf(ref, vcf, names, seqs)


@pytest.mark.parametrize("tail", [0, 1, 15])
def test_end_of_stream(tail):
    """The compacted stream has 64 + tail bases; spans and a REF end at its
    last base on both strands (zero-length flank rows behind them).  Every new
    device buffer is filled with 0xA5 first, so a read beyond the stream's
    last packed word, or of memory nothing wrote, would show as a wrong letter."""
    from pangenome_amd._lib import PG_TUNE_POISON, Context
    c = Context(27, 0)
    try:
        c.tune(PG_TUNE_POISON, 0xA5)
        names, seqs = parse(c, make_fasta([acgt(37, 7), acgt(27 + tail, 8 + tail)]))
        n = len(seqs[1])
        assert (37 + n) % 16 == tail
        rows = []
        for i, length in enumerate((1, 5, 15, 16, 17, n - 4)):
            for strand in (1, -1):
                rows += seg(1, strand, n - length, length, [10 + 2 * i + (strand == 1)], w=0)
        rows += seg(0, 1, 37 - 20, 20, [], w=0)
        ref, _, vcf = check_device(c, rows, [0, 1], 2, 2, names, seqs, 1)
        assert ref["n_placed"] == 1 and ref["pos0"] == [n - 1] and vcf.split(b"\t")[3] == seqs[1][-2:]
        ref, _, _ = check_device(c, rows[:16] + rows[-3:], [0, 1], 2, 2, names, seqs, 0)   # (the scratch is reused)
        assert ref["n_alleles"] == 5 and ref["pos0"] == [17]
    finally:
        c.tune(PG_TUNE_POISON, -1)
        c.close()


# ------------------------------------------------------------ 5. placement rules
def test_placement_rules(ctx):
    names, seqs = parse(ctx, make_fasta([acgt(200, 40 + i) for i in range(5)]))
    grp = [0, 0, 1, 2, -1]
    # site (1, 2): pos0 == 0 on the reference (a zero-length flank row at 0) - unplaced
    rows = seg(0, 1, 0, 4, [10], a=1, c=2, w=0) + seg(2, 1, 50, 0, [], a=1, c=2)
    # site (3, 4): the reference has it on the reverse strand alone - unplaced
    rows += seg(0, -1, 20, 6, [11], a=3, c=4) + seg(2, 1, 60, 2, [], a=3, c=4)
    # site (5, 6): twice on the reference, [13] at row order first but further right, then directly: the
    # earliest row is the reference segment, and the reference genome's cell is 0/1; genome 2 has none: `.`
    rows += seg(1, 1, 150, 7, [13], a=5, c=6) + seg(0, 1, 90, 0, [], a=5, c=6) + seg(2, 1, 70, 3, [14], a=5, c=6)
    # sites (7, 8) and (7, 9): the same (record, pos0) behind equal flank rows; by site index
    rows += [[0, 100, 104, 1, 7], [0, 104, 110, 1, 8], BREAK, [0, 100, 104, 1, 7], [0, 104, 111, 1, 9], BREAK]
    rows += seg(2, 1, 80, 5, [15], a=7, c=8) + seg(2, 1, 90, 5, [16], a=7, c=9)
    # sites (20, 21) and (30, 31): label order and position order disagree, over two reference records
    rows += seg(1, 1, 30, 4, [17], a=20, c=21) + seg(0, 1, 130, 4, [18], a=30, c=31)
    rows += seg(3, 1, 20, 0, [], a=20, c=21) + seg(3, 1, 30, 0, [], a=30, c=31)
    rows += seg(1, 1, 10, 2, [19], a=40, c=41) + seg(3, 1, 40, 0, [], a=40, c=41)
    ref, _, vcf = check_device(ctx, rows, grp, 3, 2, names, seqs, 0)
    bub = ref["bubbles"]
    pairs = [(bub["site_from"][s], bub["site_to"][s]) for s in ref["site"]]
    assert pairs == [(7, 8), (7, 9), (30, 31), (40, 41), (20, 21), (5, 6)] and ref["n_unplaced"] == 2
    assert ref["placed_record"] == [0, 0, 0, 1, 1, 1] and ref["pos0"] == [104, 104, 130, 10, 30, 150]
    lines = vcf.split(b"\n")
    assert lines[5].split(b"\t")[9:] == [b"0/1", b"2", b"."]
    assert lines[0].split(b"\t")[9:] == [b"0", b"1", b"."] and lines[2].split(b"\t")[9:] == [b"0", b".", b"1"]
    check_vcf(ref, vcf, names, seqs)
    # the other genomes as the reference, and none
    for ref_group in (1, 2, None):
        check_device(ctx, rows, grp, 3, 2, names, seqs, ref_group)


# ------------------------------------------------------------ 6. genome counts
@pytest.mark.parametrize("G", [65, 130])
def test_genome_counts(ctx, G):
    """Two and three presence words: a site with 12 alleles (two-digit GT
    numbers) spread over all genomes, the reference the last genome."""
    names, seqs = parse(ctx, make_fasta([acgt(300, 50)] * G, names=[b"g%d" % i for i in range(G)]))
    rows = []
    for g in range(G):
        rows += seg(g, 1 if g % 3 or g == G - 1 else -1, 20 + g, g % 12, [100 + g % 12] if g % 12 else [])
        if g % 5 == 0:
            rows += seg(g, 1, 120, 9, [100 + (g + 7) % 12] if (g + 7) % 12 else [])
    ref, _, vcf = check_device(ctx, rows, list(range(G)), G, G, names, seqs, G - 1)
    assert ref["bubbles"]["site_alleles"] == [12] and ref["n_placed"] == 1
    cells = vcf.split(b"\t")[9:]
    assert len(cells) == G and {b"10", b"11"} <= {x for c in cells for x in c.rstrip(b"\n").split(b"/")}
    assert any(b"/" in c for c in cells) and cells[G - 1].rstrip(b"\n") == b"0"


# ------------------------------------------------------------ 7. sizes
def test_wide_site_and_long_path(ctx):
    """One site with 300 alleles and one inner path of 300 regions - more
    than a wave and than a block - whose reference carries the last allele and
    the long path."""
    names, seqs = parse(ctx, make_fasta([acgt(4000, 60), acgt(4000, 61), acgt(500, 62)]))
    rows = []
    for i in range(299):
        rows += seg(i % 2, 1 if i % 3 else -1, 10 + 13 * i, i % 40, [1000 + i])
    rows += seg(2, 1, 100, 30, [1298])                        # the reference: an allele seen before, far down the list
    path = list(range(2000, 2300))
    rows += seg(0, 1, 3950, 20, path, a=3, c=4) + seg(2, 1, 200, 25, path, a=3, c=4)
    rows += seg(0, 1, 3900, 2, path[:-1] + [9], a=3, c=4) + seg(0, -1, 3850, 0, path[:-1], a=3, c=4)
    rows += seg(1, 1, 3950, 0, [], a=3, c=4)
    rows += seg(2, 1, 300, 4, [1000 + 299])                   # the 300th allele, on the reference alone
    ref, _, vcf = check_device(ctx, rows, [0, 1, 2], 3, 3, names, seqs, 2)
    bub = ref["bubbles"]
    assert bub["site_alleles"] == [300, 4] and max(bub["allele_regions"]) == 300
    assert ref["n_placed"] == 2 and ref["ref_allele"] == [298, 0] and ref["pos0"] == [100, 200]
    check_vcf(ref, vcf, names, seqs)


def test_more_than_one_stride(ctx):
    """Thirty alleles over nearly a whole 300,000-base record: 9,000,000
    letters, more than the decoder's capped grid takes in one round; its
    blocks loop, and a thread goes from one entry to the next."""
    names, seqs = parse(ctx, make_fasta([acgt(300_000, 37), acgt(50, 38)], width=1000))
    rows = []
    for i in range(30):
        rows += seg(0, 1 if i % 2 else -1, 3 + i, 299_900, [10 + i])
    rows += seg(1, 1, 20, 0, [])
    ref, _, _ = check_device(ctx, rows, [0, 1], 2, 2, names, seqs, 1)
    assert STRIDE < ref["n_bases"] <= 32 << 20 and ref["n_placed"] == 1


# ------------------------------------------------------------ 8. 9. the pipeline and the committed figures
def test_device_rows_and_golden(ctx):
    """rows=None takes the last row pass where it lies on the device: the same
    result as the exported rows uploaded again, the reference's, and the
    committed expectation; pg_region_seqs is untouched."""
    fx = Fixture("pan8_k27_c3")
    names, seqs = parse(ctx, fx.fasta)
    ids = [x.split()[0] for x in names]
    ctx.build_dbg(None, 0, True)
    ctx.build_rdbg()
    ctx.edges_count(None, True)
    ctx.cluster_cc(None, None, 4)
    n = ctx.rows_count(None, True)
    rows = ctx.rows_export(n)
    assert n == 2945
    rec_group = np.arange(8, dtype=np.int32)
    ctx.region_seqs(rec_group, 8)
    seq_fasta = ctx.region_fasta_text(ids)
    ref, fasta, vcf = check_device(ctx, rows, rec_group, 8, 5, ids, seqs, 0, rows_on_device=True)
    assert check_device(ctx, rows, rec_group, 8, 5, ids, seqs, 0)[1:] == (fasta, vcf)
    want = golden("pan8_k27_c3_w4")
    assert summary(ref, ids, seqs) == want
    assert (ref["n_alleles"], ref["n_bases"], ref["n_placed"], ref["n_unplaced"]) == (
        want["n_alleles"], want["n_bases"], want["n_placed"], want["n_unplaced"])
    assert hashlib.sha256(fasta).hexdigest() == want["fasta_sha256"]
    assert hashlib.sha256(vcf).hexdigest() == want["vcf_sha256"]
    check_vcf(ref, vcf, ids, seqs)
    assert ctx.region_fasta_text(ids) == seq_fasta
    for ref_group in (3, 7, None):
        check_device(ctx, rows, rec_group, 8, 5, ids, seqs, ref_group, rows_on_device=True)


# ------------------------------------------------------------ 10. refusals and the lifetime
def test_refusals(ctx, tmp_path):
    from pangenome_amd._lib import Context, PangenomeError, ptr
    names, seqs = parse(ctx, make_fasta(HAND_SEQS))
    ref, fasta, vcf = check_device(ctx, HAND_ROWS, HAND_GROUPS, 3, 3, names, seqs, 1)
    state = device_state(ctx, names)
    lib = ctx.lib
    r5, g = np.array(HAND_ROWS, np.int64), np.array(HAND_GROUPS, np.int32)

    def variants(h, r, nr, grp, nrec, G, ref_group):
        return lib.pg_region_variants(h, None if r is None else ptr(np.ascontiguousarray(r, np.int64)), nr,
                                      None if grp is None else ptr(np.ascontiguousarray(grp, np.int32)), nrec, G,
                                      ref_group, None, None, None, None)
    assert variants(ctx.h, r5, 12, g, 4, 3, 1) == 0                      # (every count pointer may be NULL)
    assert variants(None, r5, 12, g, 4, 3, 1) == -22
    assert variants(ctx.h, r5, 12, None, 4, 3, 1) == -22                 # NULL groups
    assert variants(ctx.h, r5, 12, [0, 0, 1, 3], 4, 3, 1) == -22         # a group outside [-1, G)
    assert variants(ctx.h, r5, 12, g, 3, 3, 1) == -22                    # another record count
    assert variants(ctx.h, r5, 12, [0, 0, 1, 2, 2], 5, 3, 1) == -22
    assert variants(ctx.h, r5, 12, g, 4, 4, 1) == -22                    # n_groups other than the bubbles'
    assert variants(ctx.h, r5, 12, g, 4, 3, 3) == -22                    # ref_group == n_groups
    assert variants(ctx.h, r5, 12, g, 4, 3, 2 ** 32 - 2) == -22
    bad = r5.copy()
    bad[11, 2] = 14                                                      # hi past its record
    assert variants(ctx.h, bad, 12, g, 4, 3, 1) == -22
    bad = r5.copy()
    bad[3, 1] = -1                                                       # lo < 0
    assert variants(ctx.h, bad, 12, g, 4, 3, 1) == -22
    for row, col, value in ((9, 4, 8), (1, 4, 6), (0, 4, 3), (2, 4, 3),  # an inner label, a flank label
                            (1, 3, 1), (10, 0, 2), (9, 4, -1)):          # a strand, a record, an unused row
        bad = r5.copy()
        bad[row, col] = value
        assert variants(ctx.h, bad, 12, g, 4, 3, 1) == -22, (row, col)
    assert variants(ctx.h, r5[:11], 11, g, 4, 3, 1) == -22               # an allele's rows leave the list
    assert variants(ctx.h, r5, 12, [0, 0, 1, -1], 4, 3, 1) == -22        # a record without a genome
    bad = r5.copy()
    bad[4, 1:3] = (3, 8)                                                 # the flank rows of r1 overlap: start > end
    assert variants(ctx.h, bad, 12, g, 4, 3, 2 ** 32 - 1) == -22
    bad = r5.copy()
    bad[7, 1:3] = (3, 10)                                                # the reference segment's (r2 is no
    assert variants(ctx.h, bad, 12, g, 4, 3, 1) == -22                   # allele's representative)
    assert variants(ctx.h, bad, 12, g, 4, 3, 0) == 0
    check_device(ctx, HAND_ROWS, HAND_GROUPS, 3, 3, names, seqs, 1)
    # a reference segment that is no allele: r2 joins the flanks through [6] (every allele's own rows still match)
    bad = r5.copy()
    bad[6, 4] = 6
    assert variants(ctx.h, bad, 12, g, 4, 3, 1) == -22
    with pytest.raises(PangenomeError, match=r"pg_region_variants failed \(-22\).*not of these rows"):
        ctx.region_variants(HAND_GROUPS, 3, 1, rows=r5[:11])
    # every refusal left the previous result in place
    assert device_state(ctx, names) == state
    # a context without a parse, and the exports before any pg_region_variants
    fresh = Context(27, 0)
    try:
        fresh.region_bubbles(HAND_GROUPS, 3, 3, rows=r5)
        assert variants(fresh.h, r5, 12, g, 4, 3, 1) == -22
        for call in (fresh.region_variants_alleles, fresh.region_variants_bases, fresh.region_variants_placed,
                     fresh.region_variants_time, lambda: fresh.region_alleles_fasta_text(names),
                     lambda: fresh.region_vcf_text(names), lambda: fresh.region_vcf_write(names, 1),
                     lambda: fresh.region_alleles_fasta_write(names, 1)):
            with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
                call()
        parse(fresh, make_fasta(HAND_SEQS))
        assert variants(fresh.h, None, 0, g, 4, 3, 1) == -22             # no row pass
        assert variants(fresh.h, r5, 12, g, 4, 3, 1) == 0
        fresh2 = Context(27, 0)
        try:
            parse(fresh2, make_fasta(HAND_SEQS))
            assert variants(fresh2.h, r5, 12, g, 4, 3, 1) == -22         # no bubbles result
        finally:
            fresh2.close()
    finally:
        fresh.close()
    # the size query, a short cap, the _fd forms, fewer names than records
    n = C.c_uint64()
    blob, off, cnt = (np.frombuffer(b"".join(names), np.uint8), np.cumsum([0] + [len(x) for x in names]).astype(np.int64),
                      len(names))
    for fn, fd_fn, text in ((lib.pg_region_alleles_fasta, lib.pg_region_alleles_fasta_fd, fasta),
                            (lib.pg_region_vcf, lib.pg_region_vcf_fd, vcf)):
        assert fn(ctx.h, ptr(blob), ptr(off), cnt, None, 0, C.byref(n)) == 0 and n.value == len(text)
        buf = np.empty(len(text), np.uint8)
        assert fn(ctx.h, ptr(blob), ptr(off), cnt, ptr(buf), len(text) - 1, C.byref(n)) == -34
        assert fn(ctx.h, ptr(blob), ptr(off), cnt, ptr(buf), len(text), C.byref(n)) == 0 and buf.tobytes() == text
        assert fn(ctx.h, ptr(blob), ptr(off), cnt, ptr(buf), len(text), None) == -22
        assert fn(ctx.h, ptr(blob), ptr(off), cnt - 1, ptr(buf), len(text), C.byref(n)) == -22
        assert fd_fn(ctx.h, ptr(blob), ptr(off), cnt, -1, C.byref(n)) == -22
    for name, write, text in (("a.fa", ctx.region_alleles_fasta_write, fasta), ("a.vcf", ctx.region_vcf_write, vcf)):
        with open(tmp_path / name, "wb") as f:
            assert write(names, f.fileno()) == len(text)
        assert (tmp_path / name).read_bytes() == text
    a = np.empty(8, np.int64)
    assert lib.pg_region_variants_alleles(ctx.h, None, None, ptr(a), None, None, None, None, None, 2) == -34
    assert lib.pg_region_variants_alleles(ctx.h, None, None, ptr(a), None, None, None, None, None, 3) == 0
    assert a[:3].tolist() == ref["hi"]
    assert lib.pg_region_variants_placed(ctx.h, None, None, ptr(a), None, None, None, 0) == -34
    assert lib.pg_region_variants_placed(ctx.h, None, None, ptr(a), None, None, None, 1) == 0 and a[0] == 4
    assert lib.pg_region_variants_bases(ctx.h, ptr(a), 6, C.byref(n)) == -34
    assert lib.pg_region_variants_bases(ctx.h, None, 0, C.byref(n)) == 0 and n.value == 7
    assert device_state(ctx, names) == state
    # the other row passes neither read nor drop it; a later pg_region_bubbles drops it
    ctx.freq(HAND_GROUPS, 3, rows=r5)
    ctx.region_graph(HAND_GROUPS, 3, rows=r5)
    ctx.region_seqs(HAND_GROUPS, 3, rows=r5)
    ctx.region_sites(HAND_GROUPS, 3, rows=r5)
    assert device_state(ctx, names) == state
    with pytest.raises(PangenomeError):
        ctx.region_bubbles(HAND_GROUPS, 3, 4, rows=r5)                   # refused: nothing is dropped
    assert device_state(ctx, names) == state
    ctx.region_bubbles(HAND_GROUPS, 3, 3, rows=r5)
    for call in (ctx.region_variants_alleles, ctx.region_variants_bases, ctx.region_variants_placed,
                 ctx.region_variants_time, lambda: ctx.region_vcf_text(names),
                 lambda: ctx.region_alleles_fasta_text(names)):
        with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
            call()


# ------------------------------------------------------------ 11. the CLI
def _run(km, d, fasta, extra):
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    km.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def test_cli(km, tmp_path):
    fx = Fixture("pan8_k27_c3")
    names = fasta_names(fx.fasta)
    ids = [n.split()[0].encode() for n in names]
    _, seqs = fasta_records(fx.fasta)
    q0, plain = _run(km, tmp_path / "plain", fx.fasta, ["-g", "record", "-b", "5"])
    q, lines = _run(km, tmp_path / "variants", fx.fasta, ["-g", "record", "-b", "5", "-V", ids[0].decode()])
    # stdout and every other file are those of the run without -V
    assert lines == plain
    new = sorted(set(os.listdir(os.path.dirname(q))) - set(os.listdir(os.path.dirname(q0))))
    assert new == ["pan8.fsa_fr_alleles.fa", "pan8.fsa_fr_alleles.tsv", "pan8.fsa_fr_variants.vcf"]
    for f in os.listdir(os.path.dirname(q0)):
        if not f.endswith(".npz"):                       # (a zip: its members carry a time)
            assert open(os.path.join(os.path.dirname(q), f), "rb").read() == \
                open(os.path.join(os.path.dirname(q0), f), "rb").read(), f
    rows = rows5_of(rows_of("\n".join(lines)), names)
    ref = reference_variants(rows, list(range(8)), 8, 5, seqs, 0)
    assert_files(q, ref, ids, seqs, ids[0], [(ids[0], len(seqs[0]))], ids)
    assert summary(ref, ids, seqs) == golden("pan8_k27_c3_w4")
    body = b"".join(ln + b"\n" for ln in open(q + "_fr_variants.vcf", "rb").read().split(b"\n")[:-1]
                    if not ln.startswith(b"#"))
    check_vcf(ref, body, ids, seqs)
    # a name that is no genome: an error before the dBG is built, nothing written
    d = tmp_path / "nogenome"
    with pytest.raises(ValueError, match="-V: no genome is called 'nobody'"):
        _run(km, d, fx.fasta, ["-g", "record", "-b", "5", "-V", "nobody"])
    assert os.listdir(str(d)) == ["pan8.fsa"]
    # refused before anything is built
    for i, extra in enumerate((["-V", ids[0].decode()], ["-g", "record", "-V", ids[0].decode()])):
        d = tmp_path / ("bad%d" % i)
        with pytest.raises(SystemExit):
            _run(km, d, fx.fasta, extra)
        assert os.listdir(str(d)) == ["pan8.fsa"]
