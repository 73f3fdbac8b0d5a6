"""The bubbles' alleles aligned on the device (pg_region_align,
pangenome_amd/csrc/pg_align.hip).

Every case compares, exactly, the five returned counts, the pair table, the
runs, the primitives, the lines with their carrier words and both texts with an
independent list-based reference (tests/align_util.py).  The synthetic shapes
are the smallest at which each mechanism can go wrong: cores of every length
around one and two 64-row strips and around one packed word of 16 choices, at
every offset mod 16 of the padded blob and on both strands; ties across the
strip border; poisoned buffers with a pair at the blob's end; the cell cap and
one pair per batch; cores of many strips; more pairs than one batch; every
merging rule of the lines with two and three carrier words."""
import ctypes as C
import hashlib
import io
import os

import numpy as np
import pytest

from align_util import (INS, REPL, SNV, assert_files, check_align, check_properties, check_vcf, device_state, golden,
                        reference_align, runs_of, summary)
from freq_util import fasta_names, rows5_of, rows_of
from golden_util import Fixture
from pangenome_rows_util import BORDERS, other, site_frame
from seq_util import fasta_records, make_fasta, parse
from test_align_host import BREAK, HAND, HAND_TAIL, mutate, seg, site_records
from variants_util import reference_variants

pytestmark = pytest.mark.gpu


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


def run(c, sites, ref_group, G=2, min_genomes=2, **kw):
    """site_records' records parsed and the three passes checked."""
    recs, rows, grp = site_records(sites)
    names, seqs = parse(c, make_fasta(recs))
    return check_align(c, rows, grp, G, min_genomes, names, seqs, ref_group, **kw) + (names, seqs)


# ------------------------------------------------------------ 1. empty cases
def test_empty(ctx):
    names, seqs = parse(ctx, make_fasta([acgt(40, 1), acgt(40, 2)]))
    for ref_group in (None, 0):
        res, tsv, vcf = check_align(ctx, np.zeros((0, 5), np.int64), [0, 1], 2, 2, names, seqs, ref_group)
        assert res["n_pairs"] == 0 and tsv.count(b"\n") == 1 and vcf == b""
        assert ctx.region_align() == (0, 0, 0, 0, 0) and ctx.region_align_time() == (0.0, 0)
    # no reference: every site unplaced, the pairs go against allele 0, no lines
    sites = [[(b"ACGTAC", 0, 1), (b"ACTTAC", 1, 1)], [(b"GGA", 0, -1), (b"GGAA", 1, 1), (b"", 1, -1)]]
    res, tsv, vcf, _, _ = run(ctx, sites, None)
    assert res["placed"] == [0, 0, 0] and res["n_lines"] == 0 and vcf == b"" and res["n_prims_all"] == 3
    # a site whose only other allele reads as the reference does
    res, tsv, vcf, _, _ = run(ctx, [[(b"ACGTACGTACGTACGTACGT", 0, 1), (b"ACGTACGTACGTACGTACGT", 1, -1)]], 0)
    assert (res["n_pairs"], res["n_ops_all"], res["n_prims_all"], res["n_lines"]) == (1, 1, 0, 0)
    assert tsv.split(b"\n")[1].endswith(b"\t0\t20\t0\t0\t0\t20=") and vcf == b""


# ------------------------------------------------------------ 2. the hand cases
@pytest.mark.parametrize("T,Q,cigar,prims,vcf", HAND)
def test_hand_cases(ctx, T, Q, cigar, prims, vcf):
    """tests/test_align_host.py's cases through the device, compared with the
    texts typed out there, with each genome in turn as the reference."""
    res, tsv, body, _, _ = run(ctx, [[(T, 0, 1), (Q, 1, 1)]], 0)
    assert tsv.split(b"\n")[1].split(b"\t")[-1] == cigar
    assert body == b"".join(ln + HAND_TAIL for ln in vcf)
    got = ctx.region_align_prims()
    assert list(zip(*[got[k].tolist() for k in ("type", "tpos", "qpos", "tlen", "qlen")])) == prims
    for ref_group in (1, None):
        check_properties(run(ctx, [[(T, 0, 1), (Q, 1, 1)]], ref_group)[0])


# ------------------------------------------------------------ 3. strip and word borders
def border_site(shift, seed=11):
    """pangenome_rows_util.site_frame's site with a 200-letter target of
    uniform noise, the cores about 5 % edits of the letters they replace, or
    unrelated letters, by turns."""
    rng = np.random.default_rng(seed + shift)

    def core(k, t, b):
        if k % 2 and t and b:
            u = mutate(rng, t, 0.05)[:b]
            return u + bytes(rng.choice(list(b"ACGT"), b - len(u)).astype(np.uint8))
        return acgt(b, 1000 * shift + k)
    return site_frame(acgt(200, 300 + shift), shift, core)


@pytest.mark.parametrize("shift", range(16))
def test_strip_and_word_borders(ctx, shift):
    res, _, vcf, names, seqs = run(ctx, border_site(shift), 0, G=3)
    cores = {(n - p - q, m - p - q) for n, m, p, q in zip(res["t_len"], res["q_len"], res["prefix"], res["suffix"])}
    assert res["n_pairs"] == 144 and cores >= {(a, b) for a in BORDERS for b in BORDERS if a * b != 1}
    assert {p % 16 for p in res["prefix"]} >= {shift} and res["n_aligned"] == 144
    check_properties(res)
    check_vcf(res, vcf, names, seqs)
    if shift % 5 == 0:                                   # unplaced: T and Q both start at a multiple of 16
        assert run(ctx, border_site(shift), None, G=3)[0]["n_lines"] == 0


# ------------------------------------------------------------ 4. ties
def tie_sites(unit):
    """Per length n = 1 .. 70 // len(unit) a site: N + n units + N against T +
    n - 1 and n + 1 units + T (letters no unit has) - nothing to trim, every
    place of the gap co-optimal."""
    return [[(b"N" + unit * n + b"N", 0, 1), (b"T" + unit * (n - 1) + b"T", 1, 1), (b"T" + unit * (n + 1) + b"T", 1, -1)]
            for n in range(1, 70 // len(unit) + 1)]


@pytest.mark.parametrize("unit", [b"A", b"AC", b"ACG"])
def test_ties(ctx, unit):
    res, tsv, _, _, _ = run(ctx, tie_sites(unit), 0)
    assert res["prefix"] == [0] * res["n_pairs"] == res["suffix"] and max(res["t_len"]) >= 68
    check_properties(res)
    u = len(unit)
    for j in range(res["n_pairs"]):                      # the gap is the leftmost one: before the first column
        ops = [(chr(res["op"][k]), res["len"][k]) for k in range(res["op_off"][j], res["op_off"][j] + res["n_ops"][j])]
        n = (res["t_len"][j] - 2) // u
        if res["q_len"][j] < res["t_len"][j]:
            assert ops == runs_of("D" * u + "X" + "=" * (u * (n - 1)) + "X"), (j, ops)
        else:
            assert ops == runs_of("I" * u + "X" + "=" * (u * n) + "X"), (j, ops)


# ------------------------------------------------------------ 5. poison
def test_poison():
    """Case 3's borders in a fresh context whose every new device buffer is
    filled with 0xA5 first: a read of a choice word, a row value or a letter
    that nothing wrote would show.  Without a reference the blob ends with the
    last pair's query."""
    from pangenome_amd._lib import PG_TUNE_POISON, Context
    c = Context(27, 0)
    try:
        c.tune(PG_TUNE_POISON, 0xA5)
        for ref_group in (0, None):
            res = run(c, border_site(3), ref_group, G=3)[0]
            assert res["n_pairs"] == 144
    finally:
        c.tune(PG_TUNE_POISON, -1)
        c.close()


# ------------------------------------------------------------ 6. the cap and the batches
def test_cap_and_batches(ctx):
    from pangenome_amd._lib import PG_TUNE_ALIGN_CELLS, PG_TUNE_ALIGN_SCRATCH
    res, tsv, vcf, names, seqs = run(ctx, border_site(7), 0, G=3)
    state = device_state(ctx, names, 3)
    try:
        ctx.tune(PG_TUNE_ALIGN_SCRATCH, 1)               # one pair per batch
        assert ctx.region_align() == (144, 144, res["n_ops_all"], res["n_prims_all"], res["n_lines"])
        assert device_state(ctx, names, 3) == state
        ctx.tune(PG_TUNE_ALIGN_SCRATCH, 1 << 12)         # a few pairs per batch
        ctx.region_align()
        assert device_state(ctx, names, 3) == state
        ctx.tune(PG_TUNE_ALIGN_SCRATCH, 0)
        ctx.tune(PG_TUNE_ALIGN_CELLS, 64)
        capped = run(ctx, border_site(7), 0, G=3, cells_cap=64)[0]
    finally:
        ctx.tune(PG_TUNE_ALIGN_SCRATCH, 0)
        ctx.tune(PG_TUNE_ALIGN_CELLS, 0)
    assert 0 < capped["n_aligned"] < 144 and capped["type"].count(REPL) == 144 - capped["n_aligned"]
    check_properties(capped)
    for j in range(144):                                 # the pairs below the cap are unchanged
        if not capped["status"][j]:
            assert all(capped[k][j] == res[k][j] for k in ("distance", "n_eq", "n_sub", "n_ins", "n_del", "n_ops"))
        else:
            assert (capped["n_prims"][j], capped["distance"][j]) == (1, 2 ** 64 - 1)


# ------------------------------------------------------------ 7. sizes
def test_long_pairs(ctx):
    """2,000 against about 2,100 letters at 1 % edits and 1,500 against 1,500
    unrelated ones: 32 and 24 strips, thousands of traceback steps."""
    rng = np.random.default_rng(9)
    T = acgt(2000, 70)
    Q = bytearray(mutate(rng, T, 0.01))
    Q[700:700] = acgt(100, 71)
    Q[0], Q[-1] = other(T[0]), other(T[-1])
    sites = [[(T, 0, 1), (bytes(Q), 1, -1)], [(b"A" + acgt(1498, 72) + b"A", 0, 1), (b"C" + acgt(1498, 73) + b"C", 1, 1)]]
    res, _, vcf, names, seqs = run(ctx, sites, 0)
    assert res["prefix"] == [0, 0] and res["t_len"] == [2000, 1500] and res["q_len"][1] == 1500
    assert 100 <= res["distance"][0] <= 200 and res["distance"][1] > 700
    check_properties(res)
    check_vcf(res, vcf, names, seqs)
    ms, cells = ctx.region_align_time()
    assert cells == 2000 * res["q_len"][0] + 1500 * 1500 and ms > 0


def test_many_pairs(ctx):
    """17 sites of 300 alleles each, spans of up to 40 letters of two records:
    5,083 pairs, in more than one batch."""
    from pangenome_amd._lib import PG_TUNE_ALIGN_SCRATCH
    names, seqs = parse(ctx, make_fasta([acgt(4100, 80), acgt(4100, 81)]))
    rows = []
    for s in range(17):
        for i in range(300):
            rows += seg(i % 2, 1 if (i + s) % 3 else -1, 10 + 13 * i + s % 5, (7 * i + s) % 41, [1000 + i], a=1 + 2 * s,
                        c=2 + 2 * s)
    try:
        ctx.tune(PG_TUNE_ALIGN_SCRATCH, 1 << 16)
        res, _, vcf = check_align(ctx, rows, [0, 1], 2, 2, names, seqs, 0)
    finally:
        ctx.tune(PG_TUNE_ALIGN_SCRATCH, 0)
    assert res["n_pairs"] == 17 * 299 and res["n_lines"] > 1000
    check_vcf(res, vcf, names, seqs)


# ------------------------------------------------------------ 8. merging
def test_merging(ctx):
    T = b"ACGTTGCAAGGCTA"
    snv = b"ACGTTGGAAGGCTA"                                # C -> G at 6
    sites = [[(T, 0, 1), (snv, 1, 1), (snv[:10] + b"T" + snv[11:], 2, 1), (snv[:2] + snv[3:], 1, -1),
              (T[:4] + b"AA" + T[4:], 3, 1), (T[:4] + b"AC" + T[4:], 3, 1), (T[:4] + b"AA" + T[4:12] + b"GA", 2, 1),
              (T[:12] + b"CC", 1, 1)]]
    # genome 4 has a record and no allele of the site
    recs, rows, grp = site_records(sites)
    recs.append(acgt(30, 90))
    grp.append(4)
    rows += [[len(recs) - 1, 0, 5, 1, 77], BREAK]
    names, seqs = parse(ctx, make_fasta(recs))
    res, _, vcf = check_align(ctx, rows, grp, 5, 2, names, seqs, 0)
    lines = {(ln["type"], ln["tpos"], ln["qlen"]): ln for ln in res["lines"]}
    assert lines[(SNV, 6, 1)]["ac"] == 3 and lines[(SNV, 6, 1)]["n_genomes"] == 2
    text = [ln.split(b"\t") for ln in vcf.split(b"\n")[:-1]]
    by_alt = {(f[1], f[3], f[4]): f[9:] for f in text}
    assert by_alt[(b"12", b"C", b"G")] == [b"0", b"0/1", b"0/1", b"0", b"."]    # genomes with carrying and other alleles
    assert by_alt[(b"9", b"T", b"TAA")] == [b"0", b"0", b"0/1", b"0/1", b"."]   # two alleles, two genomes
    assert by_alt[(b"9", b"T", b"TAC")] == [b"0", b"0", b"0", b"0/1", b"."]     # the same place and length, other letters
    assert sum(f[1] == b"9" and len(f[4]) == 3 for f in text) == 2
    check_vcf(res, vcf, names, seqs)


def test_two_sites_at_one_position(ctx):
    """Sites (7, 8) and (7, 9) behind equal flank rows of the reference: the
    same (record, pos) - by site index - and both targets empty."""
    names, seqs = parse(ctx, make_fasta([acgt(200, 91), acgt(200, 92), acgt(200, 93)]))
    rows = [[0, 100, 104, 1, 7], [0, 104, 110, 1, 8], BREAK, [0, 100, 104, 1, 7], [0, 104, 111, 1, 9], BREAK]
    rows += seg(1, 1, 80, 5, [15], a=7, c=8) + seg(1, 1, 90, 5, [16], a=7, c=9) + seg(2, -1, 40, 3, [17], a=7, c=9)
    res, _, vcf = check_align(ctx, rows, [0, 1, 2], 3, 2, names, seqs, 0)
    assert [(ln["site"], ln["pos"], ln["type"]) for ln in res["lines"]] == [(0, 104, INS), (1, 104, INS), (1, 104, INS)]
    assert [ln["qlen"] for ln in res["lines"]] == [5, 3, 5]
    check_vcf(res, vcf, names, seqs)


@pytest.mark.parametrize("G", [65, 130])
def test_genome_counts(ctx, G):
    """Two and three carrier words: 12 alleles over all genomes, eleven of
    them with one common SNV, the reference the first genome."""
    T = acgt(30, 95)
    snv = T[:9] + bytes([other(T[9])]) + T[10:]
    variants = [T] + [snv[:12 + k] + bytes([other(snv[12 + k])]) + snv[13 + k:] if k > 1 else snv for k in range(1, 12)]
    # the same inner label for the same allele, over every genome
    recs, rows, grp = [], [], []
    for g in range(G):
        body = variants[g % 12]
        rows += seg(g, 1, 5, 30, [1000 + g % 12])
        recs.append(b"GATTC" + body + b"CTTAGGA")
        grp.append(g)
    names, seqs = parse(ctx, make_fasta(recs, names=[b"g%d" % i for i in range(G)]))
    res, _, vcf = check_align(ctx, rows, grp, G, G, names, seqs, 0)
    assert res["n_pairs"] == 11
    common = [ln for ln in res["lines"] if ln["tpos"] == 9]
    carriers = sum(1 for g in range(G) if g % 12)
    assert len(common) == 1 and common[0]["ac"] == 11 and common[0]["n_genomes"] == carriers
    assert len(common[0]["bits"]) == (G + 63) // 64 and common[0]["bits"][-1] != 0
    assert vcf.split(b"\n")[0].split(b"\t")[9:] == [b"1" if g % 12 else b"0" for g in range(G)]


# ------------------------------------------------------------ 9. hash bits
def test_hash_bits(ctx):
    from pangenome_amd._lib import PG_TUNE_ALIGN_HASH_BITS, PangenomeError
    T = b"ACGTTGCAAGG"
    sites = [[(T, 0, 1)] + [(T[:5] + ins + T[5:], 1, 1) for ins in (b"AAC", b"CCA", b"GTG")]]
    res, _, _, names, _ = run(ctx, sites, 0)
    assert res["n_lines"] == 3
    state = device_state(ctx, names, 2)
    try:
        ctx.tune(PG_TUNE_ALIGN_HASH_BITS, 1)             # three letters' hashes in two values: a collision is certain
        with pytest.raises(PangenomeError, match=r"pg_region_align failed \(-5\).*PG_TUNE_ALIGN_HASH_BITS keeps 1 bits"):
            ctx.region_align()
        assert device_state(ctx, names, 2) == state
        T, Q = HAND[8][:2]
        try:
            run(ctx, [[(T, 0, 1), (Q, 1, 1)]], 0)        # the same result, or the refusal
        except PangenomeError as e:
            assert "(-5)" in str(e)
    finally:
        ctx.tune(PG_TUNE_ALIGN_HASH_BITS, 0)


# ------------------------------------------------------------ 10. the pipeline and the committed figures
def test_device_rows_and_golden(ctx):
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
    res, tsv, vcf = check_align(ctx, rows, rec_group, 8, 5, ids, seqs, 0, rows_on_device=True)
    want = golden("pan8_k27_c3_w4")
    assert summary(res, ids, seqs) == want
    assert ctx.region_align() == (want["n_pairs"], want["n_aligned"], want["n_ops"], sum(want["n_prims"].values()),
                                  want["n_lines"])
    assert hashlib.sha256(tsv).hexdigest() == want["tsv_sha256"]
    assert hashlib.sha256(vcf).hexdigest() == want["vcf_sha256"]
    check_properties(res)
    check_vcf(res, vcf, ids, seqs)
    ms, cells = ctx.region_align_time()
    print("pan8_k27_c3: fill %.3f ms, %d cells" % (ms, cells))
    # pg_region_variants' exports are as they were
    from variants_util import assert_same as variants_same
    variants_same(ctx, res["ref"], ids, seqs)
    for ref_group in (3, 7, None):
        check_align(ctx, rows, rec_group, 8, 5, ids, seqs, ref_group, rows_on_device=True)


# ------------------------------------------------------------ 11. refusals and the lifetime
def test_refusals(ctx, tmp_path):
    from pangenome_amd._lib import Context, PangenomeError, ptr
    T, Q = HAND[8][:2]
    recs, rows, grp = site_records([[(T, 0, 1), (Q, 1, 1)]])
    names, seqs = parse(ctx, make_fasta(recs))
    res, tsv, vcf = check_align(ctx, rows, grp, 2, 2, names, seqs, 0)
    state = device_state(ctx, names, 2)
    lib = ctx.lib
    assert lib.pg_region_align(ctx.h, None, None, None, None, None) == 0      # (every count pointer may be NULL)
    assert lib.pg_region_align(None, None, None, None, None, None) == -22
    # a context before any pg_region_variants, and the exports before any pg_region_align
    fresh = Context(27, 0)
    try:
        with pytest.raises(PangenomeError, match=r"pg_region_align failed \(-22\)"):
            fresh.region_align()
        parse(fresh, make_fasta(recs))
        fresh.region_bubbles(grp, 2, 2, rows=rows)
        with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
            fresh.region_align()
        fresh.region_variants(grp, 2, 0, rows=rows)
        for call in (fresh.region_align_pairs, fresh.region_align_ops, fresh.region_align_prims,
                     lambda: fresh.region_align_lines(2), fresh.region_align_time, fresh.region_align_text,
                     lambda: fresh.region_primitives_vcf_text(names), lambda: fresh.region_align_write(1),
                     lambda: fresh.region_primitives_vcf_write(names, 1)):
            with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
                call()
        assert fresh.region_align() == (1, 1, 4, 2, 2)
    finally:
        fresh.close()
    # the size queries, a short cap, the _fd forms, fewer names than records
    n = C.c_uint64()
    blob, off, cnt = (np.frombuffer(b"".join(names), np.uint8), np.cumsum([0] + [len(x) for x in names]).astype(np.int64),
                      len(names))
    assert lib.pg_region_align_format(ctx.h, None, 0, C.byref(n)) == 0 and n.value == len(tsv)
    buf = np.empty(len(tsv), np.uint8)
    assert lib.pg_region_align_format(ctx.h, ptr(buf), len(tsv) - 1, C.byref(n)) == -34
    assert lib.pg_region_align_format(ctx.h, ptr(buf), len(tsv), C.byref(n)) == 0 and buf.tobytes() == tsv
    assert lib.pg_region_align_format(ctx.h, ptr(buf), len(tsv), None) == -22
    assert lib.pg_region_align_format_fd(ctx.h, -1, C.byref(n)) == -22
    fn = lib.pg_region_primitives_vcf
    assert fn(ctx.h, ptr(blob), ptr(off), cnt, None, 0, C.byref(n)) == 0 and n.value == len(vcf)
    buf = np.empty(len(vcf), np.uint8)
    assert fn(ctx.h, ptr(blob), ptr(off), cnt, ptr(buf), len(vcf) - 1, C.byref(n)) == -34
    assert fn(ctx.h, ptr(blob), ptr(off), cnt, ptr(buf), len(vcf), C.byref(n)) == 0 and buf.tobytes() == vcf
    assert fn(ctx.h, ptr(blob), ptr(off), cnt - 1, ptr(buf), len(vcf), C.byref(n)) == -22
    assert lib.pg_region_primitives_vcf_fd(ctx.h, ptr(blob), ptr(off), cnt, -1, C.byref(n)) == -22
    for name, write, text in (("a.tsv", ctx.region_align_write, tsv),
                              ("a.vcf", lambda fd: ctx.region_primitives_vcf_write(names, fd), vcf)):
        with open(tmp_path / name, "wb") as f:
            assert write(f.fileno()) == len(text)
        assert (tmp_path / name).read_bytes() == text
    a = np.empty(8, np.uint64)
    nulls = [None] * 17
    assert lib.pg_region_align_pairs(ctx.h, *nulls, 0) == -34
    assert lib.pg_region_align_pairs(ctx.h, *(nulls[:8] + [ptr(a)] + nulls[9:]), 1) == 0 and a[0] == 3
    assert lib.pg_region_align_ops(ctx.h, None, ptr(a), 3) == -34
    assert lib.pg_region_align_ops(ctx.h, None, ptr(a), 4) == 0 and a[:4].tolist() == [2, 2, 1, 2] == res["len"]
    assert lib.pg_region_align_prims(ctx.h, None, None, ptr(a), None, None, None, 1) == -34
    assert lib.pg_region_align_prims(ctx.h, None, None, ptr(a), None, None, None, 2) == 0 and a[:2].tolist() == [2, 2]
    assert lib.pg_region_align_lines(ctx.h, *([None] * 10), 1) == -34
    assert lib.pg_region_align_lines(ctx.h, *([None] * 10), 2) == 0
    assert device_state(ctx, names, 2) == state
    # the other row passes neither read nor drop it
    ctx.freq(grp, 2, rows=rows)
    ctx.region_graph(grp, 2, rows=rows)
    ctx.region_seqs(grp, 2, rows=rows)
    ctx.region_sites(grp, 2, rows=rows)
    assert device_state(ctx, names, 2) == state
    # refused calls drop nothing; a successful pg_region_variants or pg_region_bubbles drops it
    with pytest.raises(PangenomeError):
        ctx.region_variants(grp, 2, 5, rows=rows)
    with pytest.raises(PangenomeError):
        ctx.region_bubbles(grp, 2, 3, rows=rows)
    assert device_state(ctx, names, 2) == state
    ctx.region_variants(grp, 2, 0, rows=rows)
    with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
        ctx.region_align_text()
    assert ctx.region_align() == (1, 1, 4, 2, 2) and device_state(ctx, names, 2) == state
    ctx.region_bubbles(grp, 2, 2, rows=rows)
    for call in (ctx.region_align_pairs, ctx.region_align_ops, ctx.region_align_prims, lambda: ctx.region_align_lines(2),
                 ctx.region_align_time, ctx.region_align_text, lambda: ctx.region_primitives_vcf_text(names),
                 ctx.region_align):
        with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
            call()


# ------------------------------------------------------------ 12. the CLI
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
    base = ["-g", "record", "-b", "5", "-V", ids[0].decode()]
    q0, plain = _run(km, tmp_path / "plain", fx.fasta, base)
    q, lines = _run(km, tmp_path / "align", fx.fasta, base + ["-A", "1"])
    assert lines == plain
    new = sorted(set(os.listdir(os.path.dirname(q))) - set(os.listdir(os.path.dirname(q0))))
    assert new == ["pan8.fsa_fr_align.tsv", "pan8.fsa_fr_primitives.vcf"]
    for f in os.listdir(os.path.dirname(q0)):
        if not f.endswith(".npz"):                       # (a zip: its members carry a time)
            assert open(os.path.join(os.path.dirname(q), f), "rb").read() == \
                open(os.path.join(os.path.dirname(q0), f), "rb").read(), f
    rows = rows5_of(rows_of("\n".join(lines)), names)
    res = reference_align(reference_variants(rows, list(range(8)), 8, 5, seqs, 0), seqs)
    assert_files(q, res, ids, seqs, ids[0], [(ids[0], len(seqs[0]))], ids)
    assert summary(res, ids, seqs) == golden("pan8_k27_c3_w4")
    # -A 1 without -V: the manual, nothing written
    d = tmp_path / "bad"
    with pytest.raises(SystemExit):
        _run(km, d, fx.fasta, ["-g", "record", "-b", "5", "-A", "1"])
    assert os.listdir(str(d)) == ["pan8.fsa"]
