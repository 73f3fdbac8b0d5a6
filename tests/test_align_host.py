"""The alignments' host side (no GPU): the tests' own reference
(tests/align_util.py) pinned against hand cases typed out here and four
properties over random pairs, the `-A` flag and its refusals, the manual, the
file writer driven by a fake context's texts, the multi-process refusal, and
the committed expectation for pan8_k27_c3 at -a cc -w 4 -b 5 -V g0 -A 1."""
import io
import os
import sys

import numpy as np
import pytest

from align_util import (DEL, INS, SNV, align_pair, apply_prims, check_properties, check_vcf, golden, reference_align,
                        reference_header, reference_primitives_vcf, reference_tsv, summary)
from cc_util import cc_text
from dist_util import ROOT, spawn_ranks
from freq_util import fasta_names, rows5_of
from golden_util import Fixture
from pangenome_amd.kmer import align_arg, parse_args
from seq_util import COMPLEMENT, fasta_records, make_fasta
from variants_util import reference_variants

BREAK = [0, 0, 0, 1, -1]                                 # an unused row: it ends the run
PRE, POST = b"GATTC", b"CTTAGGA"                         # what stands before and behind every allele in its record


def seg(rec, strand, p, length, inner, a=1, c=2, w=3):
    """The rows of one segment whose span is [p, p + length) of record rec,
    then an unused row (test_gpu_variants.py's idiom)."""
    q = p + length
    if strand == 1:
        return [[rec, p - w, p, 1, a]] + [[rec, p, q, 1, x] for x in inner] + [[rec, q, q + w, 1, c], BREAK]
    return [[rec, q + w, q, -1, a]] + [[rec, q, p, -1, x] for x in inner] + [[rec, p, p - w, -1, c], BREAK]


def site_records(sites):
    """sites[s]: the alleles of site s as (sequence, genome, strand) - each in
    a record of its own, PRE + the letters as the record reads them + POST,
    behind an inner label of its own.  Returns (records, rows, rec_group)."""
    recs, rows, grp = [], [], []
    for s, alleles in enumerate(sites):
        for seq, genome, strand in alleles:
            body = seq if strand == 1 else seq[::-1].translate(COMPLEMENT)
            rows += seg(len(recs), strand, len(PRE), len(seq), [1000 + len(recs)], a=1 + 2 * s, c=2 + 2 * s)
            recs.append(PRE + body + POST)
            grp.append(genome)
    return recs, rows, grp


# ------------------------------------------------------------ the hand cases
# T, Q, the CIGAR, the primitives (type, tpos, qpos, tlen, qlen) and the VCF lines with T's genome as the
# reference: T is record r0 at pos0 = 5 behind the padding base C
HAND = [
    (b"AAA", b"AA", b"1D2=", [(DEL, 0, 0, 1, 0)], [b"r0\t5\t1_2\tCA\tC"]),
    (b"ACACAC", b"ACAC", b"2D4=", [(DEL, 0, 0, 2, 0)], [b"r0\t5\t1_2\tCAC\tC"]),
    (b"AAAA", b"AA", b"2D2=", [(DEL, 0, 0, 2, 0)], [b"r0\t5\t1_2\tCAA\tC"]),
    (b"ACGT", b"ACGT", b"4=", [], []),
    (b"", b"", b"*", [], []),
    (b"", b"ACG", b"3I", [(INS, 0, 0, 0, 3)], [b"r0\t5\t1_2\tC\tCACG"]),
    (b"ACG", b"", b"3D", [(DEL, 0, 0, 3, 0)], [b"r0\t5\t1_2\tCACG\tC"]),
    (b"ACNGT", b"ACTGT", b"2=1X2=", [(SNV, 2, 2, 1, 1)], [b"r0\t8\t1_2\tN\tT"]),
    (b"AAGCC", b"AATTTCC", b"2=2I1X2=", [(INS, 2, 2, 0, 2), (SNV, 2, 4, 1, 1)],
     [b"r0\t7\t1_2\tA\tATT", b"r0\t8\t1_2\tG\tT"]),
]
HAND_TAIL = b"\t.\t.\tNS=2;AC=1\tGT\t0\t1\n"


def hand_site(T, Q):
    recs, rows, grp = site_records([[(T, 0, 1), (Q, 1, 1)]])
    names, seqs = fasta_records(make_fasta(recs))
    return rows, grp, names, seqs


@pytest.mark.parametrize("T,Q,cigar,prims,vcf", HAND)
def test_reference_hand_cases(T, Q, cigar, prims, vcf):
    r = align_pair(T, Q)
    assert b"".join(b"%d%s" % (n, c.encode()) for c, n in r["runs"]) == (b"" if cigar == b"*" else cigar)
    assert r["prims"] == prims and r["status"] == 0
    assert r["distance"] == sum(max(p[3], p[4]) for p in prims)
    assert apply_prims(T, Q, prims) == Q
    rows, grp, names, seqs = hand_site(T, Q)
    res = reference_align(reference_variants(rows, grp, 2, 2, seqs, 0), seqs)
    assert (res["n_pairs"], res["placed"], res["allele"]) == (1, [1], [1])
    assert reference_tsv(res).split(b"\n")[1].split(b"\t")[-1] == cigar
    assert reference_tsv(res).split(b"\n")[1].split(b"\t")[:8] == [b"1", b"2", b"1", b"ref", b"%d" % len(T),
                                                                   b"%d" % len(Q), b"%d" % r["prefix"],
                                                                   b"%d" % r["suffix"]]
    body = reference_primitives_vcf(res, names, seqs)
    assert body == b"".join(ln + HAND_TAIL for ln in vcf)
    check_properties(res)
    check_vcf(res, body, names, seqs)
    # without a reference the target is allele 0, the same letters: the same pair, and no lines
    res = reference_align(reference_variants(rows, grp, 2, 2, seqs, None), seqs)
    assert res["placed"] == [0] and res["lines"] == [] and reference_tsv(res).split(b"\n")[1].split(b"\t")[3] == b"0"
    assert [tuple(res[k][i] for k in ("type", "tpos", "qpos", "tlen", "qlen")) for i in range(len(prims))] == prims


def test_the_gap_is_leftmost_and_the_cap_replaces():
    assert align_pair(b"AAA", b"AA")["prims"] == [(DEL, 0, 0, 1, 0)]            # the first A
    assert align_pair(b"GAAAC", b"GAAC")["runs"] == [("=", 1), ("D", 1), ("=", 3)]
    assert align_pair(b"CACACAT", b"CACACACAT")["runs"] == [("I", 2), ("=", 7)]   # (the suffix takes all of T)
    # G against TCA: the diagonal comes first going backwards, so the mismatch is G / A and the gap lies before it
    assert align_pair(b"GCACAT", b"TCACACAG")["runs"] == [("I", 2), ("X", 1), ("=", 4), ("X", 1)]
    r = align_pair(b"GGACGTCC", b"GGTTCC", cells_cap=7)                        # core ACG / T: 4 x 2 cells
    assert (r["status"], r["runs"], r["prims"]) == (1, [("=", 2), ("D", 3), ("I", 1), ("=", 3)], [(3, 2, 2, 3, 1)])
    assert (r["n_eq"], r["n_sub"], r["n_ins"], r["n_del"]) == (5, 0, 1, 3) and r["distance"] == 2 ** 64 - 1
    assert align_pair(b"GGACGTCC", b"GGTTCC", cells_cap=8)["status"] == 0


def mutate(rng, s, rate):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append(b"ACGT"[rng.integers(0, 4)])
        out.append(b"ACGT"[rng.integers(0, 4)] if x > 1 - rate / 3 else ch)
    return bytes(out)


def test_properties_over_random_pairs():
    """300 pairs: related and unrelated, two-letter alphabets (many ties),
    lengths 0 .. 90 and one above the anti-diagonal threshold, checked with
    both fills of the matrix."""
    import align_util
    rng = np.random.default_rng(5)
    sites = []
    for i in range(300):
        alpha = b"AC" if i % 3 == 0 else b"ACGT"
        T = bytes(alpha[x] for x in rng.integers(0, len(alpha), int(rng.integers(0, 90))))
        Q = mutate(rng, T, 0.15) if i % 2 else bytes(alpha[x] for x in rng.integers(0, len(alpha), int(rng.integers(0, 90))))
        sites.append([(T, 0, 1), (Q, 1, 1 if i % 5 else -1)])
    big = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 400))
    sites.append([(big, 0, 1), (mutate(rng, big, 0.05), 1, 1)])
    recs, rows, grp = site_records(sites)
    names, seqs = fasta_records(make_fasta(recs))
    res = reference_align(reference_variants(rows, grp, 2, 2, seqs, 0), seqs)
    assert res["n_pairs"] == 301 and res["n_aligned"] == 301 and res["n_lines"] == len(res["pair"])
    check_properties(res)
    check_vcf(res, reference_primitives_vcf(res, names, seqs), names, seqs)
    saved = align_util.NUMPY_FROM
    try:
        for j in range(0, 301, 7):                        # the two fills of the matrix agree
            both = []
            for align_util.NUMPY_FROM in (0, 10 ** 12):
                both.append(align_pair(res["T"][j], res["Q"][j]))
            assert both[0] == both[1]
    finally:
        align_util.NUMPY_FROM = saved


# ------------------------------------------------------------ the flag
def test_parse_args_A():
    assert parse_args(["x", "-i", "f.fa"])["-A"] == "0"
    assert parse_args(["x", "-i", "f.fa", "-A", "1"])["-A"] == "1" and parse_args(["x", "-A1"])["-A"] == "1"
    assert align_arg({"-A": "0"}, "") is False and align_arg({"-A": "0"}, "g0") is False
    assert align_arg({"-A": "1"}, "g0") is True
    assert align_arg({"-A": "1"}, "") is None and align_arg({"-A": "1"}, None) is None
    assert align_arg({"-A": "2"}, "g0") is None and align_arg({"-A": "x"}, "g0") is None


@pytest.mark.parametrize("extra", [["-A", "1"], ["-A", "1", "-g", "record", "-b", "5"], ["-A", "1", "-V", "g0"],
                                   ["-A", "1", "-V", "g0", "-g", "record"], ["-A", "2", "-V", "g0", "-g", "record", "-b", "5"],
                                   ["-Ax", "-V", "g0", "-g", "record", "-b", "5"]])
def test_bad_A_is_usage(tmp_path, extra):
    """Refused before anything is read or built: the manual, then SystemExit."""
    from pangenome_amd import kmer
    q = tmp_path / "missing.fa"
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["x", "-i", str(q), "-k27", "-c3", "-a", "cc"] + extra, out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert os.listdir(str(tmp_path)) == []


def test_manual_has_two_A_lines():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("  -A:")]
    assert len(at) == 1 and lines[at[0] - 1].startswith("  -k:") and lines[at[0] + 2].startswith("  -d:")
    second = lines[at[0] + 1]
    assert second.startswith("      ") and "single process only" in second
    assert "_fr_align.tsv" in second and "_fr_primitives.vcf" in second


# ------------------------------------------------------------ the file writer
def test_write_align_files(tmp_path):
    from pangenome_amd import host
    gnames = [b"g0", b"g1"]
    header = host.primitives_vcf_header(b"g0", [(b"r0", 15)], gnames)
    assert header == reference_header(b"g0", [(b"r0", 15)], gnames)
    assert header.count(b"##INFO=<ID=NS,") == 1 and header.count(b"##INFO=<ID=AC,") == 1
    assert header.count(b"##FORMAT=<ID=GT,") == 1 and host.VCF_GT not in header
    assert header.split(b"\n")[-2] == b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tg0\tg1"
    assert b"ID=AC" not in host.vcf_header(b"g0", [(b"r0", 15)], gnames)      # (the -V header is as it was)
    prefix = str(tmp_path / "in.fa")
    body = HAND[0][4][0] + HAND_TAIL
    host.write_align_files(prefix, lambda f: f.write(b"tsv\n"), header, lambda f: f.write(body))
    assert sorted(os.listdir(str(tmp_path))) == ["in.fa_fr_align.tsv", "in.fa_fr_primitives.vcf"]
    assert open(prefix + "_fr_align.tsv", "rb").read() == b"tsv\n"
    assert open(prefix + "_fr_primitives.vcf", "rb").read() == header + body
    host.write_align_files(prefix, lambda f: None, header, lambda f: None)
    assert open(prefix + "_fr_align.tsv", "rb").read() == b""
    assert open(prefix + "_fr_primitives.vcf", "rb").read() == header


def _refused_rank(rank, world, port, q, argv):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from dist_util import OracleShard
    from pangenome_amd import dist as pdist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = io.StringIO()
    exited = False
    try:
        pdist.entry_point(argv, out=out, shard_factory=OracleShard)
    except SystemExit:
        exited = True
    finally:
        dist.destroy_process_group()
    q.put((rank, (exited, out.getvalue())))


def test_dist_entry_point_refuses_A(tmp_path):
    """The multi-process CLI: -A is single process only - the manual on rank
    0, then SystemExit, before anything is built."""
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-A", "1"]
    exited, text = spawn_ranks(1, _refused_rank, (argv,))[0]
    lines = text.splitlines()
    assert exited and lines[0] == "Usage:" and sum(ln.startswith("  -A:") for ln in lines) == 1
    assert os.listdir(str(tmp_path)) == ["input.fsa"]


# ------------------------------------------------------------ the committed expectation
def test_pan8_oracle_rows_match_the_committed_expectation(oracle_mod):
    """pan8_k27_c3 at -a cc -w 4 -b 5 against its first genome, one genome per
    record: the figures of tests/golden/align/pan8_k27_c3_w4.json.  That file
    was produced by this same yardstick (align_util.summary of
    align_util.reference_align) from the oracle's rows; it pins the yardstick
    and the input against drift, and the GPU tests compare the device's result
    with both."""
    fx = Fixture("pan8_k27_c3")
    lines = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, cc_text("pan8_k27_c3", 4),
                                    edge_chunk=fx.edge_chunk)["rows"]
    rows = rows5_of(lines, fasta_names(fx.fasta))
    rnames, seqs = fasta_records(fx.fasta)
    ids = [x.split()[0] for x in rnames]
    res = reference_align(reference_variants(rows, list(range(8)), 8, 5, seqs, 0), seqs)
    assert summary(res, ids, seqs) == golden("pan8_k27_c3_w4")
    assert res["n_pairs"] == 478 - 186 == 292 and res["n_lines"] == 913
    assert max((n - p - q + 1) * (m - p - q + 1) for n, m, p, q in zip(res["t_len"], res["q_len"], res["prefix"],
                                                                       res["suffix"])) == 990_640
    check_properties(res)
    check_vcf(res, reference_primitives_vcf(res, ids, seqs), ids, seqs)
