"""The variants' host side (no GPU): the `-V` flag and its refusals, the
manual, the file writer driven by a fake context's texts, the multi-process
refusal, and the tests' own reference (tests/variants_util.py) pinned against
a hand case typed out here and the committed expectation for pan8_k27_c3 at
-a cc -w 4 -b 5 -V g0."""
import io
import os
import sys

import numpy as np
import pytest

from cc_util import cc_text
from dist_util import ROOT, spawn_ranks
from freq_util import fasta_names, rows5_of
from golden_util import Fixture
from seq_util import fasta_records, make_fasta
from variants_util import (check_vcf, golden, reference_fasta, reference_header, reference_tsv, reference_variants,
                           reference_vcf, summary)

# ------------------------------------------------------------ the hand case
# Four records, three genomes (r0 and r1 are g0); the anchors 1 and 2 (in all three genomes) are joined
# through [5] (r0 on the reverse strand, r2), directly (r1) and through [6, 7] (r3).
HAND_SEQS = [b"GGCCAGACGT", b"ACGTGGCC", b"ACGTAAGGCC", b"ACGTCCNtgGGCC"]
HAND_ROWS = [[0, 10, 6, -1, 1], [0, 6, 4, -1, 5], [0, 4, 0, -1, 2],
             [1, 0, 4, 1, 1], [1, 4, 8, 1, 2],
             [2, 0, 4, 1, 1], [2, 4, 6, 1, 5], [2, 6, 10, 1, 2],
             [3, 0, 4, 1, 1], [3, 4, 7, 1, 6], [3, 7, 9, 1, 7], [3, 9, 13, 1, 2]]
HAND_GROUPS = [0, 0, 1, 2]
HAND_FASTA = (b">1_2_0 r0:4-6:- regions=1 genomes=2 len=2\nCT\n>1_2_1 r1:4-4:+ regions=0 genomes=1 len=0\n\n"
              b">1_2_2 r3:4-9:+ regions=2 genomes=1 len=5\nCCNTG\n")
HAND_VCF = {0: b"r1\t4\t1_2\tT\tTCT,TCCNTG\t.\t.\tNS=3\tGT\t0/1\t1\t2\n",
            1: b"r2\t4\t1_2\tTAA\tT,TCCNTG\t.\t.\tNS=3\tGT\t0/1\t0\t2\n",
            2: b"r3\t4\t1_2\tTCCNTG\tTCT,T\t.\t.\tNS=3\tGT\t1/2\t1\t0\n"}
HAND_PLACED = {0: (3, 1, 0), 1: (5, 0, 2), 2: (8, 2, 5)}         # ref_row, ref_allele, ref_len


def hand():
    names, seqs = fasta_records(make_fasta(HAND_SEQS))
    return names, seqs


def test_reference_hand_case():
    names, seqs = hand()
    assert seqs[3] == b"ACGTCCNTGGGCC"
    for ref_group in (0, 1, 2):
        ref = reference_variants(HAND_ROWS, HAND_GROUPS, 3, 3, seqs, ref_group)
        assert ref["record"] == [0, 1, 3] and ref["lo"] == [4, 4, 4] and ref["hi"] == [6, 4, 9]
        assert ref["strand"] == [-1, 1, 1] and ref["len"] == [2, 0, 5] and ref["offset"] == [0, 2, 2]
        assert ref["gc"] == [1, 0, 3] and ref["amb"] == [0, 0, 1] and ref["bases"] == b"CTCCNTG"
        assert (ref["n_alleles"], ref["n_bases"], ref["n_placed"], ref["n_unplaced"]) == (3, 7, 1, 0)
        assert reference_fasta(ref, names) == HAND_FASTA
        assert reference_vcf(ref, names, seqs) == HAND_VCF[ref_group]
        assert (ref["ref_row"][0], ref["ref_allele"][0], ref["ref_len"][0]) == HAND_PLACED[ref_group]
        assert ref["site"] == [0] and ref["pos0"] == [4]
        check_vcf(ref, HAND_VCF[ref_group], names, seqs)
    ref = reference_variants(HAND_ROWS, HAND_GROUPS, 3, 3, seqs, None)
    assert (ref["n_placed"], ref["n_unplaced"]) == (0, 1) and reference_vcf(ref, names, seqs) == b""
    assert reference_fasta(ref, names) == HAND_FASTA
    assert reference_tsv(ref, names) == (b"#from\tto\tallele\tregions\tseqid\tstart\tend\tstrand\tlen\tgc\tamb\n"
                                         b"1\t2\t0\t1\tr0\t4\t6\t-1\t2\t1\t0\n1\t2\t1\t0\tr1\t4\t4\t1\t0\t0\t0\n"
                                         b"1\t2\t2\t2\tr3\t4\t9\t1\t5\t3\t1\n")


def test_reference_placement_rules():
    """pos0 == 0 and a reference on the reverse strand alone give unplaced
    sites; the earliest reference row wins."""
    seqs = [b"ACGTACGTACGTACGTACGT"] * 3
    # record 0: a zero-length flank row at 0, so that pos0 = 0
    rows = [[0, 0, 0, 1, 1], [0, 0, 3, 1, 5], [0, 3, 6, 1, 2], [1, 0, 2, 1, 1], [1, 2, 6, 1, 2]]
    ref = reference_variants(rows, [0, 1, -1], 2, 2, seqs, 0)
    assert (ref["n_placed"], ref["n_unplaced"]) == (0, 1) and ref["len"] == [3, 0]
    ref = reference_variants(rows, [0, 1, -1], 2, 2, seqs, 1)
    assert (ref["n_placed"], ref["pos0"], ref["ref_allele"]) == (1, [2], [1])
    # the reference carries the site on the reverse strand alone
    rows = [[0, 9, 6, -1, 1], [0, 6, 3, -1, 5], [0, 3, 0, -1, 2], [1, 0, 2, 1, 1], [1, 2, 6, 1, 2]]
    ref = reference_variants(rows, [0, 1, -1], 2, 2, seqs, 0)
    assert (ref["n_placed"], ref["n_unplaced"]) == (0, 1) and ref["seqs"] == [b"GTA", b""]
    # twice on the reference: the earliest row, and both alleles in its cell
    rows = [[1, 0, 2, 1, 1], [1, 2, 6, 1, 2], [0, 1, 4, 1, 1], [0, 4, 5, 1, 5], [0, 5, 8, 1, 2], [0, 8, 10, 1, 1],
            [0, 10, 12, 1, 2]]
    ref = reference_variants(rows, [0, 1, -1], 2, 2, seqs, 0)
    assert ref["ref_row"] == [2] and ref["pos0"] == [4] and ref["ref_allele"] == [1]
    assert reference_vcf(ref, [b"a", b"b", b"c"], seqs) == b"a\t4\t1_2\tTA\tT\t.\t.\tNS=2\tGT\t0/1\t1\n"


# ------------------------------------------------------------ the flag
def test_parse_args_V():
    from pangenome_amd.kmer import parse_args, variants_arg
    assert parse_args(["x", "-i", "f.fa"])["-V"] == ""
    assert parse_args(["x", "-i", "f.fa", "-V", "g0", "-g", "record"])["-V"] == "g0"
    assert parse_args(["x", "-i", "f.fa", "-Vg0"])["-V"] == "g0"
    assert variants_arg({"-V": "", "-g": ""}, 0) == "" and variants_arg({"-V": "g0", "-g": "record"}, 5) == "g0"
    assert variants_arg({"-V": "g0", "-g": ""}, 5) is None and variants_arg({"-V": "g0", "-g": "record"}, 0) is None


@pytest.mark.parametrize("extra", [["-V", "g0"], ["-V", "g0", "-g", "record"], ["-V", "g0", "-g", "record", "-b", "0"],
                                   ["-V", "g0", "-b", "5"], ["-Vg0", "-g", "record", "-b", "x"]])
def test_bad_V_is_usage(tmp_path, extra):
    """Refused before anything is read or built: the manual, then SystemExit."""
    from pangenome_amd import kmer
    q = tmp_path / "missing.fa"
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["x", "-i", str(q), "-k27", "-c3", "-a", "cc"] + extra, out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert os.listdir(str(tmp_path)) == []


def test_manual_has_two_V_lines():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("  -V:")]
    assert len(at) == 1 and "single process only" in lines[at[0] + 1]
    # directly after -g's two lines and before -p: (the other flags' places, and -c: -a: -w: at the end, are pinned)
    assert lines[at[0] - 2].startswith("  -g:") and lines[at[0] + 2].startswith("  -p:")
    assert lines[-3].startswith("  -c:") and lines[-2].startswith("  -a:")
    assert lines[at[0] + 1].startswith("      ") and "_fr_variants.vcf" in lines[at[0] + 1]
    for ln in lines[at[0]:at[0] + 2]:
        assert not any(x in ln for x in ("_fr_bubbles", "_fr_sites", "_fr_links", "_fr_regions.fa"))
        assert not any(x in ln[:6] for x in ("-b", "-v", "-s", "-l"))


def test_ref_genome_and_the_parsed_records_check():
    from pangenome_amd import kmer
    assert kmer.ref_genome([b"a", b"b", b"a"], "a") == 0 and kmer.ref_genome([b"a", b"b"], b"b") == 1
    with pytest.raises(ValueError, match="-V: no genome is called 'c'"):
        kmer.ref_genome([b"a", b"b"], "c")


# ------------------------------------------------------------ the file writer
def test_write_variants_files(tmp_path):
    """The three files from the hand case: the texts are whatever the fake
    context's callbacks write, the table's file and the VCF header the host's."""
    from pangenome_amd import host
    names, seqs = hand()
    ref = reference_variants(HAND_ROWS, HAND_GROUPS, 3, 3, seqs, 1)
    table = {"from": np.array([1, 1, 1]), "to": np.array([2, 2, 2]), "allele": np.array([0, 1, 2]),
             "regions": np.array([1, 0, 2], np.uint64), "record": np.array(ref["record"]), "lo": np.array(ref["lo"]),
             "hi": np.array(ref["hi"]), "strand": np.array(ref["strand"]), "len": np.array(ref["len"], np.uint64),
             "gc": np.array(ref["gc"], np.uint64), "amb": np.array(ref["amb"], np.uint64)}
    prefix = str(tmp_path / "in.fa")
    gnames = [b"g0", b"g1", b"g2"]
    header = host.vcf_header(b"g1", [(b"r2", 10)], gnames)
    assert header == reference_header(b"g1", [(b"r2", 10)], gnames)
    assert header.split(b"\n")[:4] == [b"##fileformat=VCFv4.2", b"##source=pangenome_amd", b"##reference=g1",
                                       b"##contig=<ID=r2,length=10>"]
    assert header.split(b"\n")[-2] == b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tg0\tg1\tg2"
    assert header.count(b"##INFO=<ID=NS,") == 1 and header.count(b"##FORMAT=<ID=GT,") == 1
    host.write_variants_files(prefix, lambda f: f.write(HAND_FASTA), table, names, header,
                              lambda f: f.write(HAND_VCF[1]))
    assert sorted(os.listdir(str(tmp_path))) == ["in.fa_fr_alleles.fa", "in.fa_fr_alleles.tsv", "in.fa_fr_variants.vcf"]
    assert open(prefix + "_fr_alleles.fa", "rb").read() == HAND_FASTA
    assert open(prefix + "_fr_alleles.tsv", "rb").read() == reference_tsv(ref, names)
    assert open(prefix + "_fr_variants.vcf", "rb").read() == header + HAND_VCF[1]
    # nothing placed, no alleles: the headers alone
    empty = {k: np.zeros(0, np.int64) for k in host.VARIANT_COLS}
    host.write_variants_files(prefix, lambda f: None, empty, [], header, lambda f: None)
    assert open(prefix + "_fr_alleles.fa", "rb").read() == b""
    assert open(prefix + "_fr_alleles.tsv", "rb").read().count(b"\n") == 1
    assert open(prefix + "_fr_variants.vcf", "rb").read() == header


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


def test_dist_entry_point_refuses_V(tmp_path):
    """The multi-process CLI: -V is single process only - the manual on rank
    0, then SystemExit, before anything is built."""
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", "record",
            "-V", "g0"]
    exited, text = spawn_ranks(1, _refused_rank, (argv,))[0]
    lines = text.splitlines()
    assert exited and lines[0] == "Usage:" and sum(ln.startswith("  -V:") for ln in lines) == 1
    assert os.listdir(str(tmp_path)) == ["input.fsa"]


# ------------------------------------------------------------ the committed expectation
def test_pan8_oracle_rows_match_the_committed_expectation(oracle_mod):
    """pan8_k27_c3 at -a cc -w 4 -b 5 against its first genome, one genome per
    record: the figures of tests/golden/variants/pan8_k27_c3_w4.json.  That
    file was produced by this same yardstick (variants_util.summary of
    variants_util.reference_variants) from the oracle's rows; it pins the
    yardstick and the input against drift, and the GPU tests compare the
    device's result with both."""
    fx = Fixture("pan8_k27_c3")
    lines = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, cc_text("pan8_k27_c3", 4),
                                    edge_chunk=fx.edge_chunk)["rows"]
    names = fasta_names(fx.fasta)
    rows = rows5_of(lines, names)
    rnames, seqs = fasta_records(fx.fasta)
    ids = [x.split()[0] for x in rnames]
    ref = reference_variants(rows, list(range(8)), 8, 5, seqs, 0)
    assert summary(ref, ids, seqs) == golden("pan8_k27_c3_w4")
    assert ref["n_alleles"] == 478 and ref["n_placed"] > 20 and ref["n_unplaced"] > 20
    assert min(ref["len"]) == 0 and {1, -1} <= set(ref["strand"])
    check_vcf(ref, reference_vcf(ref, ids, seqs), ids, seqs)
