"""The region sequences' host side (no GPU): the `-s` flag and its refusals,
the manual, the file writer, the multi-process refusal, and the tests' own
reference (tests/seq_util.py) pinned against hand-written cases and the
committed expectation for pan8_k27_c3 at -a cc -w 4."""
import io
import os
import sys

import numpy as np
import pytest

from cc_util import cc_text
from dist_util import ROOT, spawn_ranks
from freq_util import fasta_names, rows5_of
from golden_util import Fixture
from region_util import reference_region
from seq_util import (INT_COLS, UINT_COLS, fasta_records, golden, make_fasta, reference_fasta, reference_gfa_seq,
                      reference_seqs, reference_tsv, summary)


def test_parse_args_s():
    from pangenome_amd.kmer import parse_args, seqs_arg
    assert parse_args(["x", "-i", "f.fa"])["-s"] == "0"
    assert parse_args(["x", "-i", "f.fa", "-s", "1", "-g", "record"])["-s"] == "1"
    assert parse_args(["x", "-i", "f.fa", "-s1", "-k27"])["-s"] == "1"
    assert seqs_arg({"-s": "0", "-g": ""}) is False and seqs_arg({"-s": "1", "-g": "record"}) is True
    assert seqs_arg({"-s": "1", "-g": ""}) is None and seqs_arg({"-s": "01", "-g": "record"}) is None


@pytest.mark.parametrize("extra", [["-s", "1"], ["-s", "2", "-g", "record"], ["-s", "x", "-g", "record"], ["-s1"]])
def test_bad_s_is_usage(tmp_path, extra):
    """Refused before anything is read or built: the manual, then SystemExit."""
    from pangenome_amd import kmer
    q = tmp_path / "missing.fa"
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["x", "-i", str(q), "-k27", "-c3", "-a", "cc"] + extra, out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert os.listdir(str(tmp_path)) == []


def test_manual_has_two_s_lines():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("  -s:")]
    assert len(at) == 1 and "single process only" in lines[at[0]]
    # the flag's line and its continuation, directly after -n: and before -g:
    assert lines[at[0] - 1].startswith("  -n:") and lines[at[0] + 1].startswith("      <in>_fr_regions.fa")
    assert lines[at[0] + 2].startswith("  -g:")
    assert sum("-s" in ln[:6] for ln in lines) == 1 and sum("_fr_regions.fa" in ln for ln in lines) == 1
    assert "-s" in kmer.__doc__.split("ours:")[1].split(")")[0].split()


HAND = {"label": [2, 5, 9], "row": [4, 0, 7], "record": [1, 0, 1], "start": [3, 2 ** 33, 9], "end": [7, 2 ** 33 + 2, 9],
        "strand": [1, -1, 1], "len": [4, 2, 0], "gc": [2, 0, 0], "amb": [1, 0, 0], "offset": [0, 4, 6],
        "seqs": [b"ACGN", b"TT", b""]}


def test_write_region_seq_files(tmp_path):
    """The table's file from a hand-made table; the two texts are whatever
    the callbacks write, and the GFA only when one is given."""
    from pangenome_amd import host
    ids = [b"g0", b"g1"]
    prefix = str(tmp_path / "in.fa")
    table = {k: np.array(HAND[k]) for k in INT_COLS + UINT_COLS}
    host.write_region_seq_files(prefix, lambda f: f.write(reference_fasta(HAND, ids)), table, ids)
    assert sorted(os.listdir(str(tmp_path))) == ["in.fa_fr_regions.fa", "in.fa_fr_regions.tsv"]
    assert open(prefix + "_fr_regions.tsv", "rb").read() == (
        b"#label\trow\tseqid\tstart\tend\tstrand\tlen\tgc\tamb\n2\t4\tg1\t3\t7\t1\t4\t2\t1\n"
        b"5\t0\tg0\t8589934592\t8589934594\t-1\t2\t0\t0\n9\t7\tg1\t9\t9\t1\t0\t0\t0\n") == reference_tsv(HAND, ids)
    assert open(prefix + "_fr_regions.fa", "rb").read() == (b">2 g1:3-7:+ len=4\nACGN\n>5 g0:8589934592-8589934594:- "
                                                            b"len=2\nTT\n>9 g1:9-9:+ len=0\n\n")
    host.write_region_seq_files(prefix, lambda f: None, table, ids, lambda f: f.write(b"H\tVN:Z:1.0\n"))
    assert sorted(os.listdir(str(tmp_path))) == ["in.fa_fr_graph_seq.gfa", "in.fa_fr_regions.fa",
                                                 "in.fa_fr_regions.tsv"]
    assert open(prefix + "_fr_graph_seq.gfa", "rb").read() == b"H\tVN:Z:1.0\n"
    # an empty table: the header alone
    empty = {k: np.zeros(0, np.int64) for k in INT_COLS + UINT_COLS}
    host.write_region_seq_files(prefix, lambda f: None, empty, [])
    assert open(prefix + "_fr_regions.tsv", "rb").read() == b"#label\trow\tseqid\tstart\tend\tstrand\tlen\tgc\tamb\n"
    assert open(prefix + "_fr_regions.fa", "rb").read() == b""


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


def test_dist_entry_point_refuses_s(tmp_path):
    """The multi-process CLI: -s is single process only - the manual on rank
    0, then SystemExit, before anything is built."""
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", "record",
            "-s", "1"]
    exited, text = spawn_ranks(1, _refused_rank, (argv,))[0]
    lines = text.splitlines()
    assert exited and lines[0] == "Usage:" and sum(ln.startswith("  -s:") for ln in lines) == 1
    assert os.listdir(str(tmp_path)) == ["input.fsa"]


# ------------------------------------------------------------ the yardstick itself
FASTA = b">chr1 first\nACGTAC\nGTNNac\n>chr2\ngtRYacgt\n\n>e\n"


def test_fasta_records_and_make_fasta():
    names, seqs = fasta_records(FASTA)
    assert names == [b"chr1 first", b"chr2", b"e"] and seqs == [b"ACGTACGTNNAC", b"GTNNACGT", b""]
    assert fasta_records(make_fasta([b"ACGTACGTNNAC", b"gtRYacgt", b""], width=5)) == (
        [b"r0", b"r1", b"r2"], seqs)
    assert make_fasta([b"ACGTACG"], width=3) == b">r0\nACG\nTAC\nG\n"


def test_reference_hand_cases():
    names, seqs = fasta_records(FASTA)
    # both strands, start > end on the reverse strand, N and lower case in the input
    rows = [[0, 0, 4, 1, 3], [0, 12, 6, -1, 1], [1, 0, 8, 1, 7], [1, 8, 2, -1, 0]]
    ref = reference_seqs(rows, [0, 0, -1], 1, seqs)
    assert ref["label"] == [0, 1, 3, 7] and ref["row"] == [3, 1, 0, 2] and ref["n_skipped"] == 0
    assert ref["seqs"] == [b"ACGTNN", b"GTNNAC", b"ACGT", b"GTNNACGT"]
    assert (ref["len"], ref["gc"], ref["amb"], ref["offset"]) == ([6, 6, 4, 8], [2, 2, 2, 3], [2, 2, 0, 2],
                                                                   [0, 6, 12, 16])
    assert ref["start"] == [8, 12, 0, 0] and ref["end"] == [2, 6, 4, 8] and ref["strand"] == [-1, -1, 1, 1]
    assert ref["bases"] == b"ACGTNNGTNNACACGTGTNNACGT"
    assert reference_fasta(ref, names) == (b">0 chr2:2-8:- len=6\nACGTNN\n>1 chr1 first:6-12:- len=6\nGTNNAC\n"
                                           b">3 chr1 first:0-4:+ len=4\nACGT\n>7 chr2:0-8:+ len=8\nGTNNACGT\n")
    assert reference_tsv(ref, [b"chr1", b"chr2", b"e"]).split(b"\n")[1] == b"0\t3\tchr2\t8\t2\t-1\t6\t2\t2"
    # a tie: the first row wins; a strictly longer later row wins; a longer unused row does not
    rows = [[0, 0, 3, 1, 5], [0, 4, 7, 1, 5], [0, 1, 4, -1, 5]]
    assert reference_seqs(rows, [0, 0, 0], 1, seqs)["row"] == [0]
    assert reference_seqs(rows + [[1, 0, 4, 1, 5]], [0, 0, 0], 1, seqs)["seqs"] == [b"GTNN"]
    ref = reference_seqs(rows + [[1, 0, 4, 1, 5], [0, 0, 9, 1, -1], [2, 0, 0, 1, 5]], [0, -1, 0], 1, seqs)
    assert ref["row"] == [0] and ref["n_skipped"] == 2 and ref["seqs"] == [b"ACG"]
    # a row of length 0, and no rows at all
    ref = reference_seqs([[2, 0, 0, -1, 4]], [0, 0, 0], 1, seqs)
    assert ref["len"] == [0] and ref["bases"] == b"" and reference_fasta(ref, names) == b">4 e:0-0:- len=0\n\n"
    ref = reference_seqs(np.zeros((0, 5), np.int64), [0, 0, 0], 1, seqs)
    assert ref["label"] == [] and reference_fasta(ref, names) == b""
    # the GFA with sequences: region_util's text with the S lines filled in
    rows = [[0, 0, 4, 1, 3], [0, 4, 10, 1, 1]]
    ref, graph = reference_seqs(rows, [0, 0, 0], 1, seqs), reference_region(rows, [0, 0, 0], 1)
    assert reference_gfa_seq(graph, ref, names) == (b"H\tVN:Z:1.0\nS\t1\tACGTNN\tLN:i:6\nS\t3\tACGT\tLN:i:4\n"
                                                    b"L\t3\t+\t1\t+\t0M\tRC:i:1\tgn:i:1\n"
                                                    b"P\tchr1 first:0-10:+\t3+,1+\t*\n")


def test_pan8_oracle_rows_match_the_committed_expectation(oracle_mod):
    """pan8_k27_c3 at -a cc -w 4, one genome per record: the figures of
    tests/golden/regionseq/pan8_k27_c3_w4.json.  That file was produced by
    this same yardstick (seq_util.summary of seq_util.reference_seqs) from the
    oracle's rows; it pins the yardstick and the input against drift, and the
    GPU tests compare the device's result with both."""
    fx = Fixture("pan8_k27_c3")
    lines = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, cc_text("pan8_k27_c3", 4),
                                    edge_chunk=fx.edge_chunk)["rows"]
    names = fasta_names(fx.fasta)
    rows = rows5_of(lines, names)
    rnames, seqs = fasta_records(fx.fasta)
    assert [x.decode() for x in rnames] == names
    ref = reference_seqs(rows, list(range(8)), 8, seqs)
    got = summary(ref, [x.split()[0] for x in rnames])
    assert got == golden("pan8_k27_c3_w4")
    assert got["n_regions"] == 909
    graph = reference_region(rows, list(range(8)), 8)
    assert ref["label"] == graph["labels"] and ref["len"] == graph["max_len"]
