"""The region graph's host side (no GPU): the `-l` flag and its refusals, the
manual, the nodes-file and npz writer, the multi-process refusal, and the
tests' own reference (tests/region_util.py) pinned against hand-written cases
and the committed expectation for pan8_k27_c3 at -a cc -w 4."""
import io
import os
import sys

import numpy as np
import pytest

from cc_util import cc_text
from dist_util import ROOT, spawn_ranks
from freq_util import fasta_names, rows5_of
from golden_util import Fixture
from region_util import (DTYPES, LINK_COLS, NODE_COLS, PATH_COLS, assert_files, golden, reference_gfa,
                         reference_links_text, reference_region, summary)


def test_parse_args_l():
    from pangenome_amd.kmer import links_arg, parse_args
    assert parse_args(["x", "-i", "f.fa"])["-l"] == "0"
    assert parse_args(["x", "-i", "f.fa", "-l", "1", "-g", "record"])["-l"] == "1"
    assert parse_args(["x", "-i", "f.fa", "-l1", "-k27"])["-l"] == "1"
    assert links_arg({"-l": "0", "-g": ""}) is False and links_arg({"-l": "1", "-g": "record"}) is True
    assert links_arg({"-l": "1", "-g": ""}) is None and links_arg({"-l": "01", "-g": "record"}) is None


@pytest.mark.parametrize("extra", [["-l", "1"], ["-l", "2", "-g", "record"], ["-l", "x", "-g", "record"],
                                   ["-l1"], ["-l-1", "-g", "record"]])
def test_bad_l_is_usage(tmp_path, extra):
    """Refused before anything is read or built: the manual, then SystemExit."""
    from pangenome_amd import kmer
    q = tmp_path / "missing.fa"
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["x", "-i", str(q), "-k27", "-c3", "-a", "cc"] + extra, out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert os.listdir(str(tmp_path)) == []


def test_manual_has_two_l_lines():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("  -l:")]
    assert len(at) == 1 and "single process only" in lines[at[0]]
    # the flag's line and its continuation, directly after -p's two lines
    assert lines[at[0] - 2].startswith("  -p:") and lines[at[0] + 1].startswith("      <in>_fr_links.tsv")
    assert lines[at[0] + 2].startswith("  -c:")
    assert sum("-l" in ln[:6] for ln in lines) == 1 and sum("_fr_links" in ln for ln in lines) == 1
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")


HAND = {"labels": [2, 5, 9], "rows": [3, 2, 1], "max_len": [2 ** 40, 7, 0], "n_out": [2, 1, 0], "n_in": [1, 1, 1],
        "link_from": [2, 2, 5], "link_to": [2, 5, 9], "link_count": [1, 2, 1], "link_genomes": [1, 2, 1],
        "path_record": [0, 1], "path_strand": [1, -1], "path_lo": [-4, 10], "path_hi": [90, 2 ** 35],
        "path_steps": [4, 2], "path_labels": [[2, 2, 5, 9], [2, 5]]}


def test_write_region_files(tmp_path):
    """The nodes file and the npz from a hand-made table; the two texts are
    whatever the callbacks write."""
    from pangenome_amd import host
    names = [b"g0", b"g1"]
    prefix = str(tmp_path / "in.fa")
    table = {k: np.array(HAND[k]) for k in NODE_COLS + LINK_COLS + PATH_COLS}          # (int64: the writer casts)
    host.write_region_files(prefix, lambda f: f.write(reference_links_text(HAND).encode()),
                            lambda f: f.write(reference_gfa(HAND, names)), table, [b"A", b"B"])
    assert sorted(os.listdir(str(tmp_path))) == ["in.fa_fr_graph.gfa", "in.fa_fr_graph.npz", "in.fa_fr_links.tsv",
                                                 "in.fa_fr_nodes.tsv"]
    assert open(prefix + "_fr_nodes.tsv").read() == ("#label\trows\tmax\tout\tin\n2\t3\t1099511627776\t2\t1\n"
                                                     "5\t2\t7\t1\t1\n9\t1\t0\t0\t1\n")
    assert_files(prefix, HAND, names, ["A", "B"])
    z = np.load(prefix + "_fr_graph.npz")
    assert all(z[k].dtype == DTYPES[k] for k in DTYPES) and z["genomes"].dtype.kind == "S"
    # an empty graph: the header alone, empty arrays of the same types
    empty = {k: np.zeros(0, np.int64) for k in NODE_COLS + LINK_COLS + PATH_COLS}
    host.write_region_files(prefix, lambda f: None, lambda f: None, empty, [])
    assert open(prefix + "_fr_nodes.tsv").read() == "#label\trows\tmax\tout\tin\n"
    z = np.load(prefix + "_fr_graph.npz")
    assert all(z[k].dtype == DTYPES[k] and z[k].shape == (0,) for k in DTYPES) and z["genomes"].shape == (0,)


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


def test_dist_entry_point_refuses_l(tmp_path):
    """The multi-process CLI: -l is single process only - the manual on rank
    0, then SystemExit, before anything is built."""
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", "record",
            "-l", "1"]
    exited, text = spawn_ranks(1, _refused_rank, (argv,))[0]
    lines = text.splitlines()
    assert exited and lines[0] == "Usage:" and sum(ln.startswith("  -l:") for ln in lines) == 1
    assert os.listdir(str(tmp_path)) == ["input.fsa"]


# ------------------------------------------------------------ the yardstick itself
def two_rows(second, rec_group=(0, 0)):
    return [[0, 10, 30, 1, 4], second], list(rec_group)


def test_reference_two_rows():
    # same record and strand: one path of two steps, one link
    ref = reference_region(*two_rows([0, 50, 90, 1, 7]), 1)
    assert (ref["labels"], ref["rows"], ref["max_len"], ref["n_out"], ref["n_in"]) == ([4, 7], [1, 1], [20, 40], [1, 0],
                                                                                      [0, 1])
    assert [ref[k] for k in LINK_COLS] == [[4], [7], [1], [1]]
    assert [ref[k] for k in PATH_COLS] == [[0], [1], [10], [90], [2]] and ref["path_labels"] == [[4, 7]]
    assert reference_links_text(ref) == "#from\tto\tcount\tgenomes\n4\t7\t1\t1\n"
    assert reference_gfa(ref, [b"chr1 x"]) == (b"H\tVN:Z:1.0\nS\t4\t*\tLN:i:20\nS\t7\t*\tLN:i:40\n"
                                               b"L\t4\t+\t7\t+\t0M\tRC:i:1\tgn:i:1\nP\tchr1 x:10-90:+\t4+,7+\t*\n")
    # different records, and the same record on two strands: two paths, no link
    for second, grp in (([1, 50, 90, 1, 7], (0, 0)), ([0, 90, 50, -1, 7], (0, 0))):
        ref = reference_region(*two_rows(second, grp), 1)
        assert ref["link_from"] == [] and ref["path_steps"] == [1, 1] and ref["n_out"] == ref["n_in"] == [0, 0]
        assert ref["path_strand"] == [1, second[3]] and ref["path_lo"] == [10, second[1]]
    assert reference_gfa(ref, [b"r"]).endswith(b"P\tr:10-30:+\t4+\t*\nP\tr:90-50:-\t7+\t*\n")
    # an unused row between them, by its label and by its record: two paths, no link, one skipped
    for mid, grp in (([0, 35, 40, 1, -1], (0, 0)), ([1, 35, 40, 1, 6], (0, -1))):
        rows = [[0, 10, 30, 1, 4], mid, [0, 50, 90, 1, 7]]
        ref = reference_region(rows, list(grp), 1)
        assert ref["n_skipped"] == 1 and ref["labels"] == [4, 7] and ref["link_from"] == []
        assert ref["path_steps"] == [1, 1] and ref["path_record"] == [0, 0]


def test_reference_five_rows():
    """A self link, and a link repeated inside one genome: counted twice, one genome."""
    rows = [[0, 0, 10, 1, 5], [0, 10, 13, 1, 5], [0, 13, 20, 1, 8], [0, 20, 21, 1, 5], [0, 30, 21, 1, 8],
            [1, 0, 9, -1, 5], [1, 9, 12, -1, 8]]
    ref = reference_region(rows[:5], [0], 1)
    assert (ref["labels"], ref["rows"], ref["max_len"]) == ([5, 8], [3, 2], [10, 9])
    assert [ref[k] for k in LINK_COLS] == [[5, 5, 8], [5, 8, 5], [1, 2, 1], [1, 1, 1]]
    assert ref["n_out"] == [2, 1] and ref["n_in"] == [2, 1]
    assert [ref[k] for k in PATH_COLS] == [[0], [1], [0], [21], [5]]
    ref = reference_region(rows, [0, 1], 2)                # ... and once more in a second genome
    assert [ref[k] for k in LINK_COLS] == [[5, 5, 8], [5, 8, 5], [1, 3, 1], [1, 2, 1]]
    assert ref["path_steps"] == [5, 2] and ref["path_strand"] == [1, -1]
    s = summary(ref)
    assert (s["n_rows"], s["n_paths"], s["n_pairs"], s["self_links"], s["links_with_reverse"]) == (7, 2, 5, 1, 2)


def test_pan8_oracle_rows_match_the_committed_expectation(oracle_mod):
    """pan8_k27_c3 at -a cc -w 4, one genome per record: the figures of
    tests/golden/region/pan8_k27_c3_w4.json from the oracle's rows."""
    fx = Fixture("pan8_k27_c3")
    lines = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, cc_text("pan8_k27_c3", 4),
                                    edge_chunk=fx.edge_chunk)["rows"]
    ref = reference_region(rows5_of(lines, fasta_names(fx.fasta)), list(range(8)), 8)
    want = golden("pan8_k27_c3_w4")
    got = summary(ref)
    assert {k: want[k] for k in got} == got
    assert got["n_pairs"] == got["n_rows"] - got["n_paths"] == 2929 and got["n_links"] == 1947
