"""The variable sites' host side (no GPU): the `-v` flag and its refusals, the
manual, the file writer, the multi-process refusal, and the tests' own
reference (tests/sites_util.py) pinned against hand-written cases and the
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
from sites_util import (ALLELE_COLS, DTYPES, GENOME_COLS, HEADER, SITE_COLS, assert_files, golden, reference_sites,
                        reference_text, summary)


def test_parse_args_v():
    from pangenome_amd.kmer import parse_args, sites_arg
    assert parse_args(["x", "-i", "f.fa"])["-v"] == "0"
    assert parse_args(["x", "-i", "f.fa", "-v", "1", "-g", "record"])["-v"] == "1"
    assert parse_args(["x", "-i", "f.fa", "-v1", "-k27"])["-v"] == "1"
    assert sites_arg({"-v": "0", "-g": ""}) is False and sites_arg({"-v": "1", "-g": "record"}) is True
    assert sites_arg({"-v": "0", "-g": "record"}) is False
    assert sites_arg({"-v": "1", "-g": ""}) is None and sites_arg({"-v": "01", "-g": "record"}) is None


@pytest.mark.parametrize("extra", [["-v", "1"], ["-v", "2", "-g", "record"], ["-v", "x", "-g", "record"],
                                   ["-v1"], ["-v-1", "-g", "record"]])
def test_bad_v_is_usage(tmp_path, extra):
    """Refused before anything is read or built: the manual, then SystemExit."""
    from pangenome_amd import kmer
    q = tmp_path / "missing.fa"
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["x", "-i", str(q), "-k27", "-c3", "-a", "cc"] + extra, out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert os.listdir(str(tmp_path)) == []


def test_manual_has_two_v_lines():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("  -v:")]
    assert len(at) == 1 and "with -g" in lines[at[0]]
    # the flag's line and its continuation, directly after -R: and before -I:
    assert lines[at[0] - 1].startswith("  -R:") and lines[at[0] + 2].startswith("  -I:")
    two = lines[at[0]] + lines[at[0] + 1]
    assert lines[at[0] + 1].startswith("      ") and "single process only" in two
    assert all(s in two for s in ("<in>_fr_sites.tsv", "_fr_sites_genomes.tsv", "_fr_sites.npz"))
    assert "_fr_links" not in two and "_fr_regions.fa" not in two
    assert sum("-v" in ln[:6] for ln in lines) == 1 and sum("_fr_sites" in ln for ln in lines) == 1


HAND = {"site_from": [2, 7], "site_to": [9, 7], "site_alleles": [2, 3], "site_first": [0, 2], "site_count": [3, 2 ** 33],
        "site_genomes": [2, 70], "allele_site": [0, 0, 1, 1, 1], "allele_via": [-1, 4, -1, 7, 2 ** 31 - 1],
        "allele_count": [2, 1, 5, 2 ** 33 - 6, 1], "allele_genomes": [2, 1, 1, 69, 1],
        "allele_min": [0, 3, 0, 1, 2 ** 40], "allele_max": [0, 3, 0, 8, 2 ** 40],
        "bits": [[3, 0], [2, 0], [1, 0], [2 ** 64 - 2, 63], [0, 32]],
        "genome_sites": [2, 2] + [1] * 68, "genome_alleles": [2, 3] + [1] * 68, "genome_private": [1, 1] + [0] * 67 + [1]}


def test_write_sites_files(tmp_path):
    """The genomes file and the npz from a hand-made table; the text is
    whatever the callback writes."""
    from pangenome_amd import host
    gnames = ["g%d" % i for i in range(70)]
    prefix = str(tmp_path / "in.fa")
    table = {k: np.array(HAND[k]) for k in SITE_COLS + ALLELE_COLS + GENOME_COLS}      # (the writer casts)
    table["bits"] = np.array(HAND["bits"], np.uint64)
    host.write_sites_files(prefix, lambda f: f.write(reference_text(HAND).encode()), table,
                           [x.encode() for x in gnames])
    assert sorted(os.listdir(str(tmp_path))) == ["in.fa_fr_sites.npz", "in.fa_fr_sites.tsv",
                                                 "in.fa_fr_sites_genomes.tsv"]
    assert open(prefix + "_fr_sites.tsv").read() == (HEADER + "2\t9\t*\t2\t2\t0\t0\n2\t9\t4\t1\t1\t3\t3\n"
                                                     "7\t7\t*\t5\t1\t0\t0\n7\t7\t7\t8589934586\t69\t1\t8\n"
                                                     "7\t7\t2147483647\t1\t1\t1099511627776\t1099511627776\n")
    assert open(prefix + "_fr_sites_genomes.tsv").read().startswith("#genome\tsites\talleles\tprivate\ng0\t2\t2\t1\n"
                                                                    "g1\t2\t3\t1\ng2\t1\t1\t0\n")
    assert_files(prefix, HAND, gnames)
    z = np.load(prefix + "_fr_sites.npz")
    assert all(z[k].dtype == DTYPES[k] for k in DTYPES) and z["genomes"].dtype.kind == "S"
    assert z["bits"].dtype == np.uint64 and z["bits"].shape == (5, 2)
    # no sites: the headers alone, empty arrays of the same types
    empty = {k: np.zeros(0, np.int64) for k in SITE_COLS + ALLELE_COLS}
    empty.update({k: np.zeros(3, np.int64) for k in GENOME_COLS}, bits=np.zeros((0, 1), np.uint64))
    host.write_sites_files(prefix, lambda f: f.write(HEADER.encode()), empty, [b"A", b"B", b"C"])
    assert open(prefix + "_fr_sites.tsv").read() == HEADER
    assert open(prefix + "_fr_sites_genomes.tsv").read() == "#genome\tsites\talleles\tprivate\nA\t0\t0\t0\nB\t0\t0\t0\nC\t0\t0\t0\n"
    z = np.load(prefix + "_fr_sites.npz")
    assert all(z[k].dtype == DTYPES[k] and z[k].shape == (0,) for k in SITE_COLS + ALLELE_COLS)
    assert z["bits"].shape == (0, 1) and z["genome_sites"].tolist() == [0, 0, 0] and z["genomes"].shape == (3,)
    host.write_sites_files(prefix, lambda f: None, {**empty, **{k: np.zeros(0, np.int64) for k in GENOME_COLS},
                                                    "bits": np.zeros((0, 0), np.uint64)}, [])
    z = np.load(prefix + "_fr_sites.npz")
    assert z["bits"].shape == (0, 0) and z["genomes"].shape == (0,)


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


def test_dist_entry_point_refuses_v(tmp_path):
    """The multi-process CLI: -v is single process only - the manual on rank
    0, then SystemExit, before anything is built."""
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", "record",
            "-v", "1"]
    exited, text = spawn_ranks(1, _refused_rank, (argv,))[0]
    lines = text.splitlines()
    assert exited and lines[0] == "Usage:" and sum(ln.startswith("  -v:") for ln in lines) == 1
    assert os.listdir(str(tmp_path)) == ["input.fsa"]


# ------------------------------------------------------------ the yardstick itself
def run_rows(labels, rec=0, strand=1, at=0):
    """One run: a row of length 10 + its label per label (label < 0: an unused row)."""
    return [[rec, at + 100 * i, at + 100 * i + 10 + max(l, 0), strand, l] for i, l in enumerate(labels)]


def tables(ref):
    sites = list(zip(*[ref[k] for k in SITE_COLS]))
    alleles = list(zip(*[ref[k] for k in ALLELE_COLS]))
    return sites, alleles


def test_reference_short_runs_give_no_site():
    for labels in ([5], [5, 6], [5, 6, 7]):
        ref = reference_sites(run_rows(labels), [0], 1)
        assert tables(ref) == ([], []) and reference_text(ref) == HEADER
        assert ref["n_records"] == max(0, len(labels) - 1) + max(0, len(labels) - 2) and ref["n_runs"] == 1
        assert ref["genome_sites"] == ref["genome_alleles"] == ref["genome_private"] == [0]
    # the conserved chain in two genomes: every pair has one allele
    ref = reference_sites(run_rows([5, 6, 7, 8]) + run_rows([5, 6, 7, 8], rec=1), [0, 1], 2)
    assert tables(ref) == ([], []) and ref["pairs"] == 5 and ref["n_records"] == 10


def test_reference_insertion_against_direct():
    """a x c beside a c: the site (a, c) with {*, x}."""
    rows = run_rows([1, 4, 3]) + run_rows([1, 3], rec=1)
    ref = reference_sites(rows, [0, 1], 2)
    sites, alleles = tables(ref)
    assert sites == [(1, 3, 2, 0, 2, 2)]
    assert alleles == [(0, -1, 1, 1, 0, 0), (0, 4, 1, 1, 14, 14)] and ref["bits"] == [[2], [1]]
    assert (ref["genome_sites"], ref["genome_alleles"], ref["genome_private"]) == ([1, 1], [1, 1], [1, 1])
    assert reference_text(ref) == HEADER + "1\t3\t*\t1\t1\t0\t0\n1\t3\t4\t1\t1\t14\t14\n"
    assert summary(ref) == {"n_paths": 2, "n_pairs": 3, "n_sites": 1, "sites_2_alleles": 1, "sites_3_alleles": 0,
                            "sites_4_alleles": 0, "n_alleles": 2, "sites_with_direct": 1, "sites_in_2_genomes": 1}
    # both in one genome: the same site, one genome
    ref = reference_sites(rows, [0, 0], 1)
    assert tables(ref)[0] == [(1, 3, 2, 0, 2, 1)] and ref["genome_private"] == [2]


def test_reference_substitution():
    """a x c beside a y c: {x, y}, no direct allele; the other strand's labels are other sites."""
    rows = run_rows([1, 4, 3]) + run_rows([1, 9, 3], rec=1) + run_rows([3, 4, 1], rec=1, strand=-1)
    ref = reference_sites(rows, [0, 1], 2)
    sites, alleles = tables(ref)
    assert sites == [(1, 3, 2, 0, 2, 2)]
    assert alleles == [(0, 4, 1, 1, 14, 14), (0, 9, 1, 1, 19, 19)]
    assert summary(ref)["sites_with_direct"] == 0 and ref["n_runs"] == 3


def test_reference_a_equals_c():
    rows = run_rows([6, 2, 6]) + run_rows([6, 6], rec=1) + run_rows([6, 6, 6], rec=2)
    ref = reference_sites(rows, [0, 1, 1], 2)
    sites, alleles = tables(ref)
    # (6, 6): direct once in record 1 and twice in record 2; via 2 in genome 0; via 6 (x == a == c) in genome 1
    assert sites == [(6, 6, 3, 0, 5, 2)]
    assert alleles == [(0, -1, 3, 1, 0, 0), (0, 2, 1, 1, 12, 12), (0, 6, 1, 1, 16, 16)]
    assert ref["bits"] == [[2], [1], [2]] and ref["genome_alleles"] == [1, 2] and ref["genome_private"] == [1, 2]


def test_reference_unused_row_splits_a_run():
    whole = reference_sites(run_rows([1, 4, 3]) + run_rows([1, 3], rec=1), [0, 1], 2)
    assert len(whole["site_from"]) == 1
    for rows, grp in ((run_rows([1, -1, 4, 3]) + run_rows([1, 3], rec=1), [0, 1]),
                      (run_rows([1, 4], rec=0) + run_rows([7], rec=2) + run_rows([3], rec=0) + run_rows([1, 3], rec=1),
                       [0, 1, -1])):
        ref = reference_sites(rows, grp, 2)
        assert tables(ref) == ([], []) and ref["n_skipped"] == 1
    ref = reference_sites(run_rows([1, -1, 4, 3]) + run_rows([1, 3], rec=1), [0, 1], 2)
    assert ref["n_runs"] == 3 and ref["n_records"] == 2


def test_reference_same_allele_twice_in_one_genome():
    rows = run_rows([1, 4, 3, 1, 4, 3]) + run_rows([1, 3], rec=1)
    ref = reference_sites(rows, [0, 1], 2)
    sites, alleles = tables(ref)
    assert (1, 3, 2, 0, 3, 2) in sites
    i = ref["site_from"].index(1)
    assert alleles[ref["site_first"][i] + 1] == (i, 4, 2, 1, 14, 14)
    # min and max differ when the middle rows do
    rows[4][2] += 100
    ref = reference_sites(rows, [0, 1], 2)
    assert tables(ref)[1][ref["site_first"][i] + 1] == (i, 4, 2, 1, 14, 114)


def test_pan8_oracle_rows_match_the_committed_expectation(oracle_mod):
    """pan8_k27_c3 at -a cc -w 4, one genome per record: the figures of
    tests/golden/sites/pan8_k27_c3_w4.json from the oracle's rows."""
    fx = Fixture("pan8_k27_c3")
    lines = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, cc_text("pan8_k27_c3", 4),
                                    edge_chunk=fx.edge_chunk)["rows"]
    ref = reference_sites(rows5_of(lines, fasta_names(fx.fasta)), list(range(8)), 8)
    want = golden("pan8_k27_c3_w4")
    got = summary(ref)
    assert {k: want[k] for k in got} == got
    assert (got["n_paths"], got["n_pairs"], got["n_sites"], got["n_alleles"]) == (16, 3725, 625, 1342)
    assert got["sites_2_alleles"] + got["sites_3_alleles"] + got["sites_4_alleles"] == got["n_sites"]
