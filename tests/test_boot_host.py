"""host.tree_bootstrap (the specification pg_tree_bootstrap equals) against
tests/boot_util.py's loops, the properties of the definition, the labelled
Newick text and -B's arguments; no device."""
import functools
import io

import numpy as np
import pytest

from boot_util import (MASK, clades, clean_table, coin_table, draw, index_of, labels_by_clade, mixed_table,
                       parse_newick_labels, reference_bootstrap, rows_as_ints, splitmix_one, star_table, table_dist)
from tree_util import parse_newick

from pangenome_amd import host, kmer, synth

SEED = synth.DEFAULT_SEED


def lr(joins):
    return [(int(a), int(b)) for a, b in zip(joins["left"], joins["right"])]


@functools.lru_cache(maxsize=None)
def rated(kind):
    """(bits, G, joins, root) of a table and its own tree."""
    bits, G = {"clean12": (lambda: clean_table(12, 40), 12), "clean70": (lambda: clean_table(70, 8), 70),
               "coin20": (lambda: coin_table(600, 20, seed=1), 20), "mixed20": (mixed_table, 20),
               "small7": (lambda: coin_table(45, 7, seed=3), 7), "small9": (lambda: coin_table(90, 9, seed=4), 9),
               "star6": (lambda: star_table(6), 6), "star70": (lambda: star_table(70, 100), 70)}[kind]
    bits = bits()
    joins, root = host.tree_nj(table_dist(bits, G))
    return bits, G, joins, root


@pytest.mark.parametrize("kind,R", [("small7", 5), ("small9", 4), ("star6", 3)])
def test_equals_the_reference(kind, R):
    bits, G, joins, _ = rated(kind)
    got = host.tree_bootstrap(bits, G, joins, R, SEED, dist=table_dist(bits, G), rep_dist=True)
    support, rep_joins, rep_dist = reference_bootstrap(rows_as_ints(bits, G), G, lr(joins), R, SEED)
    assert got["support"].tolist() == support and got["support"].dtype == np.uint32
    assert [list(zip(a.tolist(), b.tolist())) for a, b in zip(got["rep_left"], got["rep_right"])] == rep_joins
    assert got["rep_dist"].tolist() == rep_dist
    if kind == "star6":                                       # every d_b equal: the smallest live pair, every time
        assert all(rj == [(0, 1), (6, 2), (7, 3)] for rj in rep_joins) and support == [R, R, R]


def test_draws():
    for L in (1, 3, 2 ** 31):
        for x in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, MASK - 1, MASK, splitmix_one(SEED, 1, 0)):
            i = index_of(x, L)
            assert 0 <= i < L
            assert int(host.boot_index(np.array([x], np.uint64), L)[0]) == i
    assert index_of(MASK, 2 ** 31) == 2 ** 31 - 1
    with pytest.raises(ValueError):
        host.boot_index(np.zeros(1, np.uint64), 2 ** 31 + 1)
    for L in (1, 3, 1000):
        got = host.boot_draws(SEED, 2, L).tolist()
        assert got == [draw(SEED, 2, t, L) for t in range(L)] and all(0 <= v < L for v in got)
    assert host.boot_draws(SEED, 0, 0).shape == (0,)
    assert len(set(host.boot_draws(SEED, 0, 1000).tolist())) > 500          # (about 632 of 1000 are drawn at all)
    assert host.boot_draws(SEED, 0, 50).tolist() != host.boot_draws(SEED, 1, 50).tolist()


@pytest.mark.parametrize("kind", ["clean12", "clean70"])
def test_clean_tables_are_fully_supported(kind):
    bits, G, joins, _ = rated(kind)
    got = host.tree_bootstrap(bits, G, joins, 8, SEED)
    assert got["support"].tolist() == [8] * (G - 3)


def test_coin_flips_and_the_mixed_table_spread():
    bits, G, joins, _ = rated("coin20")
    s = host.tree_bootstrap(bits, G, joins, 16, SEED)["support"]
    assert int(s.min()) < 16
    bits, G, joins, _ = rated("mixed20")
    s = host.tree_bootstrap(bits, G, joins, 16, SEED)["support"]
    assert int(s.min()) < 16 and int(s.max()) > 0


def test_no_labels_and_few_genomes():
    for G in (1, 2, 3):
        bits = coin_table(10, G, seed=G)
        joins, _ = host.tree_nj(table_dist(bits, G))
        got = host.tree_bootstrap(bits, G, joins, 3, SEED)
        assert got["support"].shape == (0,) and got["rep_left"].shape == (3, 0)
    joins, _ = host.tree_nj(np.zeros((5, 5), np.uint64))
    got = host.tree_bootstrap(np.zeros((0, 1), np.uint64), 5, joins, 3, SEED, rep_dist=True)
    assert not got["rep_dist"].any() and got["support"].tolist() == [3, 3]     # the star's tie rule, every time


def test_refusals():
    bits, G, joins, _ = rated("small7")
    for R in (0, 4097):
        with pytest.raises(ValueError):
            host.tree_bootstrap(bits, G, joins, R, SEED)
    bad = bits.copy()
    bad[3, 0] |= np.uint64(1 << 7)
    with pytest.raises(ValueError):
        host.tree_bootstrap(bad, G, joins, 2, SEED)
    other = coin_table(45, 7, seed=9)
    with pytest.raises(ValueError, match="not built from this table"):
        host.tree_bootstrap(other, G, joins, 2, SEED, dist=table_dist(bits, G))
    with pytest.raises(ValueError):
        host.tree_bootstrap(coin_table(30, 8), 8, joins, 2, SEED)            # another number of joins


@pytest.mark.parametrize("kind", ["clean12", "mixed20", "small7"])
def test_newick_with_support(kind):
    bits, G, joins, root = rated(kind)
    names = ["g%d" % i for i in range(G)]
    plain = host.tree_newick(names, joins, root)
    assert host.tree_newick(names, joins, root, support=None) == plain
    R = 16
    sup = host.tree_bootstrap(bits, G, joins, R, SEED)["support"]
    text = host.tree_newick(names, joins, root, support=(sup, R))
    # the same topology and lengths
    e0, l0 = parse_newick(plain)
    e1, l1, labels = parse_newick_labels(text)
    assert e1 == e0 and l1 == l0
    assert parse_newick_labels(plain)[2] == {}
    # every join's percentage on its own node, none on the root
    want = {frozenset(names[i] for i in c): "%d" % (100 * int(s) // R) for c, s in zip(clades(lr(joins), G), sup)}
    got = labels_by_clade(text)
    assert {k: v[0] for k, v in got.items()} == want and 0 not in labels
    assert {k: v[1] for k, v in got.items()} == {k: v[1] for k, v in labels_by_clade(plain).items()}


def test_support_files(tmp_path):
    bits, G, joins, root = rated("mixed20")
    names = [b"g%d" % i for i in range(G)]
    boot = host.tree_bootstrap(bits, G, joins, 6, SEED)
    p = str(tmp_path / "x")
    host.write_tree_support_files(p, names, joins, root, boot, SEED)
    host.write_tree_support_files(p, names, joins, root, boot, SEED, var=True)
    import os
    assert sorted(os.listdir(tmp_path)) == ["x_fr_tree_boot.npz", "x_fr_tree_support.nwk", "x_fr_tree_support.tsv",
                                            "x_fr_vartree_support.nwk", "x_fr_vartree_support.tsv"]
    assert open(p + "_fr_tree_support.nwk", "rb").read() == host.tree_newick(names, joins, root, (boot["support"], 6))
    tsv = open(p + "_fr_tree_support.tsv").read().split("\n")
    assert tsv[0] == "#node\tsupport\treplicates\tleaves" and tsv[-1] == ""
    sizes = [len(c) for c in clades(lr(joins), G)]
    assert [ln.split("\t") for ln in tsv[1:-1]] == [
        [str(G + t), str(int(s)), "6", str(k)] for t, (s, k) in enumerate(zip(boot["support"], sizes))]
    z = np.load(p + "_fr_tree_boot.npz")
    assert sorted(z.files) == ["genomes", "rep_left", "rep_right", "replicates", "seed", "support"]
    assert int(z["replicates"]) == 6 and int(z["seed"]) == SEED and z["rep_left"].shape == (6, G - 3)
    assert np.array_equal(z["support"], boot["support"]) and z["support"].dtype == np.uint32


@pytest.mark.parametrize("extra", [["-g", "record", "-B", "3"], ["-g", "record", "-T", "1", "-B", "x"],
                                   ["-g", "record", "-T", "1", "-B", "4097"], ["-g", "record", "-T", "1", "-B", "-1"],
                                   ["-g", "record", "-T", "0", "-B", "2"]])
def test_refused_arguments_print_the_manual(extra):
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["kmer_numba.py", "-i", "nothing.fsa", "-k27", "-acc"] + extra, out=out)
    assert out.getvalue().startswith("Usage:") and "  -B:" in out.getvalue()


def test_boot_argument():
    args = kmer.parse_args(["x"])
    assert args["-B"] == "0" and kmer.boot_arg(args, False) == 0
    assert kmer.boot_arg(kmer.parse_args(["x", "-B", "16"]), True) == 16
    assert kmer.boot_arg(kmer.parse_args(["x", "-B4096"]), True) == 4096
    assert kmer.boot_arg(kmer.parse_args(["x", "-B", "16"]), False) is None
    assert kmer.boot_arg(kmer.parse_args(["x", "-B", "1.5"]), True) is None
