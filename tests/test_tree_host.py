"""The genome tree's host side (no GPU): host.tree_nj against the independent
loops of tests/tree_util.py, additive trees recovered exactly, the tie rule,
the Newick text and its quoting, and -T's refusals."""
import io

import numpy as np
import pytest

from tree_util import (ONE, additive, as_lists, hamming, joins_as_sets, joins_of_newick, newick_leaf_dist,
                       parse_newick, reference_nj, star)


@pytest.fixture(scope="module")
def host():
    from pangenome_amd import host
    return host


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 6, 17, 40])
def test_host_equals_the_definition(host, n):
    d = hamming(n, seed=1)
    got = as_lists(*host.tree_nj(d))
    assert got == reference_nj(d.tolist())
    assert len(got[0]) == max(n - 3, 0) and len(got[1]) == min(n, 3)
    if n == 2:
        assert got[1][0][1] + got[1][1][1] == int(d[0, 1]) << 16


@pytest.mark.parametrize("seed", range(12))
def test_additive_trees_come_back_exactly(host, seed):
    n = (4, 5, 7, 8, 13, 16, 21, 25, 31, 33, 39, 40)[seed]
    d, total = additive(n, seed)
    joins, root = as_lists(*host.tree_nj(d))
    assert (joins, root) == reference_nj(d.tolist())
    lens = [v for row in joins for v in row[2:]] + [v for _, v in root]
    assert all(v % ONE == 0 for v in lens)
    assert sum(lens) == total * ONE
    names = ["g%d" % i for i in range(n)]
    text = host.tree_newick(names, *host.tree_nj(d))
    assert np.array_equal(newick_leaf_dist(text, names), d * np.uint64(1000000))


def test_tie_rule_star(host):
    joins, root = as_lists(*host.tree_nj(star(6)))
    assert joins[0][:2] == (0, 1)
    assert (joins, root) == reference_nj(star(6).tolist())


def test_refused_matrices(host):
    d = hamming(5, seed=2)
    for bad in ("asym", "diag", "big"):
        e = d.copy()
        if bad == "asym":
            e[1, 3] += 1
        elif bad == "diag":
            e[2, 2] = 1
        else:
            e[0, 4] = e[4, 0] = 2 ** 31 + 1
        with pytest.raises(ValueError):
            host.tree_nj(e)
    e = d.copy()
    e[0, 4] = e[4, 0] = 2 ** 31                              # (the limit itself is allowed)
    assert as_lists(*host.tree_nj(e)) == reference_nj(e.tolist())


def test_newick_text(host):
    assert host.tree_newick([], *host.tree_nj(np.zeros((0, 0), np.uint64))) == b""
    assert host.tree_newick([b"only"], *host.tree_nj(np.zeros((1, 1), np.uint64))) == b"(only:0.000000);\n"
    d2 = np.array([[0, 3], [3, 0]], np.uint64)
    assert host.tree_newick(["a", "b"], *host.tree_nj(d2)) == b"(a:1.500000,b:1.500000);\n"
    # a length prints cut to six decimals: 1 / 65536 = 0.0000152..
    assert host.tree_len_text(1) == b"0.000015" and host.tree_len_text((7 << 16) + 65535) == b"7.999984"
    # each join's left child before its right, nested
    d = hamming(6, seed=3)
    joins, root = host.tree_nj(d)
    names = ["n%d" % i for i in range(6)]
    text = host.tree_newick(names, joins, root)
    assert joins_of_newick(text, names) == joins_as_sets(names, as_lists(joins, root)[0], 6)
    edges, leaves = parse_newick(text)
    assert len([b for a, b, _ in edges if a == 0]) == 3
    first = as_lists(joins, root)[0][0]
    inner = "(%s:%s,%s:%s)" % (names[first[0]], host.tree_len_text(first[2]).decode(), names[first[1]],
                               host.tree_len_text(first[3]).decode())
    assert inner in text.decode()


def test_quoting_round_trip(host):
    names = ["a b", "x'y", "(z)", "plain", "tab\there", "c:d"]
    d = hamming(len(names), seed=4)
    text = host.tree_newick(names, *host.tree_nj(d))
    _, leaves = parse_newick(text)
    assert sorted(leaves.values()) == sorted(names)
    assert b"'a b'" in text and b"'x''y'" in text and b"'(z)'" in text and b"plain:" in text


@pytest.mark.parametrize("extra", [["-g", "record", "-T", "2"], ["-T", "1"], ["-g", "record", "-T", "x"],
                                   ["-g", "record", "-T", ""]])
def test_cli_refusals(extra, tmp_path):
    """Refused before anything is built: the manual, and no file written."""
    from pangenome_amd import kmer
    q = tmp_path / "in.fsa"
    q.write_bytes(b">a\nACGT\n")
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["kmer.py", "-i", str(q), "-k27", "-acc"] + extra, out=out)
    assert out.getvalue().startswith("Usage:") and "  -T:" in out.getvalue()
    assert [p.name for p in tmp_path.iterdir()] == ["in.fsa"]


def test_dist_entry_point_refuses_T(tmp_path):
    """The multi-process CLI refuses -T as it refuses -l: the manual on rank
    0, then SystemExit, before anything is built."""
    import os

    from dist_util import spawn_ranks
    from golden_util import Fixture
    from test_align_host import _refused_rank
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", "record",
            "-T", "1"]
    exited, text = spawn_ranks(1, _refused_rank, (argv,))[0]
    lines = text.splitlines()
    assert exited and lines[0] == "Usage:" and sum(ln.startswith("  -T:") for ln in lines) == 1
    assert os.listdir(str(tmp_path)) == ["input.fsa"]


def test_cli_tree_arg():
    from pangenome_amd import kmer
    args = kmer.parse_args(["x", "-i", "f"])
    assert args["-T"] == "0" and kmer.tree_arg(args) is False
    assert kmer.tree_arg(kmer.parse_args(["x", "-g", "record", "-T", "1"])) is True
    assert kmer.tree_arg(kmer.parse_args(["x", "-g", "record", "-T1"])) is True
    assert kmer.tree_arg(kmer.parse_args(["x", "-T", "1"])) is None
