"""CPU-side checks of the k-mer colours (-K): host.kmer_colors against a
brute-force set implementation, the precondition of every GPU comparison (the
union of the per-genome oracle key sets is the oracle's key set of the whole
file), -K's parsing and refusals, the manual, the multi-process refusal and
the prefixed file writers."""
import io
import os

import numpy as np
import pytest

from colors_util import CASES, brute_colors, yardstick


def as_lists(t):
    return {k: np.asarray(t[k]).tolist() for k in ("keys", "bits", "kmers_by_g", "g_kmers", "g_core", "g_shell",
                                                   "g_unique", "shared")}


# ------------------------------------------------------------ the specification
HAND = [
    ([[3, 5, 9]], 1, None),                                              # G = 1: everything is core
    ([[1, 2, 7], [2, 7, 8], [2, 9]], 3, None),                           # key 2 in all genomes
    ([[1, 2], [2, 3]], 2, [0, 1, 2, 3, 2 ** 64 - 2]),                    # keys 0 and 2^64 - 2 in none
    ([[4], []], 2, None),                                                # an empty genome
    ([], 0, None),
]


@pytest.mark.parametrize("sets,G,keys", HAND)
def test_kmer_colors_hand(sets, G, keys):
    from pangenome_amd import host
    got = host.kmer_colors([np.array(s, np.uint64) for s in sets], G, keys=None if keys is None else np.array(keys, np.uint64))
    assert as_lists(got) == brute_colors(sets, G, keys)
    assert got["bits"].shape == (len(got["keys"]), (G + 63) // 64) and got["bits"].dtype == np.uint64


def test_kmer_colors_hand_values():
    from pangenome_amd import host
    t = host.kmer_colors([np.array(s, np.uint64) for s in ([1, 2], [2, 3])], 2, keys=np.array([0, 1, 2, 3], np.uint64))
    assert t["keys"].tolist() == [0, 1, 2, 3] and t["bits"].reshape(-1).tolist() == [0, 1, 3, 2]
    assert t["kmers_by_g"].tolist() == [1, 2, 1]
    assert (t["g_kmers"].tolist(), t["g_core"].tolist(), t["g_shell"].tolist(), t["g_unique"].tolist()) == \
        ([2, 2], [1, 1], [0, 0], [1, 1])
    assert t["shared"].tolist() == [[2, 1], [1, 2]]
    one = host.kmer_colors([np.array([5, 6], np.uint64)], 1)
    assert one["g_core"].tolist() == [2] and one["g_unique"].tolist() == [0] and one["kmers_by_g"].tolist() == [0, 2]
    with pytest.raises(ValueError):
        host.kmer_colors([np.zeros(0, np.uint64)], 2)


def test_kmer_colors_65_genomes():
    """G = 65: the second word holds genome 64 alone and no bit above it."""
    from pangenome_amd import host
    rng = np.random.default_rng(65)
    sets = [np.unique(rng.integers(0, 90, 40).astype(np.uint64)) for _ in range(65)]
    sets[64] = np.array([3, 89, 200], np.uint64)
    got = host.kmer_colors(sets, 65)
    assert as_lists(got) == brute_colors([s.tolist() for s in sets], 65)
    assert got["bits"].shape[1] == 2 and not (got["bits"][:, 1] >> np.uint64(1)).any()
    assert int(got["bits"][got["keys"].tolist().index(200), 1]) == 1
    assert int(got["g_kmers"].sum()) == sum(len(s) for s in sets) and int(got["kmers_by_g"].sum()) == len(got["keys"])
    assert np.array_equal(got["g_core"] + got["g_shell"] + got["g_unique"], got["g_kmers"])


def test_kmer_distance_limit():
    from pangenome_amd import host
    s = np.array([[5, 2], [2, 4]], np.uint64)
    assert host.kmer_distance(s).tolist() == [[0, 5], [5, 0]]
    big = np.array([[2 ** 31 + 1, 0], [0, 0]], np.uint64)
    with pytest.raises(ValueError, match="2\\^31"):
        host.kmer_distance(big)


# ------------------------------------------------------------ the GPU tests' inputs
@pytest.mark.parametrize("name,k,c", CASES, ids=["%s-k%d-c%d" % x for x in CASES])
def test_union_of_genome_key_sets_is_the_files(oracle_mod, name, k, c):
    """What the colour comparisons rest on: the dBG of the file is the union of
    the dBGs of its genomes' records (no key spans two records)."""
    sets, whole = yardstick(name, k, c)
    assert np.array_equal(np.unique(np.concatenate(sets)), whole)
    assert all(s.shape[0] for s in sets)


# ------------------------------------------------------------ the CLI
def _refused(tmp_path, extra):
    from pangenome_amd import kmer
    q = str(tmp_path / "input.fsa")
    open(q, "wb").write(b">a\nACGTACGTAC\n")
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["kmer_numba.py", "-i", q, "-k", "5"] + extra, out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert os.listdir(str(tmp_path)) == ["input.fsa"]            # nothing is written on a refusal


@pytest.mark.parametrize("extra", [["-K", "2"], ["-K", "yes"], ["-K", ""], ["-K", "1"], ["-K1"],
                                   ["-K", "1", "-g", "record", "-D", "x_rdb.npz"]])
def test_cli_refuses(tmp_path, extra):
    _refused(tmp_path, extra)


def test_kmers_arg():
    from pangenome_amd import kmer
    args = kmer.parse_args(["x", "-i", "f"])
    assert args["-K"] == "0" and kmer.kmers_arg(args) is False
    assert kmer.kmers_arg(kmer.parse_args(["x", "-i", "f", "-K", "1", "-g", "record"])) is True
    assert kmer.kmers_arg(kmer.parse_args(["x", "-i", "f", "-K1", "-g", "groups.tsv", "-d", "x_db.npz"])) is True
    assert kmer.kmers_arg(kmer.parse_args(["x", "-i", "f", "-K", "1"])) is None
    assert kmer.kmers_arg(kmer.parse_args(["x", "-i", "f", "-K", "1", "-g", "record", "-D", "r.npz"])) is None
    assert kmer.kmers_arg(kmer.parse_args(["x", "-i", "f", "-K", "01", "-g", "record"])) is None


def test_manual_has_the_K_lines():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("  -K:")]
    assert len(at) == 1 and "with -g" in lines[at[0]] and lines[at[0] + 4].startswith("  -D:")
    text = "".join(lines[at[0]:at[0] + 4])
    assert all(ln.startswith("      ") for ln in lines[at[0] + 1:at[0] + 4]) and "single process only" in text
    for name in ("<in>_km_spectrum.tsv", "_km_genomes.tsv", "_km_shared.tsv", "_km_jaccard.tsv", "_km_compare.npz",
                 "_km_curve.tsv", "_km_dist.tsv", "_km_tree.nwk", "_km_tree.tsv", "_km_tree.npz"):
        assert name in text
    assert sum("_km_" in ln for ln in lines) == 2 and "-K" in kmer.__doc__.split("ours:")[1].split(")")[0].split()


def test_dist_entry_point_refuses_K(tmp_path):
    """The multi-process CLI refuses -K as it refuses -l: the manual on rank
    0, then SystemExit, before anything is built."""
    from dist_util import spawn_ranks
    from golden_util import Fixture
    from test_align_host import _refused_rank
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", "record",
            "-K", "1"]
    exited, text = spawn_ranks(1, _refused_rank, (argv,))[0]
    lines = text.splitlines()
    assert exited and lines[0] == "Usage:" and sum(ln.startswith("  -K:") for ln in lines) == 1
    assert os.listdir(str(tmp_path)) == ["input.fsa"]


# ------------------------------------------------------------ the writers
def test_write_kmer_files(tmp_path):
    from pangenome_amd import host
    p = str(tmp_path / "in.fa")
    t = {"kmers_by_g": np.array([1, 2 ** 40, 3], np.uint64), "g_kmers": np.array([7, 2 ** 33], np.uint64),
         "g_core": np.array([3, 3], np.uint64), "g_shell": np.array([0, 1], np.uint64),
         "g_unique": np.array([4, 2 ** 33 - 4], np.uint64)}
    host.write_kmer_files(p, t, [b"gA", b"g B"])
    assert open(p + "_km_spectrum.tsv").read() == "#genomes\tkmers\n0\t1\n1\t%d\n2\t3\n" % 2 ** 40
    assert open(p + "_km_genomes.tsv", "rb").read() == (b"#genome\tkmers\tcore\tshell\tunique\ngA\t7\t3\t0\t4\n"
                                                        b"g B\t%d\t3\t1\t%d\n" % (2 ** 33, 2 ** 33 - 4))
    assert sorted(os.listdir(str(tmp_path))) == ["in.fa_km_genomes.tsv", "in.fa_km_spectrum.tsv"]


def test_prefixed_compare_and_tree_writers(tmp_path):
    """tag = "_km_": the same bytes as the `_fr_` files under the other names;
    curve False: no curve file; the default still writes the `_fr_` names."""
    from pangenome_amd import host
    names = [b"a", b"b", b"c", b"d"]
    shared = np.array([[5, 2, 1, 0], [2, 4, 1, 0], [1, 1, 3, 0], [0, 0, 0, 0]], np.uint64)
    orders = host.compare_orders(4, 2)
    pan = np.array([[5, 7, 8, 8], [3, 7, 8, 8]], np.uint64)
    core = np.array([[5, 2, 1, 0], [3, 1, 1, 0]], np.uint64)
    fr, km, nc = str(tmp_path / "fr" / "x"), str(tmp_path / "km" / "x"), str(tmp_path / "nc" / "x")
    for d in ("fr", "km", "nc"):
        os.mkdir(str(tmp_path / d))
    host.write_compare_files(fr, names, shared, orders, pan, core)
    host.write_compare_files(km, names, shared, orders, pan, core, tag="_km_")
    host.write_compare_files(nc, names, shared, orders, pan, core, tag="_km_", curve=False)
    d = host.kmer_distance(shared)
    joins, root = host.tree_nj(d)
    host.write_tree_files(fr, names, d, joins, root)
    host.write_tree_files(km, names, d, joins, root, tag="_km_")
    want = ["x_fr_" + s for s in ("compare.npz", "curve.tsv", "dist.tsv", "jaccard.tsv", "shared.tsv", "tree.npz",
                                  "tree.nwk", "tree.tsv")]
    assert sorted(os.listdir(str(tmp_path / "fr"))) == want
    assert sorted(os.listdir(str(tmp_path / "km"))) == [w.replace("_fr_", "_km_") for w in want]
    assert sorted(os.listdir(str(tmp_path / "nc"))) == ["x_km_compare.npz", "x_km_jaccard.tsv", "x_km_shared.tsv"]
    for w in want:
        a, b = str(tmp_path / "fr" / w), str(tmp_path / "km" / w.replace("_fr_", "_km_"))
        if w.endswith(".npz"):
            za, zb = np.load(a), np.load(b)
            assert sorted(za.files) == sorted(zb.files) and all(np.array_equal(za[k], zb[k]) for k in za.files)
        else:
            assert open(a, "rb").read() == open(b, "rb").read()
    assert open(km + "_km_shared.tsv", "rb").read().split(b"\n")[1] == b"a\t5\t2\t1\t0"
    assert open(km + "_km_dist.tsv", "rb").read().split(b"\n")[2] == b"b\t5\t0\t5\t4"
    assert open(km + "_km_tree.nwk", "rb").read() == host.tree_newick(names, joins, root)
