"""Markov clustering's specification, host.cluster_markov, against an
independent dense restatement of the definition (tests/markov_util.py), the
hand cases, the committed expectations of the pan8_k27_c3 fixture, and the
command line's parsing of -a markov and -I."""
import gzip
import io
import json
import os

import numpy as np
import pytest

from cc_util import random_graph, xyz_arrays
from golden_util import GOLDEN, Fixture
import markov_util as mu

MK = os.path.join(GOLDEN, "markov")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_as_dense(t, c, w, i2, sel):
    from pangenome_amd import host
    for mi in (0, 1, 2, 200):
        d_text, d_iter, d_chaos, d_matrix = mu.dense_markov(t, c, w, i2, sel, mi)
        text, keys, vals, line, n_iter, chaos, matrix = host.cluster_markov(t, c, w, i2, sel, mi)
        assert (n_iter, chaos) == (d_iter, d_chaos), (w, i2, sel, mi)
        assert mu.matrix_lists(matrix) == d_matrix, (w, i2, sel, mi)
        assert matrix[1].shape == (len(d_matrix[0]), sel) and matrix[1].dtype == np.uint32
        assert text == d_text, (w, i2, sel, mi)
        mk, mv, mi_, n_lines = host.mcl_labels(text)             # the label table is the written file's
        assert np.array_equal(keys, mk) and np.array_equal(vals, mv) and np.array_equal(line, mi_)
    return text


@pytest.mark.parametrize("seed", range(20))
def test_specification_equals_dense_restatement(seed):
    U = 8 + (seed * 56) // 19                                    # 8 .. 64 nodes
    t, c = random_graph(seed, U, U + (seed % 4) * U // 2)
    for i2, sel, w in mu.GRID:
        same_as_dense(t, c, w, i2, sel)


@pytest.mark.parametrize("name", sorted(mu.hand_cases()))
def test_hand_cases(name):
    t, c, clusters = mu.hand_cases()[name]
    for i2, sel, w in mu.GRID:
        text = same_as_dense(t, c, w, i2, sel)
        if (i2, sel, w) == (3, 64, 1):
            assert text == mu.text_of(clusters)


@pytest.mark.parametrize("i2", [3, 39, 40])
def test_inflation_arithmetic(i2):
    """weights over 1 .. 2^31: the scaled values run from below 2^7 to ONE (tests/test_gpu_markov.py has the
    same graph for the device)"""
    t, c = mu.inflation_graph()
    same_as_dense(t, c, 1, i2, 64)
    same_as_dense(t, c, 1, i2, 5)


def test_hand_values():
    """the weights add over both directions; the loop is the column's largest; prune's arithmetic by hand"""
    from pangenome_amd import host
    t, c, _ = mu.hand_cases()["both_directions"]                 # w(0,1) = 2, w(1,2) = 1
    col_len, rows, vals = host.cluster_markov(t, c, max_iter=0)[6]
    assert col_len.tolist() == [2, 3, 2]
    assert rows[1, :3].tolist() == [0, 1, 2]
    n = [(2 << 31) // 5, (2 << 31) // 5, (1 << 31) // 5]         # column 1: weights 2, loop 2, 1
    assert vals[1, :3].tolist() == [(x << 31) // sum(n) for x in n]
    assert vals[0, :2].tolist() == [mu.ONE // 2, mu.ONE // 2] and vals[2, :2].tolist() == [mu.ONE // 2, mu.ONE // 2]
    z = host.cluster_markov(np.zeros((0, 4), np.uint64), np.zeros(0, np.int64))
    assert z[0] == "" and z[4:6] == (0, 0) and z[6][1].shape == (0, 64)
    one = host.cluster_markov([[7, 1, 7, 1]], [9])               # a self-loop only: one node, its loop of 1
    assert one[0] == "7_1\n" and one[6][2][0, 0] == mu.ONE
    # a light edge's ends are still nodes
    assert host.cluster_markov([[1, 0, 2, 0], [2, 0, 3, 0]], [5, 1], min_weight=2)[0] == "1_0\t2_0\n3_0\n"


def test_refusals():
    from pangenome_amd import host
    t = mu.tuples_of([[0, 1], [1, 0], [1, 2]])
    with pytest.raises(OverflowError):                           # a weight sum of exactly 2^32
        host.cluster_markov(t, [2 ** 31, 2 ** 31, 1])
    assert host.cluster_markov(t, [2 ** 31, 2 ** 31 - 1, 1], max_iter=1)[4] == 1
    with pytest.raises(OverflowError):
        mu.dense_markov(t, [2 ** 31, 2 ** 31, 1])
    for kw in (dict(min_weight=0), dict(inflation2=2), dict(inflation2=41), dict(select=0), dict(select=65),
               dict(max_iter=-1), dict(max_iter=10001)):
        with pytest.raises(ValueError):
            host.cluster_markov(t, [1, 1, 1], **kw)


def figures(text, n_iter, chaos):
    sizes = [ln.count("\t") + 1 for ln in text.splitlines()]
    return {"nodes": sum(sizes), "iterations": n_iter, "chaos": chaos, "clusters": len(sizes), "largest": max(sizes),
            "singletons": sizes.count(1)}


def test_pan8_fixture():
    """The committed expectations were written once by this same yardstick,
    host.cluster_markov (tests/golden/make_markov_goldens.py); the device and
    the command line are held to them in tests/test_gpu_markov.py.  The
    README's table of the fixture must hold."""
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    t, c = xyz_arrays(fx.xyz)
    gold = json.load(open(os.path.join(MK, "pan8_k27_c3.json")))
    r3 = host.cluster_markov(t, c)
    assert r3[0] == gzip.open(os.path.join(MK, "pan8_k27_c3_I3.mcl.gz")).read().decode()
    assert figures(r3[0], r3[4], r3[5]) == gold["inflation2_3"]
    r4 = host.cluster_markov(t, c, inflation2=4)
    assert figures(r4[0], r4[4], r4[5]) == gold["inflation2_4"]
    g3, g4 = gold["inflation2_3"], gold["inflation2_4"]
    assert (g3["nodes"], g3["iterations"], g3["clusters"], g3["largest"], g3["singletons"]) == (10205, 40, 520, 38, 0)
    assert (g4["iterations"], g4["clusters"], g4["largest"], g4["singletons"]) == (28, 1462, 26, 18)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "| 1 | 1.5 | 40 | 520 | 38 | 0 |" in readme and "| 1 | 2.0 | 28 | 1,462 | 26 | 18 |" in readme


def test_big_column_digest():
    """regenerates tests/golden/markov/bigcol.json, the expectation of the device's block class"""
    from pangenome_amd import host
    gold = json.load(open(os.path.join(MK, "bigcol.json")))
    t, c = mu.bigcol()
    m0 = host.cluster_markov(t, c, 1, 3, 64, 0)[6]
    assert int(mu.candidates(m0).max()) == gold["max_candidates"] == 4096
    assert mu.matrix_digest(host.cluster_markov(t, c, 1, 3, 64, 1)[6]) == gold["sha256"]


# ------------------------------------------------------------ command line
def test_parse_inflation():
    from pangenome_amd.kmer import cluster_args, inflation_arg, parse_args
    assert parse_args(["x"])["-I"] == "1.5" and inflation_arg(parse_args(["x"])) == 3
    assert inflation_arg(parse_args(["x", "-I", "2"])) == 4 and inflation_arg(parse_args(["x", "-I1.5"])) == 3
    assert inflation_arg(parse_args(["x", "-I", "2.50"])) == 5 and inflation_arg(parse_args(["x", "-I", "20"])) == 40
    assert inflation_arg(parse_args(["x", "-I", "20.0"])) == 40
    for bad in ("1", "1.25", "21", "x", "20.5", "-2", "1.5x", ""):
        assert inflation_arg(parse_args(["x", "-I", bad])) is None, bad
    a = parse_args(["x", "-i", "f.fa", "-amarkov", "-w2", "-I2"])
    assert cluster_args(a) == dict(cluster="markov", min_weight=2, inflation2=4)
    assert cluster_args(parse_args(["x", "-a", "markov"])) == dict(cluster="markov", min_weight=1, inflation2=3)
    assert cluster_args(parse_args(["x", "-a", "markov", "-w", "auto"])) is None
    # -I is read with -a markov alone
    assert cluster_args(parse_args(["x", "-I", "x"])) == {}
    assert cluster_args(parse_args(["x", "-a", "cc", "-I", "x", "-w", "auto"])) == dict(cluster="cc", min_weight="auto")


@pytest.mark.parametrize("extra", [["-I", "1"], ["-I", "1.25"], ["-I", "21"], ["-I", "x"], ["-w", "auto"]])
def test_bad_markov_arguments_print_the_manual(tmp_path, extra):
    from pangenome_amd import kmer
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["x", "-i", str(tmp_path / "missing.fa"), "-k27", "-a", "markov"] + extra, out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-1].startswith("  -w:")
    assert os.listdir(str(tmp_path)) == []


def test_manual():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    assert lines[-3] == "  -c: complementary reverse sequence. 00,01,10,11"
    assert lines[-2].startswith("  -a:") and "markov" in lines[-2] and "mcl" in lines[-2] and " cc " in lines[-2]
    assert lines[-1].startswith("  -w:") and "markov" in lines[-1]
    at = [i for i, ln in enumerate(lines) if ln.startswith("  -I:")]
    assert len(at) == 1 and at[0] < len(lines) - 3 and "1.5" in lines[at[0]] and "-a markov" in lines[at[0]]


def test_markov_note():
    from pangenome_amd import host
    assert host.markov_note(40, 1062428) is None and host.markov_note(200, host.MK_STOP) is None
    assert host.markov_note(200, mu.ONE // 4) == "# -a markov: not converged after 200 iterations (chaos 0.250000)"


def test_binding_marshals_markov_entry_points():
    """The ctypes argument lists accept what the Context methods pass (a NULL
    context: PG_EINVAL, no device touched)."""
    from pangenome_amd import _lib
    lib = _lib.load()

    class Fake:
        pass
    f = Fake()
    f.lib, f.h = lib, None
    t, c = random_graph(1, 10, 5)
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_markov failed \(-22\)"):
        _lib.Context.cluster_markov(f, t, c, 2, 4, 8, 10)
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_markov failed \(-22\)"):
        _lib.Context.cluster_markov(f)
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_markov_matrix failed \(-22\)"):
        _lib.Context.cluster_markov_matrix(f)
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_markov_stats failed \(-22\)"):
        _lib.Context.cluster_markov_stats(f)
