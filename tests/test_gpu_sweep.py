"""The cluster curve on the device (pg_cluster_sweep, pangenome_amd/csrc/
pg_cluster.hip): one union-find kept from the highest threshold down, the
figures of every level reduced on the device.

Every case compares all four arrays, exactly, with an independent union-find
made from scratch per threshold (tests/sweep_util.py).  The synthetic shapes
are the smallest at which each mechanism can go wrong; the pipeline case runs
the CLI with `-a cc -w auto`.
"""
import ctypes as C
import io

import numpy as np
import pytest

from cc_util import random_graph, reference_mcl, xyz_arrays
from golden_util import Fixture
from sweep_util import as_lists, golden_sweep, reference_sweep, sweep_file_text

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


def rows_of(text):
    return [ln for ln in text.split("\n") if len(ln.split("\t")) == 5 and ln.split("\t")[3] in ("+", "-")]


def tuples_of(pairs):
    """Edges between abstract node numbers -> (key, value) tuples: distinct
    64-bit keys (an odd multiplier is a bijection mod 2^64), small values."""
    p = np.asarray(pairs, np.uint64).reshape(-1, 2)
    key = p * np.uint64(0x9E3779B97F4A7C15)
    val = p % np.uint64(7)
    return np.stack([key[:, 0], val[:, 0], key[:, 1], val[:, 1]], axis=1)


def check(ctx, t, c, thr):
    t = np.asarray(t, np.uint64).reshape(-1, 4)
    c = np.asarray(c, np.int64)
    want = reference_sweep(t, c, thr)
    got = as_lists(ctx.cluster_sweep(thr, t, c))
    assert got == want
    n_nodes = len({(int(k), int(v)) for k, v in t.reshape(-1, 2).tolist()})
    assert ctx.cluster_weights(t, c) == (n_nodes, int(c.max()) if c.shape[0] else 0)
    return got


def test_no_edges(ctx):
    got = check(ctx, np.zeros((0, 4), np.uint64), np.zeros(0, np.int64), [1, 2, 9])
    assert got["clusters"] == [0, 0, 0] and got["largest"] == [0, 0, 0]


def test_one_edge(ctx):
    got = check(ctx, [[5, 0, 8, 0]], [3], [1, 3, 4])
    assert (got["edges"], got["clusters"], got["largest"], got["singletons"]) == ([1, 1, 0], [1, 1, 2], [2, 2, 1], [0, 0, 2])


def test_one_self_loop(ctx):
    got = check(ctx, [[2 ** 64 - 1, 5, 2 ** 64 - 1, 5]], [3], [1, 4])
    assert (got["edges"], got["clusters"], got["largest"], got["singletons"]) == ([1, 0], [1, 1], [1, 1], [1, 1])


def test_one_key_two_values(ctx):
    got = check(ctx, [[5, 0, 8, 0], [5, 1, 9, 0]], [1, 2], [1, 2, 3])
    assert got["clusters"] == [2, 3, 4]


def test_thresholds_above_every_weight(ctx):
    t, c = random_graph(21, 300, 500, 5)
    got = check(ctx, t, c, [6, 7, 100])
    assert got["edges"] == [0, 0, 0] and got["largest"] == [1, 1, 1] and got["clusters"] == got["singletons"]


def test_single_threshold(ctx):
    t, c = random_graph(22, 300, 500, 5)
    check(ctx, t, c, [1])


@pytest.mark.parametrize("thr", [[2, 5], [1, 2, 3, 4, 5, 6]])
def test_bands(ctx, thr):
    """Weights 1..6: [2, 5] makes a level of several weights (2, 3, 4) and
    leaves weight 1 below every level."""
    t, c = random_graph(23, 400, 700, 6)
    assert sorted(set(c.tolist())) == [1, 2, 3, 4, 5, 6]
    check(ctx, t, c, thr)
    assert ctx.cluster_weights(t, c)[1] == 6


def test_path_grows_level_by_level(ctx):
    """70,000 nodes in one path numbered in walk order, weights cycling 1..4:
    274 blocks; every level joins the chains the level above left, so the
    finds start from the flattened array and the trees deepen again."""
    n = 70_000
    i = np.arange(n - 1)
    t, c = tuples_of(np.stack([i, i + 1], axis=1)), (i % 4 + 1).astype(np.int64)
    got = check(ctx, t, c, [1, 2, 3, 4, 5])
    assert got["largest"][0] == n and got["clusters"][0] == 1 and got["clusters"][4] == n


def test_hot_root(ctx):
    """A star of 20,000 leaves at weight 3 and 5,000 isolated light edges:
    the size pass with one root holding most nodes."""
    leaves = np.arange(1, 20_001)
    star = np.stack([np.zeros(20_000, np.int64), leaves], axis=1)
    light = np.arange(20_001, 30_001).reshape(5000, 2)
    e = np.concatenate([star, light])
    c = np.concatenate([np.full(20_000, 3), np.ones(5000)]).astype(np.int64)
    o = np.random.default_rng(5).permutation(e.shape[0])
    got = check(ctx, tuples_of(e[o]), c[o], [1, 2, 3, 4])
    assert got["largest"] == [20_001, 20_001, 20_001, 1] and got["clusters"] == [5001, 10_001, 10_001, 30_001]


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_random_graphs(ctx, seed):
    t, c = random_graph(seed, 3000, 5000, 5)           # 5,000 edges: no multiple of the block size
    check(ctx, t, c, [1, 2, 3, 4, 5, 6])


def test_agrees_with_the_clusterer(ctx):
    t, c = random_graph(34, 3000, 5000, 5)
    thr = [1, 2, 3, 4, 5, 6]
    got = ctx.cluster_sweep(thr, t, c)
    for i, w in enumerate(thr):
        n_clusters, _ = ctx.cluster_cc(t, c, w)
        assert int(got["clusters"][i]) == n_clusters
        assert int(got["largest"][i]) == ctx.clusters_text().split(b"\n")[0].count(b"\t") + 1


def test_a_sweep_is_a_pure_query(ctx):
    from pangenome_amd._lib import Context, PangenomeError
    t, c = random_graph(35, 3000, 5000, 5)
    ctx.cluster_cc(t, c, 2)
    text, labels, gen = ctx.clusters_text(), ctx.labels(), ctx.label_gen
    other = random_graph(36, 500, 900, 5)
    ctx.cluster_sweep([1, 3, 6], *other)
    ctx.cluster_weights(*other)
    assert ctx.clusters_text() == text and ctx.label_gen == gen
    assert all(np.array_equal(a, b) for a, b in zip(ctx.labels(gen), labels))
    fresh = Context(27, 0)
    try:
        fresh.cluster_sweep([1, 3, 6], *other)
        with pytest.raises(PangenomeError, match=r"pg_clusters_format failed \(-22\)"):
            fresh.clusters_text()
    finally:
        fresh.close()


def test_device_edges_equal_host_edges(ctx):
    """tuples=None sweeps the last edge pass where it lies on the device."""
    fx = Fixture("pan8_k27_c3")
    ctx.parse_host(np.frombuffer(fx.fasta, np.uint8))
    ctx.build_dbg(None, 0, True)
    ctx.build_rdbg()
    assert ctx.edges_count(None, True) == fx.meta["n_edges"]
    want = golden_sweep()
    assert ctx.cluster_weights() == (10205, 7)
    assert as_lists(ctx.cluster_sweep(want["w"])) == want
    t, c, _ = ctx.edges_export()
    assert check(ctx, t, c, want["w"]) == want


def test_argument_errors(ctx):
    """Refused before any launch, and the context stays usable."""
    from pangenome_amd._lib import Context, PangenomeError, ptr
    t, c = random_graph(37, 50, 80)
    t = np.ascontiguousarray(t)
    thr = np.array([1, 3], np.int64)
    out = np.zeros(2, np.uint64)

    def usable():
        assert as_lists(ctx.cluster_sweep([1, 3], t, c)) == reference_sweep(t, c, [1, 3])
    for bad in ([0], [-2, 1], [2, 2], [3, 1], [1, 2, 2], list(range(1, 4098))):
        with pytest.raises(PangenomeError, match=r"pg_cluster_sweep failed \(-22\)"):
            ctx.cluster_sweep(bad, t, c)
        usable()
    assert len(ctx.cluster_sweep(list(range(1, 4097)), t, c)["w"]) == 4096            # the limit itself is fine
    sweep = ctx.lib.pg_cluster_sweep
    assert sweep(None, ptr(t), ptr(c), t.shape[0], ptr(thr), 2, None, None, ptr(out), None, None, None) == -22
    assert sweep(ctx.h, ptr(t), None, t.shape[0], ptr(thr), 2, None, None, ptr(out), None, None, None) == -22
    usable()
    assert sweep(ctx.h, ptr(t), ptr(c), t.shape[0], None, 2, None, None, ptr(out), None, None, None) == -22
    usable()
    big = t.copy()
    big[7, 3] = 2 ** 32
    with pytest.raises(PangenomeError, match=r"pg_cluster_sweep failed \(-22\)"):
        ctx.cluster_sweep([1, 3], big, c)
    usable()
    big[7, 3] = 2 ** 32 - 1                             # the largest value is fine
    assert as_lists(ctx.cluster_sweep([1, 3], big, c)) == reference_sweep(big, c, [1, 3])
    # every output pointer may be NULL
    assert sweep(ctx.h, ptr(t), ptr(c), t.shape[0], ptr(thr), 2, None, None, None, None, None, None) == 0
    n = C.c_uint64()
    assert sweep(ctx.h, ptr(t), ptr(c), t.shape[0], ptr(thr), 2, C.byref(n), None, None, ptr(out), None, None) == 0
    assert out.tolist() == reference_sweep(t, c, [1, 3])["clusters"] and n.value == ctx.cluster_weights(t, c)[0]
    fresh = Context(27, 0)
    try:
        with pytest.raises(PangenomeError, match=r"pg_cluster_sweep failed \(-22\)"):
            fresh.cluster_sweep([1, 3])                 # no pg_edges yet
        with pytest.raises(PangenomeError, match=r"pg_cluster_sweep failed \(-22\)"):
            fresh.cluster_weights()
        assert as_lists(fresh.cluster_sweep([1, 3], t, c)) == reference_sweep(t, c, [1, 3])
    finally:
        fresh.close()


def test_cli_weight_auto(km, tmp_path):
    fx = Fixture("pan8_k27_c3")
    runs = {}
    for w in ("auto", "5"):
        d = tmp_path / w
        d.mkdir()
        q = d / "input.fsa"
        q.write_bytes(fx.fasta)
        argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", w, "-g", "record"]
        out = io.StringIO()
        km.entry_point(argv, out=out)
        runs[w] = (d, argv, out.getvalue())
    d, argv, text = runs["auto"]
    sweep = d / "input.fsa_rdbg_weight.xyz.sweep.tsv"
    want_sweep = sweep_file_text(golden_sweep(), 5)
    assert sweep.read_text() == want_sweep
    assert text.count("# -w auto: 5\n") == 1 and "# -w auto" not in runs["5"][2]
    assert not (runs["5"][0] / "input.fsa_rdbg_weight.xyz.sweep.tsv").exists()
    assert (d / "input.fsa_rdbg_weight.xyz").read_text() == fx.xyz
    mcl = d / "input.fsa_rdbg_weight.xyz.mcl"
    assert mcl.read_text() == reference_mcl(*xyz_arrays(fx.xyz), 5)
    assert rows_of(text) == rows_of(runs["5"][2]) and len(rows_of(text)) > 0
    for name in ("input.fsa_fr_freq.tsv", "input.fsa_fr_spectrum.tsv"):
        assert (d / name).read_bytes() == (runs["5"][0] / name).read_bytes()
    sweep.write_text("stale\n")                         # a second run: the `.mcl` reused, the sweep file rewritten
    again = io.StringIO()
    km.entry_point(argv, out=again)
    assert "# the mcl has been ran" in again.getvalue() and "# -w auto" not in again.getvalue()
    assert sweep.read_text() == want_sweep and rows_of(again.getvalue()) == rows_of(text)
