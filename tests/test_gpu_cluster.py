"""The built-in clusterer on the device (pg_cluster_cc, pangenome_amd/csrc/
pg_cluster.hip): weight cut plus connected components of the `.xyz` graph,
written as a `.mcl`.

Every case compares, exactly: the text with an independent union-find
(tests/cc_util.py), the context's label table with what host.mcl_labels reads
back from that text (arrays in file order), and the returned counts.  The
synthetic shapes are the smallest at which each mechanism can go wrong; the
pipeline cases run the CLI against the networkx-made tests/golden/cc files.
"""
import io
import os
import threading

import numpy as np
import pytest

from cc_util import cc_cases, cc_text, random_graph, reference_mcl, xyz_arrays
from golden_util import Fixture

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


def check(ctx, t, c, w):
    from pangenome_amd import host
    t = np.asarray(t, np.uint64).reshape(-1, 4)
    c = np.asarray(c, np.int64)
    n_clusters, n_nodes = ctx.cluster_cc(t, c, w)
    text = ctx.clusters_text().decode()
    assert text == reference_mcl(t, c, w)
    mk, mv, mi, n_lines = host.mcl_labels(text)
    k, v, i = ctx.labels()
    assert np.array_equal(k, mk) and np.array_equal(v, mv) and np.array_equal(i, mi)
    assert (n_clusters, n_nodes) == (n_lines, mk.shape[0])
    return text


def test_empty(ctx):
    assert check(ctx, np.zeros((0, 4), np.uint64), np.zeros(0, np.int64), 1) == ""
    assert ctx.clusters_text() == b"" and ctx.labels()[0].shape == (0,)


def test_self_loop(ctx):
    assert check(ctx, [[2 ** 64 - 1, 5, 2 ** 64 - 1, 5]], [3], 1) == "18446744073709551615_5\n"


def test_one_key_two_values(ctx):
    t = [[5, 0, 8, 0], [5, 1, 9, 0]]
    assert check(ctx, t, [1, 1], 1) == "5_0\t8_0\n5_1\t9_0\n"


def test_path_across_all_blocks(ctx):
    """65,537 nodes in one path, edges shuffled and randomly oriented: 256
    blocks of 256 threads hook into one component from every XCD (deep find
    chains, path halving, contended CAS).  Twice: the same bytes."""
    rng = np.random.default_rng(65537)
    n = 65537
    perm = rng.permutation(n)                                  # node numbers along the path
    e = np.stack([perm[:-1], perm[1:]], axis=1)
    flip = rng.integers(0, 2, n - 1).astype(bool)
    e[flip] = e[flip][:, ::-1]
    e = e[rng.permutation(n - 1)]
    t, c = tuples_of(e), np.ones(n - 1, np.int64)
    text = check(ctx, t, c, 1)
    assert text.count("\n") == 1 and text.count("\t") == n - 1
    first = ctx.clusters_text()
    ctx.cluster_cc(t, c, 1)
    assert ctx.clusters_text() == first


@pytest.mark.parametrize("hub", ["first", "last"])
def test_star(ctx, hub):
    """5,000 leaves on one hub: every union contends for one root.  The hub
    as the smallest node id, and (its leaves named first by self-loops) as
    the largest."""
    leaves = np.arange(1, 5001)
    star = np.stack([np.zeros(5000, np.int64), leaves], axis=1)
    if hub == "last":
        star = np.concatenate([np.stack([leaves, leaves], axis=1), star[:, ::-1]])
    text = check(ctx, tuples_of(star), np.ones(star.shape[0], np.int64), 1)
    assert text.count("\n") == 1 and text.count("\t") == 5000
    assert text.startswith("0_0\t") == (hub == "first") and text.endswith("\t0_0\n") == (hub == "last")


def test_size_ties_order_by_first_appearance(ctx):
    """3,000 disjoint triangles and 1,000 isolated self-loops, interleaved:
    every size ties."""
    rng = np.random.default_rng(3)
    tri = np.arange(9000).reshape(3000, 3)
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]],
                        np.repeat(np.arange(9000, 10000), 2).reshape(1000, 2)])
    e = e[rng.permutation(e.shape[0])]
    text = check(ctx, tuples_of(e), np.ones(e.shape[0], np.int64), 1)
    sizes = [ln.count("\t") + 1 for ln in text.splitlines()]
    assert sizes == [3] * 3000 + [1] * 1000


def test_bridge_and_threshold(ctx):
    """Two paths of 20,000 nodes (weight 3) joined by a last edge of weight 2."""
    a, b = np.arange(20000), np.arange(20000, 40000)
    e = np.concatenate([np.stack([a[:-1], a[1:]], axis=1), np.stack([b[:-1], b[1:]], axis=1), [[19999, 20000]]])
    c = np.full(e.shape[0], 3, np.int64)
    c[-1] = 2
    t = tuples_of(e)
    assert check(ctx, t, c, 2).count("\n") == 1
    two = check(ctx, t, c, 3)
    assert [ln.count("\t") + 1 for ln in two.splitlines()] == [20000, 20000]
    single = check(ctx, t, c, 4)
    assert single.count("\n") == 40000 and "\t" not in single
    assert ctx.labels()[2].tolist() == list(range(40000))


@pytest.mark.parametrize("E", [10_000, 40_000])
@pytest.mark.parametrize("w", [1, 3])
def test_random_graphs(ctx, E, w):
    """U = 20,000 below (E = U / 2) and above (E = 2 U) the giant-component threshold."""
    t, c = random_graph(7 + E, 20_000, E)
    check(ctx, t, c, w)


@pytest.mark.parametrize("sink", ["file", "append", "pipe"])
def test_clusters_write(ctx, tmp_path, sink):
    t, c = random_graph(11, 3000, 5000)
    ctx.cluster_cc(t, c, 2)
    want = ctx.clusters_text()
    assert want == reference_mcl(t, c, 2).encode()
    if sink == "pipe":
        r, w = os.pipe()
        got = []
        th = threading.Thread(target=lambda: got.append(os.fdopen(r, "rb").read()))
        th.start()
        try:
            n = ctx.clusters_write(w)
        finally:
            os.close(w)
        th.join()
        data = got[0]
    else:
        fn = tmp_path / "out.mcl"
        fn.write_bytes(b"# before\n")
        with open(fn, "ab" if sink == "append" else "r+b") as f:
            f.seek(0, os.SEEK_END)
            n = ctx.clusters_write(f.fileno())
            assert os.lseek(f.fileno(), 0, os.SEEK_CUR) == len(b"# before\n") + n
        data = fn.read_bytes()
        assert data.startswith(b"# before\n")
        data = data[len(b"# before\n"):]
    assert n == len(want) and data == want


def test_argument_errors(ctx):
    """Refused before any launch: no device fault is involved."""
    import ctypes as C
    from pangenome_amd._lib import Context, PangenomeError, ptr
    t, c = random_graph(13, 50, 80)
    with pytest.raises(PangenomeError, match=r"pg_cluster_cc failed \(-22\)"):
        ctx.cluster_cc(t, c, 0)
    with pytest.raises(PangenomeError, match=r"pg_cluster_cc failed \(-22\)"):
        ctx.cluster_cc(t, c, -3)
    n = C.c_uint64()
    rc = ctx.lib.pg_cluster_cc(ctx.h, ptr(np.ascontiguousarray(t)), None, t.shape[0], 1, None, None)
    assert rc == -22
    ctx.cluster_cc(t, c, 1)
    text = ctx.clusters_text()
    buf = np.empty(len(text), np.uint8)
    assert ctx.lib.pg_clusters_format(ctx.h, ptr(buf), len(text) - 1, C.byref(n)) == -34
    assert ctx.lib.pg_clusters_format(ctx.h, ptr(buf), len(text), C.byref(n)) == 0 and buf.tobytes() == text
    fresh = Context(27, 0)
    try:
        with pytest.raises(PangenomeError, match=r"pg_clusters_format failed \(-22\)"):
            fresh.clusters_text()
    finally:
        fresh.close()


def test_device_edges_equal_host_edges(ctx):
    """tuples=None clusters the last edge pass where it lies on the device:
    the same text as the exported edges uploaded again."""
    fx = Fixture("pan8_k27_c3")
    ctx.parse_host(np.frombuffer(fx.fasta, np.uint8))
    ctx.build_dbg(None, 0, True)
    ctx.build_rdbg()
    assert ctx.edges_count(None, True) == fx.meta["n_edges"]
    assert ctx.cluster_cc(None, None, 4)[0] == 6063
    text = ctx.clusters_text().decode()
    assert text == cc_text("pan8_k27_c3", 4)
    t, c, _ = ctx.edges_export()
    assert check(ctx, t, c, 4) == text


# ------------------------------------------------------------ whole pipeline
def _oracle_rows(oracle_mod, fx, mcl_text):
    return oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, mcl_text, edge_chunk=fx.edge_chunk)["rows"]


@pytest.mark.parametrize("name,w", cc_cases())
def test_cli_cc_vs_goldens(km, oracle_mod, tmp_path, name, w):
    fx = Fixture(name)
    assert fx.meta["chunk"] is None
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", str(w)]
    if fx.ns is not None:
        argv += ["-n", str(fx.meta["n"])]
    mcl = tmp_path / "input.fsa_rdbg_weight.xyz.mcl"
    assert not mcl.exists()
    out = io.StringIO()
    km.entry_point(argv, out=out)
    want_mcl = cc_text(name, w)
    want_rows = _oracle_rows(oracle_mod, fx, want_mcl)
    assert mcl.read_text() == want_mcl
    assert (tmp_path / "input.fsa_rdbg_weight.xyz").read_text() == fx.xyz
    assert rows_of(out.getvalue()) == want_rows
    assert "# the mcl has been ran" not in out.getvalue()
    again = io.StringIO()                            # the file is the cache: the unchanged reuse path
    km.entry_point(argv, out=again)
    assert "# the mcl has been ran" in again.getvalue()
    assert rows_of(again.getvalue()) == want_rows
    assert mcl.read_text() == want_mcl


def test_cc_labels_carry_meaning(km, tmp_path):
    """The issue's point: at W = 4 pan8_k27_c3's rows share labels (909
    distinct over 2945 rows) where the empty `.mcl` gave one per row."""
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    out = io.StringIO()
    km.entry_point(["kmer_numba.py", "-i", str(q), "-k27", "-c3", "-acc", "-w4"], out=out)
    rows = rows_of(out.getvalue())
    assert (len(rows), len({r.split("\t")[4] for r in rows})) == (2945, 909)


def test_seq2graph_cc_host_edges_path(km, oracle_mod, tmp_path):
    """pan8_k27_chunk's edge checkpoints leave the edges on the host
    (rdbg_edges' reversal): cluster_cc takes the host arrays."""
    from pangenome_amd import host
    fx = Fixture("pan8_k27_chunk")
    assert fx.meta["chunk"]
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    Ns = fx.ns if fx.ns is not None else 2 ** 63
    out = io.StringIO()
    g = km.seq2rdbg(str(q), fx.k, 5, Ns, brkpt="", chunk=2 ** 33, rc=(fx.c >> 1) == 1)
    km.dbg2rdbg(g)
    km.seq2graph(str(q), kmer=fx.k, bits=5, Ns=Ns, rdbg_dict=g, chunk=fx.edge_chunk, brkpt="", rc=(fx.c & 1) == 1,
                 cluster="cc", min_weight=2, out=out)
    assert (tmp_path / "input.fsa_rdbg_weight.xyz").read_text() == fx.xyz
    t, c = xyz_arrays(fx.xyz)
    want_mcl = host.cluster_cc(t, c, 2)[0]
    assert want_mcl == reference_mcl(t, c, 2)
    assert (tmp_path / "input.fsa_rdbg_weight.xyz.mcl").read_text() == want_mcl
    assert rows_of(out.getvalue()) == _oracle_rows(oracle_mod, fx, want_mcl)


def test_default_still_runs_mcl(km, tmp_path, monkeypatch):
    """Without -a nothing changes: no `.mcl` is written before the external
    `mcl` command is issued (stood in for here: it is not installed)."""
    fx = Fixture("edge_k27")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    mcl = tmp_path / "input.fsa_rdbg_weight.xyz.mcl"
    calls = []

    def fake_system(cmd):
        calls.append((cmd, mcl.exists()))
        mcl.write_text("")
        return 0
    monkeypatch.setattr(km.os, "system", fake_system)
    out = io.StringIO()
    km.entry_point(["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c)], out=out)
    xyz = str(q) + "_rdbg_weight.xyz"
    assert calls == [("mcl %s --abc -I 1.5 -te 8 -o %s.mcl -q x -V all" % (xyz, xyz), False)]
    assert rows_of(out.getvalue()) == fx.rows
