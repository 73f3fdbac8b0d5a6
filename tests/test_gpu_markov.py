"""Markov clustering on the device (pg_cluster_markov, pangenome_amd/csrc/
pg_markov.hip) against its specification, host.cluster_markov, bit for bit:
the exported matrix after 0, 1, 2 and up to 200 iterations, the iteration
count, the chaos, the counts, the `.mcl` text and the label table.  The
specification itself is held to an independent dense restatement in
tests/test_markov_host.py."""
import gzip
import io
import json
import os
import sys

import numpy as np
import pytest

from cc_util import random_graph, xyz_arrays
from dist_util import ROOT, spawn_ranks
from golden_util import GOLDEN, Fixture
import markov_util as mu

pytestmark = pytest.mark.gpu

MK = os.path.join(GOLDEN, "markov")
GRID = mu.GRID + [(3, sel, 1) for sel in (1, 3, 8)]


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


def state(ctx):
    """everything a clustering call leaves: the text, the label table, the matrix"""
    return (ctx.clusters_text(),) + tuple(a.tobytes() for a in ctx.labels()) + \
        tuple(a.tobytes() for a in ctx.cluster_markov_matrix())


def check(ctx, t, c, w=1, i2=3, sel=64, iters=(0, 1, 2, 200), device_edges=False):
    """the device equals the specification at every iteration cap of `iters`; returns the last result"""
    from pangenome_amd import host
    t = np.asarray(t, np.uint64).reshape(-1, 4)
    c = np.asarray(c, np.int64)
    want = None
    for mi in iters:
        want = host.cluster_markov(t, c, w, i2, sel, mi)
        got = ctx.cluster_markov(None, None, w, i2, sel, mi) if device_edges else ctx.cluster_markov(t, c, w, i2, sel, mi)
        text, wk, wv, wl, n_iter, chaos, (col_len, rows, vals) = want
        assert got == (text.count("\n"), wk.shape[0], n_iter, chaos), (w, i2, sel, mi)
        g_len, g_rows, g_vals = ctx.cluster_markov_matrix()
        assert g_rows.shape == (wk.shape[0], sel)
        assert np.array_equal(g_len, col_len), (w, i2, sel, mi)
        assert np.array_equal(g_rows, rows) and np.array_equal(g_vals, vals), (w, i2, sel, mi)
        assert ctx.clusters_text().decode() == text
        k, v, i = ctx.labels()
        assert np.array_equal(k, wk) and np.array_equal(v, wv) and np.array_equal(i, wl)
    return want


@pytest.mark.parametrize("name", sorted(mu.hand_cases()))
def test_hand_cases(ctx, name):
    t, c, clusters = mu.hand_cases()[name]
    for i2, sel, w in GRID:
        want = check(ctx, t, c, w, i2, sel)
        if (i2, sel, w) == (3, 64, 1):
            assert want[0] == mu.text_of(clusters)


@pytest.mark.parametrize("seed", range(12))
def test_random_graphs(ctx, seed):
    """50 to 400 nodes, weights 1 to 5 (so values tie often), the whole parameter grid"""
    U = 50 + (seed * 350) // 11
    t, c = random_graph(100 + seed, U, 2 * U + seed)
    for i2, sel, w in GRID:
        check(ctx, t, c, w, i2, sel)


def test_star_initial_column_exceeds_select(ctx):
    t, c = mu.star(200)
    assert check(ctx, t, c, sel=64, iters=(0,))[6][0][0] == 64     # the hub: 201 weights pruned to 64
    check(ctx, t, c, sel=64, iters=(1, 200))
    check(ctx, t, c, sel=8)


def test_clique_all_values_tie(ctx):
    """80 nodes, every weight equal: the selection is by row alone"""
    t, c = mu.clique(80)
    m = check(ctx, t, c, sel=64)[6]
    check(ctx, t, c, sel=3, i2=4)
    assert m[0].max() <= 64


def test_ring_long_flow(ctx):
    t, c = mu.ring(300)
    assert check(ctx, t, c, iters=(200,))[4] > 10
    check(ctx, t, c, i2=4, sel=2, iters=(1, 2, 200))


def test_big_columns_run_the_block_class(ctx):
    """4,500 nodes, each linked to 32 neighbours on either side: one iteration
    from 64-entry columns has select^2 candidates per column, the block
    class's table.  Compared through the committed digest of the
    specification's matrix (tests/test_markov_host.py regenerates it)."""
    from pangenome_amd import host
    gold = json.load(open(os.path.join(MK, "bigcol.json")))
    t, c = mu.bigcol()
    ctx.cluster_markov(t, c, 1, 3, 64, 0)
    m0 = ctx.cluster_markov_matrix()
    w0 = host.cluster_markov(t, c, 1, 3, 64, 0)[6]
    assert all(np.array_equal(a, b) for a, b in zip(m0, w0))
    assert int(mu.candidates(w0).max()) == gold["max_candidates"] > 2048
    ctx.cluster_markov(t, c, 1, 3, 64, 1)
    assert mu.matrix_digest(ctx.cluster_markov_matrix()) == gold["sha256"]
    nu, sel, cols_wave, cols_mid, cols_block = ctx.cluster_markov_stats()
    assert (nu, sel) == (4500, 64) and (cols_wave, cols_mid, cols_block) == (0, 0, 4500)
    # every class in one call: a long path (bounds of 2 to 9) and a ring with 8 neighbours on either side
    # (17 x 17 = 289) beside the dense ring
    path = mu.tuples_of([[10000 + i, 10001 + i] for i in range(500)])
    r = np.repeat(np.arange(300), 8)
    ring8 = mu.tuples_of(np.stack([20000 + r, 20000 + (r + np.tile(np.arange(1, 9), 300)) % 300], axis=1))
    t2 = np.concatenate([t, path, ring8])
    c2 = np.concatenate([c, np.ones(500, np.int64), np.full(2400, 3, np.int64)])
    ctx.cluster_markov(t2, c2, 1, 3, 64, 1)
    assert ctx.cluster_markov_stats() == (5301, 64, 501, 300, 4500)
    want = host.cluster_markov(t2, c2, 1, 3, 64, 1)[6]
    assert all(np.array_equal(a, b) for a, b in zip(ctx.cluster_markov_matrix(), want))


@pytest.mark.parametrize("i2", [3, 39])
def test_inflation_arithmetic(ctx, i2):
    """Weights from 1 to 2^31 around one hub and along a chain: the scaled
    values x of the first iteration run from below 2^7 to ONE, with perfect
    squares and others among the x << 31 whose root is taken, so the products,
    the exact division and the integer root with its fix-up (odd inflation2)
    run across their range.  (Stored values are at least CUT, so an expanded
    value is at least CUT^2 >> 31 = 21: x = 1 cannot occur.)"""
    import math
    from pangenome_amd import host
    t, c = mu.inflation_graph()
    xs = mu.scaled_values(host.cluster_markov(t, c, 1, i2, 64, 0)[6])
    squares = [x for x in xs if math.isqrt(x << 31) ** 2 == x << 31]
    assert min(xs) < 2 ** 7 and max(xs) == mu.ONE and 0 < len(squares) < len(xs)
    check(ctx, t, c, 1, i2, 64)
    check(ctx, t, c, 1, i2, 5, iters=(1, 2, 200))


def test_schedule_independence(ctx):
    t, c = random_graph(5, 400, 1500)
    ctx.cluster_markov(t, c, 1, 3, 8)
    first = state(ctx)
    ctx.cluster_markov(t, c, 1, 3, 8)
    assert state(ctx) == first
    ctx.cluster_cc(*random_graph(6, 300, 500), 2)
    ctx.cluster_markov(t, c, 1, 3, 8)
    assert state(ctx) == first


def test_device_edges_equal_host_edges(ctx):
    """tuples == NULL clusters the last edge pass where it lies on the device"""
    fx = Fixture("pan8_k27_c3")
    ctx.parse_host(np.frombuffer(fx.fasta, np.uint8))
    ctx.build_dbg(None, 0, True)
    ctx.build_rdbg()
    assert ctx.edges_count(None, True) == fx.meta["n_edges"]
    t, c, _ = ctx.edges_export()
    check(ctx, t, c, 1, 3, 64, iters=(0, 2), device_edges=True)
    check(ctx, t, c, 2, 4, 8, iters=(3,), device_edges=True)


def test_refusals_keep_the_previous_result(ctx):
    import ctypes as C
    from pangenome_amd._lib import Context, PangenomeError, ptr
    t, c = random_graph(13, 50, 80)
    U = ctx.cluster_markov(t, c, 1, 3, 8)[1]
    before = state(ctx)
    for kw in (dict(min_weight=0), dict(inflation2=2), dict(inflation2=41), dict(select=0), dict(select=65),
               dict(max_iter=10001)):
        with pytest.raises(PangenomeError, match=r"pg_cluster_markov failed \(-22\)"):
            ctx.cluster_markov(t, c, **kw)
        assert state(ctx) == before
    assert ctx.lib.pg_cluster_markov(ctx.h, ptr(np.ascontiguousarray(t)), None, t.shape[0], 1, 3, 64, 200,
                                     None, None, None, None) == -22
    with pytest.raises(PangenomeError, match=r"pg_cluster_markov failed \(-22\)"):     # a node value above 2^32 - 1
        ctx.cluster_markov([[1, 2 ** 32, 2, 0]], [1])
    heavy = mu.tuples_of([[0, 1], [1, 0], [1, 2]])
    with pytest.raises(PangenomeError, match=r"pg_cluster_markov failed \(-34\)"):     # a weight sum of exactly 2^32
        ctx.cluster_markov(heavy, [2 ** 31, 2 ** 31, 1])
    assert state(ctx) == before
    ctx.cluster_markov(heavy, [2 ** 31, 2 ** 31 - 1, 1], max_iter=1)                   # one below: accepted
    ctx.cluster_markov(t, c, 1, 3, 8)
    assert state(ctx) == before
    buf = [np.zeros(U, np.uint32), np.zeros((U, 8), np.uint32), np.zeros((U, 8), np.uint32)]
    sel = C.c_uint32()
    assert ctx.lib.pg_cluster_markov_matrix(ctx.h, *[ptr(a) for a in buf], U - 1, C.byref(sel)) == -34
    assert ctx.lib.pg_cluster_markov_matrix(ctx.h, *[ptr(a) for a in buf], U, C.byref(sel)) == 0 and sel.value == 8
    assert all(np.array_equal(a, b) for a, b in zip(buf, ctx.cluster_markov_matrix()))
    fresh = Context(27, 0)
    try:
        assert fresh.lib.pg_cluster_markov_matrix(fresh.h, *[ptr(a) for a in buf], U, C.byref(sel)) == -22
        with pytest.raises(PangenomeError, match=r"pg_cluster_markov_stats failed \(-22\)"):
            fresh.cluster_markov_stats()
    finally:
        fresh.close()


# ------------------------------------------------------------ whole pipeline
def golden_mcl():
    return gzip.open(os.path.join(MK, "pan8_k27_c3_I3.mcl.gz")).read().decode()


def test_cli_markov_vs_golden(km, oracle_mod, tmp_path):
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "markov"]
    mcl = tmp_path / "input.fsa_rdbg_weight.xyz.mcl"
    out = io.StringIO()
    km.entry_point(argv, out=out)
    want_mcl = golden_mcl()
    want_rows = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, want_mcl, edge_chunk=fx.edge_chunk)["rows"]
    assert mcl.read_text() == want_mcl
    assert (tmp_path / "input.fsa_rdbg_weight.xyz").read_text() == fx.xyz
    assert rows_of(out.getvalue()) == want_rows
    assert "# the mcl has been ran" not in out.getvalue() and "not converged" not in out.getvalue()
    again = io.StringIO()
    km.entry_point(argv, out=again)
    assert "# the mcl has been ran" in again.getvalue() and rows_of(again.getvalue()) == want_rows
    assert mcl.read_text() == want_mcl


def test_cli_markov_inflation_and_groups(km, tmp_path):
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    km.entry_point(["kmer_numba.py", "-i", str(q), "-k27", "-c3", "-a", "markov", "-I", "2", "-g", "record"],
                   out=io.StringIO())
    t, c = xyz_arrays(fx.xyz)
    assert (tmp_path / "input.fsa_rdbg_weight.xyz.mcl").read_text() == host.cluster_markov(t, c, 1, 4)[0]
    for name in ("_fr_freq.tsv", "_fr_spectrum.tsv", "_fr_genomes.tsv", "_fr_presence.npz"):
        assert (tmp_path / ("input.fsa" + name)).stat().st_size > 0


def _cli_rank(rank, world, port, q, argv, cwd):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from pangenome_amd import dist as pdist
    os.chdir(cwd)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = io.StringIO()
    calls = []
    real = pdist.GpuShard.cluster_markov

    def spy(self, tuples, counts, w, i2):
        calls.append((len(counts), int(w), int(i2)))
        return real(self, tuples, counts, w, i2)
    pdist.GpuShard.cluster_markov = spy
    try:
        pdist.entry_point(argv, out=out, device=torch.device("cuda", 0), dev_index=0)
    finally:
        dist.destroy_process_group()
    q.put((rank, (out.getvalue(), calls)))


def test_dist_cli_markov_one_rank_one_gpu(oracle_mod, tmp_path):
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "markov"]
    got = spawn_ranks(1, _cli_rank, (argv, str(tmp_path)))
    want_mcl = golden_mcl()
    assert got[0][1] == [(fx.meta["n_edges"], 1, 3)]
    assert (tmp_path / "input.fsa_rdbg_weight.xyz.mcl").read_text() == want_mcl
    want_rows = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, want_mcl, edge_chunk=fx.edge_chunk)["rows"]
    assert rows_of(got[0][0]) == want_rows
