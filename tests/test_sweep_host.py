"""The cluster curve's host side (no GPU): the independent reference
(tests/sweep_util.py) against the committed table, host.cluster_sweep (the
executable specification of pg_cluster_sweep) against that reference, the
thresholds and the rule of `-w auto`, the sweep file, the CLI flags, and the
sharded CLI with `-a cc -w auto` on CPU with gloo (OracleShard has no device
context, so rank 0 sweeps its merged edges with host.cluster_sweep)."""
import io
import os
import sys

import numpy as np
import pytest

from cc_util import random_graph, reference_mcl, xyz_arrays
from dist_util import ROOT, OracleShard, spawn_ranks
from golden_util import Fixture
from sweep_util import as_lists, golden_sweep, reference_sweep, sweep_file_text

# the weight -w auto picks on each fixture: the peak of the clusters of two or more nodes
AUTO = {"pan8_k27_c3": (5, 440), "pan8_k27_c2": (5, 220), "pan8_k15": (6, 652)}


@pytest.fixture(scope="module")
def curves():
    """name -> (tuples, counts, thresholds, the reference's rows), made once."""
    from pangenome_amd import host
    out = {}
    for name in AUTO:
        t, c = xyz_arrays(Fixture(name).xyz)
        thr = host.sweep_thresholds(int(c.max()))
        out[name] = (t, c, thr, reference_sweep(t, c, thr))
    return out


def test_reference_matches_the_committed_table(curves):
    t, c, thr, ref = curves["pan8_k27_c3"]
    assert (t.shape[0], int(c.max()), thr) == (12583, 7, list(range(1, 9)))
    assert ref == golden_sweep()


@pytest.mark.parametrize("name", sorted(AUTO))
def test_host_sweep_matches_reference_on_fixtures(curves, name):
    from pangenome_amd import host
    t, c, thr, ref = curves[name]
    got = host.cluster_sweep(t, c, thr)
    assert as_lists(got) == ref
    assert got["w"].dtype == np.int64 and all(got[k].dtype == np.uint64 for k in ("edges", "clusters", "largest"))
    multi = [a - b for a, b in zip(ref["clusters"], ref["singletons"])]
    assert (host.sweep_choice(got), max(multi)) == AUTO[name]
    assert ref["edges"][-1] == 0 and ref["singletons"][-1] == ref["clusters"][-1]      # the all-singletons row


@pytest.mark.parametrize("seed,thr", [(1, [1, 2, 3, 4, 5, 6]), (2, [2, 5]), (3, [1]), (4, [7, 9]), (5, [3])])
def test_host_sweep_matches_reference_on_random_graphs(seed, thr):
    from pangenome_amd import host
    t, c = random_graph(200 + seed, 2000, 3100)
    assert as_lists(host.cluster_sweep(t, c, thr)) == reference_sweep(t, c, thr)


def test_host_sweep_small_cases():
    from pangenome_amd import host
    z = host.cluster_sweep(np.zeros((0, 4), np.uint64), np.zeros(0, np.int64), [1, 2])
    assert as_lists(z) == {"w": [1, 2], "edges": [0, 0], "clusters": [0, 0], "largest": [0, 0], "singletons": [0, 0]}
    t = [[5, 0, 8, 0], [5, 1, 9, 0], [7, 3, 7, 3]]            # one key with two values; a self-loop
    got = as_lists(host.cluster_sweep(t, [1, 2, 3], [1, 2, 3, 4]))
    assert got == reference_sweep(t, [1, 2, 3], [1, 2, 3, 4])
    assert got["edges"] == [3, 2, 1, 0] and got["clusters"] == [3, 4, 5, 5] and got["singletons"] == [1, 3, 5, 5]
    assert as_lists(host.cluster_sweep(t, [1, 2, 3], [])) == {k: [] for k in got}
    for bad in ([0, 1], [2, 2], [3, 1], [-1]):
        with pytest.raises(ValueError):
            host.cluster_sweep(t, [1, 2, 3], bad)
    with pytest.raises(ValueError):
        host.cluster_sweep(t, [1, 2, 3], list(range(1, 4098)))
    with pytest.raises(ValueError):
        host.cluster_sweep(t, [1, 2], [1])


def test_sweep_thresholds():
    from pangenome_amd.host import sweep_thresholds
    assert sweep_thresholds(0) == [1]
    assert sweep_thresholds(1) == [1, 2]
    assert sweep_thresholds(7) == list(range(1, 9))
    assert sweep_thresholds(63) == list(range(1, 65))
    assert sweep_thresholds(64) == list(range(1, 65)) + [65]
    assert sweep_thresholds(200) == list(range(1, 65)) + [128, 201]
    assert sweep_thresholds(1000) == list(range(1, 65)) + [128, 256, 512, 1001]
    assert sweep_thresholds(128) == list(range(1, 65)) + [128, 129]
    for m in (0, 1, 7, 63, 64, 200, 1000, 2 ** 40):
        thr = sweep_thresholds(m)
        assert thr[-1] == m + 1 and all(a < b for a, b in zip(thr, thr[1:])) and len(thr) <= 4096


def test_sweep_choice():
    from pangenome_amd.host import sweep_choice
    tab = lambda w, c, s: {"w": np.array(w, np.int64), "clusters": np.array(c, np.uint64),
                           "singletons": np.array(s, np.uint64)}
    assert sweep_choice(tab([1, 2, 3, 4], [2, 10, 12, 9], [0, 3, 5, 9])) == 2        # 2, 7, 7, 0: the smaller of equals
    assert sweep_choice(tab([2, 5, 9], [4, 9, 9], [3, 2, 9])) == 5
    assert sweep_choice(tab([], [], [])) == 1
    assert sweep_choice(tab([3, 4], [5, 6], [5, 6])) == 1                             # no cluster of two anywhere
    assert sweep_choice(golden_sweep()) == 5


def test_write_sweep_file(tmp_path):
    from pangenome_amd import host
    q = str(tmp_path / "in.fsa")
    host.write_sweep_file(q, golden_sweep(), 5)
    assert sorted(os.listdir(tmp_path)) == ["in.fsa_rdbg_weight.xyz.sweep.tsv"]        # no .tmp left behind
    data = (tmp_path / "in.fsa_rdbg_weight.xyz.sweep.tsv").read_bytes()
    assert data == (b"#w\tedges\tclusters\tlargest\tsingletons\tmulti\n"
                    b"1\t12583\t2\t5103\t0\t2\n2\t4964\t5249\t1410\t5239\t10\n3\t4762\t5443\t182\t5367\t76\n"
                    b"4\t4142\t6063\t93\t5845\t218\n5\t2754\t7451\t30\t7011\t440\n6\t1088\t9117\t14\t8713\t404\n"
                    b"7\t48\t10157\t3\t10113\t44\n8\t0\t10205\t1\t10205\t0\n#auto\t5\n")
    assert data.decode() == sweep_file_text(golden_sweep(), 5)
    t = {"w": np.array([2 ** 40], np.int64), "edges": np.array([2 ** 63], np.uint64), "clusters": np.array([7], np.uint64),
         "largest": np.array([0], np.uint64), "singletons": np.array([7], np.uint64)}
    host.write_sweep_file(q, t, 1)                                                    # replaced whole; unsigned
    assert (tmp_path / "in.fsa_rdbg_weight.xyz.sweep.tsv").read_text().splitlines()[1:] == \
        ["1099511627776\t9223372036854775808\t7\t0\t7\t0", "#auto\t1"]


def test_parse_args_weight_auto():
    from pangenome_amd.kmer import parse_args, weight_arg
    a = parse_args(["x", "-i", "f.fa", "-a", "cc", "-w", "auto"])
    assert a["-w"] == "auto" and weight_arg(a) == "auto"
    a = parse_args(["x", "-i", "f.fa", "-acc", "-wauto", "-k27"])
    assert a["-a"] == "cc" and a["-w"] == "auto" and a["-k"] == "27" and weight_arg(a) == "auto"
    assert weight_arg(parse_args(["x", "-w", "4"])) == 4 and weight_arg(parse_args(["x"])) == 1
    with pytest.raises(ValueError):                     # any other non-integer fails as before
        weight_arg(parse_args(["x", "-w", "heavy"]))


def test_manual_ends_with_the_weight_line():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    assert lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert "auto" in lines[-1] and "sweep.tsv" in lines[-1] and "default 1" in lines[-1]


def test_binding_marshals_sweep_entry_point():
    """The ctypes argument list of pg_cluster_sweep accepts what the Context
    methods pass (a NULL context: PG_EINVAL, no device touched)."""
    from pangenome_amd import _lib

    class Fake:
        pass
    f = Fake()
    f.lib, f.h = _lib.load(), None
    f._sweep = lambda *a: _lib.Context._sweep(f, *a)
    t, c = random_graph(1, 10, 5)
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_sweep failed \(-22\)"):
        _lib.Context.cluster_sweep(f, [1, 2], t, c)
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_sweep failed \(-22\)"):
        _lib.Context.cluster_sweep(f, [1])
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_sweep failed \(-22\)"):
        _lib.Context.cluster_weights(f, t, c)


# ------------------------------------------------------------ sharded CLI
def _cli_rank(rank, world, port, q, argv):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from pangenome_amd import dist as pdist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = io.StringIO()
    try:
        pdist.entry_point(argv, out=out, shard_factory=OracleShard)
    finally:
        dist.destroy_process_group()
    q.put((rank, out.getvalue()))


def rows_of(text):
    return [ln for ln in text.split("\n") if len(ln.split("\t")) == 5 and ln.split("\t")[3] in ("+", "-")]


def test_dist_cli_cc_auto_two_ranks(oracle_mod, tmp_path):
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    mcl = tmp_path / "input.fsa_rdbg_weight.xyz.mcl"
    sweep = tmp_path / "input.fsa_rdbg_weight.xyz.sweep.tsv"
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "auto"]
    outs = spawn_ranks(2, _cli_rank, (argv,))
    assert (tmp_path / "input.fsa_rdbg_weight.xyz").read_text() == fx.xyz
    assert sweep.read_text() == sweep_file_text(golden_sweep(), 5)
    want_mcl = reference_mcl(*xyz_arrays(fx.xyz), 5)
    assert mcl.read_text() == want_mcl
    want_rows = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, want_mcl, edge_chunk=fx.edge_chunk)["rows"]
    assert rows_of(outs[0]) == want_rows and rows_of(outs[1]) == []
    assert outs[0].count("# -w auto: 5\n") == 1 and "# -w auto" not in outs[1]
    assert "# the mcl has been ran" not in outs[0]
    sweep.unlink()                                      # the `.mcl` is reused; the sweep file is still written
    outs = spawn_ranks(2, _cli_rank, (argv,))
    assert "# the mcl has been ran" in outs[0] and "# -w auto" not in outs[0] and rows_of(outs[0]) == want_rows
    assert sweep.read_text() == sweep_file_text(golden_sweep(), 5) and mcl.read_text() == want_mcl
