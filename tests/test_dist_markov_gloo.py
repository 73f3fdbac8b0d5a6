"""The sharded CLI with Markov clustering (-a markov) on CPU with gloo: the
oracle stands in for the kernels (OracleShard has no device context, so rank
0 clusters its reduced edge list with host.cluster_markov), writes the `.mcl`
and goes on through the unchanged reuse path."""
import gzip
import io
import os
import sys

from dist_util import ROOT, OracleShard, spawn_ranks
from golden_util import GOLDEN, Fixture


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


def test_dist_cli_markov_two_ranks(oracle_mod, tmp_path):
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    mcl = tmp_path / "input.fsa_rdbg_weight.xyz.mcl"
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "markov", "-I", "1.5"]
    outs = spawn_ranks(2, _cli_rank, (argv,))
    want_mcl = gzip.open(os.path.join(GOLDEN, "markov", "pan8_k27_c3_I3.mcl.gz")).read().decode()
    assert mcl.read_text() == want_mcl
    assert (tmp_path / "input.fsa_rdbg_weight.xyz").read_text() == fx.xyz
    want_rows = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, want_mcl, edge_chunk=fx.edge_chunk)["rows"]
    assert rows_of(outs[0]) == want_rows and rows_of(outs[1]) == []
    assert "# the mcl has been ran" not in outs[0] and "not converged" not in outs[0]
    outs = spawn_ranks(2, _cli_rank, (argv,))          # the file is reused
    assert "# the mcl has been ran" in outs[0] and rows_of(outs[0]) == want_rows
