"""The sharded CLI with the built-in clusterer (-a cc) through the HIP
library: 2 ranks sharing one GPU (gloo collectives, as tests/test_gpu_dist.py);
rank 0 clusters its reduced host edge list on its device
(GpuShard.cluster_cc -> pg_cluster_cc) and writes the `.mcl`."""
import io
import os
import sys

import pytest

from dist_util import ROOT, spawn_ranks
from cc_util import cc_text
from golden_util import Fixture

pytestmark = pytest.mark.gpu


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
    real = pdist.GpuShard.cluster_cc

    def spy(self, tuples, counts, w):
        calls.append((len(counts), int(w)))
        return real(self, tuples, counts, w)
    pdist.GpuShard.cluster_cc = spy
    try:
        pdist.entry_point(argv, out=out, device=torch.device("cuda", 0), dev_index=0)
    finally:
        dist.destroy_process_group()
    q.put((rank, (out.getvalue(), calls)))


def rows_of(text):
    return [ln for ln in text.split("\n") if len(ln.split("\t")) == 5 and ln.split("\t")[3] in ("+", "-")]


def test_dist_cli_cc_two_ranks_one_gpu(oracle_mod, tmp_path):
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4"]
    got = spawn_ranks(2, _cli_rank, (argv, str(tmp_path)))
    want_mcl = cc_text("pan8_k27_c3", 4)
    assert got[0][1] == [(fx.meta["n_edges"], 4)] and got[1][1] == []
    assert (tmp_path / "input.fsa_rdbg_weight.xyz.mcl").read_text() == want_mcl
    assert (tmp_path / "input.fsa_rdbg_weight.xyz").read_text() == fx.xyz
    want_rows = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, want_mcl, edge_chunk=fx.edge_chunk)["rows"]
    assert rows_of(got[0][0]) == want_rows and rows_of(got[1][0]) == []
