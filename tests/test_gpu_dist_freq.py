"""The sharded CLI's frequency table (-g) through the HIP library: 2 ranks
sharing one GPU (gloo collectives, as tests/test_gpu_dist_cluster.py); every
rank makes its partial table on its device (GpuShard.freq -> pg_freq on the
rows of the pass just run) and rank 0 merges them."""
import io
import os
import sys

import pytest

from cc_util import cc_text
from dist_util import ROOT, spawn_ranks
from freq_util import assert_files, fasta_names, reference_freq, rows5_of
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
    real = pdist.GpuShard.freq

    def spy(self, rec_group, n_groups):
        t = real(self, rec_group, n_groups)
        calls.append((len(rec_group), int(n_groups), int(t["n_used"])))
        return t
    pdist.GpuShard.freq = spy
    try:
        pdist.entry_point(argv, out=out, device=torch.device("cuda", 0), dev_index=0)
    finally:
        dist.destroy_process_group()
    q.put((rank, (out.getvalue(), calls)))


def test_dist_cli_freq_two_ranks_one_gpu(oracle_mod, tmp_path):
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    names = fasta_names(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", "record"]
    got = spawn_ranks(2, _cli_rank, (argv, str(tmp_path)))
    lines = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, cc_text("pan8_k27_c3", 4),
                                    edge_chunk=fx.edge_chunk)["rows"]
    ref = reference_freq(rows5_of(lines, names), list(range(8)), 8)
    assert_files(str(q), ref, [n.split()[0] for n in names])
    c0, c1 = got[0][1], got[1][1]
    assert len(c0) == len(c1) == 1 and c0[0][1] == c1[0][1] == 8
    assert c0[0][0] + c1[0][0] == 8 and c0[0][2] + c1[0][2] == 2945
