"""The sharded CLI's genome comparison (-p) through the HIP library: 2 ranks
sharing one GPU (gloo collectives, as tests/test_gpu_dist_freq.py); rank 0
merges the partial tables on the host and compares the genomes on its device
from the merged presence bits (GpuShard.freq_compare -> pg_freq_compare)."""
import io
import os
import sys

import numpy as np
import pytest

from compare_util import NEW_FILES, OLD_FILES, assert_compare_files, fr_files, reference_compare
from dist_util import ROOT, spawn_ranks
from freq_util import fasta_names, golden
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
    real = pdist.GpuShard.freq_compare

    def spy(self, bits, n_groups, orders):
        calls.append((tuple(np.asarray(bits).shape), int(n_groups), tuple(np.asarray(orders).shape)))
        return real(self, bits, n_groups, orders)
    pdist.GpuShard.freq_compare = spy
    try:
        pdist.entry_point(argv, out=out, device=torch.device("cuda", 0), dev_index=0)
    finally:
        dist.destroy_process_group()
    q.put((rank, calls))


def test_dist_cli_compare_two_ranks_one_gpu(tmp_path):
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    ids = [n.split()[0] for n in fasta_names(fx.fasta)]
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", "record",
            "-p", "5"]
    got = spawn_ranks(2, _cli_rank, (argv, str(tmp_path)))
    assert got[0] == [((909, 1), 8, (5, 8))] and got[1] == []           # rank 0's device, once
    assert fr_files(str(q)) == sorted(OLD_FILES + NEW_FILES)
    orders = host.compare_orders(8, 5)
    shared, pan, core = reference_compare(np.load(str(q) + "_fr_presence.npz")["bits"], 8, orders)
    assert_compare_files(str(q), ids, shared, orders, pan, core)
    assert [p[7] for p in pan] == [909] * 5
    assert [c[7] for c in core] == [golden("pan8_k27_c3_w4")["spectrum_labels"][8]] * 5
