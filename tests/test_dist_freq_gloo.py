"""The sharded CLI's frequency table (-g) on CPU with gloo: the oracle stands
in for the kernels (OracleShard has no device context, so every rank parses
its own row text and runs host.freq_table); rank 0 merges the partial tables
(host.freq_merge) and writes the four `<in>_fr_*` files."""
import io
import os
import sys

import numpy as np
import pytest

from cc_util import cc_text
from dist_util import ROOT, OracleShard, spawn_ranks
from freq_util import assert_files, as_lists, fasta_names, rows5_of
from golden_util import Fixture

THREE = [0, 0, 1, 1, 1, 1, 2, 2]                     # g0, g1 / g2 .. g5 / g6, g7


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
        bounds = pdist.shard_bounds(np.frombuffer(open(argv[2], "rb").read(), np.uint8), world)
    finally:
        dist.destroy_process_group()
    q.put((rank, (out.getvalue(), bounds)))


def _expect(oracle_mod, fx):
    """host.freq_table over the oracle's rows of the whole input, three genomes."""
    from pangenome_amd import host
    lines = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, cc_text("pan8_k27_c3", 4),
                                    edge_chunk=fx.edge_chunk)["rows"]
    return as_lists(host.freq_table(rows5_of(lines, fasta_names(fx.fasta)), THREE, 3))


@pytest.mark.parametrize("world", [2, 3])
def test_dist_cli_freq(oracle_mod, tmp_path, world):
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    ids = [n.split()[0] for n in fasta_names(fx.fasta)]
    gf = tmp_path / "groups.tsv"
    gf.write_text("".join("%s\t%s\n" % (i, "ABC"[g]) for i, g in zip(ids, THREE)))
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4"]
    outs = spawn_ranks(world, _cli_rank, (argv,))
    assert not [f for f in os.listdir(tmp_path) if "_fr_" in f]          # without -g no file is written
    plain = [ln for ln in outs[0][0].split("\n") if not ln.startswith("# finished in")]
    outs = spawn_ranks(world, _cli_rank, (argv + ["-g", str(gf)],))
    with_g = [ln for ln in outs[0][0].split("\n") if not ln.startswith("# finished in")]
    assert [ln for ln in with_g if ln != "# the mcl has been ran"] == plain
    assert_files(str(q), _expect(oracle_mod, fx), ["A", "B", "C"])
    if world == 3:
        # genome B (g2 .. g5) has records on two ranks
        starts = [fx.fasta.index(b">" + i.encode()) for i in ids[2:6]]
        b = outs[0][1]
        assert len({max(r for r in range(world) if b[r] <= s) for s in starts}) >= 2
