"""The sharded CLI's genome comparison (-p) on CPU with gloo: the oracle
stands in for the kernels (OracleShard has no freq_compare, so rank 0 runs
host.freq_compare over the merged table's presence bits) and writes the four
comparison files, which must equal what the independent reference gives from
the written `_fr_presence.npz`."""
import io
import os
import sys

import pytest

from compare_util import NEW_FILES, OLD_FILES, assert_compare_files, fr_files, reference_compare
from dist_util import ROOT, OracleShard, spawn_ranks
from freq_util import fasta_names
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
    finally:
        dist.destroy_process_group()
    q.put((rank, out.getvalue()))


@pytest.mark.parametrize("world", [2, 3])
def test_dist_cli_compare(tmp_path, world):
    import numpy as np
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    ids = [n.split()[0] for n in fasta_names(fx.fasta)]
    gf = tmp_path / "groups.tsv"
    gf.write_text("".join("%s\t%s\n" % (i, "ABC"[g]) for i, g in zip(ids, THREE)))
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-g", str(gf)]
    outs = spawn_ranks(world, _cli_rank, (argv,))
    assert fr_files(str(q)) == OLD_FILES                                  # without -p there is no fifth file
    plain = [ln for ln in outs[0].split("\n") if not ln.startswith("# finished in")]
    before = {s: open(str(q) + s, "rb").read() for s in OLD_FILES}
    outs = spawn_ranks(world, _cli_rank, (argv + ["-p", "4"],))
    with_p = [ln for ln in outs[0].split("\n") if not ln.startswith("# finished in")]
    assert [ln for ln in with_p if ln != "# the mcl has been ran"] == plain
    assert fr_files(str(q)) == sorted(OLD_FILES + NEW_FILES)
    assert {s: open(str(q) + s, "rb").read() for s in OLD_FILES if s.endswith(".tsv")} == \
        {s: b for s, b in before.items() if s.endswith(".tsv")}
    z = np.load(str(q) + "_fr_presence.npz")
    assert z["bits"].shape == (909, 1)
    orders = host.compare_orders(3, 4)
    shared, pan, core = reference_compare(z["bits"], 3, orders)
    assert_compare_files(str(q), ["A", "B", "C"], shared, orders, pan, core)
    assert pan[0][2] == 909 and shared[1][1] >= max(shared[0][1], shared[1][2])
