"""tests/walk_util.py against the oracle alone (no GPU): the properties of
its inputs that tests/test_gpu_walks.py relies on."""
import numpy as np
import pytest

import walk_util as wu
from cc_util import xyz_arrays
from golden_util import Fixture

KS = (1, 2, 6, 11, 13, 14, 20, 27)      # tests/test_gpu_walks.py's


def test_standard_input_shape():
    for k in KS:
        fasta = wu.standard_fasta(k)
        n, hs, hl = wu.record_table(fasta)
        assert n.shape[0] == 20 and len(fasta) < 40_000
        for want in (0, 1, k - 1, k, k + 1, k + 2, k + 14, k + 15, k + 16, k + 31, k + 32, 200, 237, 3000, 3040):
            assert want in n.tolist(), (k, want)
        names = wu.names_of(fasta)
        assert len(set(names)) == 20 and all(b" " in x for x in names)
        assert wu.subset_fasta(fasta, np.ones(20, np.uint8)) == fasta
        sub = wu.subset_fasta(fasta, wu.flag_patterns(fasta, k)["alternate"])
        assert wu.names_of(sub) == names[1::2] and wu.record_table(sub)[0].tolist() == n[1::2].tolist()
        assert wu.subset_fasta(fasta, wu.flag_patterns(fasta, k)["none"]) == b""
        short = wu.subset_fasta(fasta, wu.flag_patterns(fasta, k)["short"])
        assert wu.record_table(short)[0].tolist() == [k + 1]


@pytest.mark.parametrize("c", [3, 2])
@pytest.mark.parametrize("k", KS)
def test_dense_table_makes_every_window_a_hit(oracle_mod, k, c):
    """Under one constant label every walk of a record with n > k is one row
    from 0: each window is a hit, the first (idx 0) is never taken (idx >
    last with last = 0), idx 1 opens the row and every later taken hit
    extends it.  Taken hits are idx 1, 1 + (k + 1), 1 + 2 (k + 1), ...
    (last = idx + k), so the row ends k past the last of those that is a
    window (idx <= n - k).  A record with n <= k has at most the idx 0 hit:
    no row."""
    fasta = wu.standard_fasta(k)
    run = oracle_mod.OracleRun(fasta, k, c)
    keys, vals = wu.dense_table(*run.dbg())
    assert keys.shape[0] == np.unique(np.stack([keys, vals]), axis=1).shape[1]
    lines = run.rows((keys, vals, np.full(keys.shape[0], 7, np.int64)))
    want = []
    n, _, _ = wu.record_table(fasta)
    for name, ln in zip(wu.names_of(fasta), n.tolist()):
        if ln <= k:
            continue
        end = k + 1 + (ln - k - 1) // (k + 1) * (k + 1)
        want.append("%s\t0\t%d\t+\t7" % (name.decode(), end))
        if c & 1:
            want.append("%s\t%d\t%d\t-\t7" % (name.decode(), ln - end, ln))
    assert lines == want
    assert len(want) == int((n > k).sum()) * (2 if c & 1 else 1) >= 16


def test_k2_edges_outgrow_the_edge_table_floor(oracle_mod):
    """walk_edges starts its edge table at max(1024, 4 (n_rdbg + 1)) slots: at
    k = 2 (at most 26 keys) more than 1024 distinct edges force the x4 re-run."""
    fasta = wu.standard_fasta(2)
    for c in (3, 2):
        run = oracle_mod.OracleRun(fasta, 2, c)
        keys, _ = run.dbg()
        assert keys.shape[0] <= 26
        run.set_rdbg(keys)
        t, cnt = run.edges()
        assert t.shape[0] > 1024, (c, t.shape[0])


def test_label_dict_restates_the_oracle():
    from oracle import oracle
    fx = Fixture("pan8_k27_mcl")
    assert fx.mcl
    want = oracle.label_table(fx.xyz, fx.mcl)
    t, _ = xyz_arrays(fx.xyz)
    ent, n_lines = wu.mcl_entries(fx.mcl)
    got = wu.label_dict(t, ent, n_lines)
    assert n_lines == fx.mcl.count("\n") and len(ent) > n_lines
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    mk, mv, mi = wu.mcl_arrays(ent)
    assert np.array_equal(mk, want[0][:mk.shape[0]]) and np.array_equal(mi, want[2][:mk.shape[0]])
    # a later `.mcl` entry replaces the id, not the position
    k2, v2, i2 = wu.label_dict([[5, 1, 6, 2], [6, 2, 5, 1], [9, 0, 5, 1]], [(6, 2, 0), (7, 7, 1), (6, 2, 2)], 10)
    assert (k2.tolist(), v2.tolist(), i2.tolist()) == ([6, 7, 5, 9], [2, 7, 1, 0], [2, 1, 10, 11])
