"""The frequency table's host side (no GPU): host.freq_table - the
specification pg_freq is held to - against a hand-written expectation and an
independent dict-based reference (tests/freq_util.py), the merge of per-rank
tables, the `-g` group file, the flag, the binding's marshalling, and the
committed expectation for pan8_k27_c3 at -a cc -w 4."""
import numpy as np
import pytest

from cc_util import cc_text
from freq_util import (GROUP_COLS, assert_same, fasta_names, golden, reference_freq, reference_text, rows5_of)
from golden_util import Fixture


def random_rows(seed=20, n=20_000, n_labels=700, n_records=90, G=37):
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(5 * n_labels, n_labels, replace=False))      # labels with gaps
    rec_group = rng.permutation(np.arange(n_records) % G).astype(np.int32)
    rec_group[rng.integers(0, n_records, 3)] = -1
    start = rng.integers(0, 10 ** 6, n)
    rows = np.stack([np.sort(rng.integers(0, n_records, n)), start, start + rng.integers(-500, 5000, n),
                     rng.choice([1, -1], n), pool[rng.integers(0, n_labels, n)]], axis=1).astype(np.int64)
    rows[rng.integers(0, n, 50), 4] = -1
    return rows, rec_group, G


def test_hand_written():
    from pangenome_amd import host
    # records 0 and 4 are genome 0, 1 is genome 1, 2 is genome 2, 3 has none
    rec_group = [0, 1, 2, -1, 0]
    rows = [[0, 0, 10, 1, 2],       # label 2: genome 0, + strand, 10 bases
            [0, 30, 18, -1, 2],     # reversed interval: 12 bases
            [1, 5, 6, 1, 2],        # label 2 in genome 1
            [2, 0, 100, -1, 2],     # ... and in genome 2: core
            [4, 7, 9, 1, 2],        # genome 0 again, through its second record
            [1, 0, 50, 1, 7],       # label 7: genomes 1 and 2: shell
            [2, 50, 0, -1, 7],
            [4, 0, 3, -1, 9],       # label 9: genome 0 only: unique
            [1, 0, 1000, 1, -1],    # label -1: skipped
            [3, 0, 1000, 1, 2]]     # a record without a genome: skipped
    t = host.freq_table(np.array(rows, np.int64), rec_group, 3)
    assert (t["n_used"], t["n_skipped"]) == (8, 2)
    assert t["labels"].tolist() == [2, 7, 9]
    assert t["n_genomes"].tolist() == [3, 2, 1]
    assert t["rows"].tolist() == [5, 2, 1] and t["plus"].tolist() == [3, 1, 0]
    assert t["bp"].tolist() == [125, 100, 3]
    assert t["min_len"].tolist() == [1, 50, 3] and t["max_len"].tolist() == [100, 50, 3]
    assert t["bits"].tolist() == [[7], [6], [1]]
    assert t["spectrum_labels"].tolist() == [0, 1, 1, 1] and t["spectrum_bp"].tolist() == [0, 3, 100, 125]
    assert t["g_rows"].tolist() == [4, 2, 2] and t["g_bp"].tolist() == [27, 51, 150]
    assert t["g_core"].tolist() == [24, 1, 100] and t["g_shell"].tolist() == [0, 50, 50]
    assert t["g_unique"].tolist() == [3, 0, 0]
    assert host.freq_text(t) == ("#label\tgenomes\trows\tplus\tbp\tmin\tmax\n"
                                 "2\t3\t5\t3\t125\t1\t100\n7\t2\t2\t1\t100\t50\t50\n9\t1\t1\t0\t3\t3\t3\n")
    assert_same(t, reference_freq(rows, rec_group, 3))
    one = host.freq_table(np.array(rows, np.int64), [0, 0, 0, -1, 0], 1)      # one genome: everything is core
    assert one["g_core"].tolist() == one["g_bp"].tolist() == [228] and one["g_unique"].tolist() == [0]
    empty = host.freq_table(np.zeros((0, 5), np.int64), np.zeros(0, np.int32), 0)
    assert host.freq_text(empty) == "#label\tgenomes\trows\tplus\tbp\tmin\tmax\n"
    assert empty["spectrum_labels"].tolist() == [0]
    with pytest.raises(ValueError):
        host.freq_table(np.array(rows, np.int64), rec_group, 2)
    with pytest.raises(ValueError):
        host.freq_table(np.array(rows, np.int64), rec_group[:3], 3)


def test_random_against_reference():
    from pangenome_amd import host
    rows, rec_group, G = random_rows()
    t = host.freq_table(rows, rec_group, G)
    ref = reference_freq(rows, rec_group, G)
    assert len(ref["labels"]) > 600 and ref["n_skipped"] > 50
    assert_same(t, ref)
    assert host.freq_text(t) == reference_text(ref)
    for g in range(G):
        assert ref["g_core"][g] + ref["g_shell"][g] + ref["g_unique"][g] == ref["g_bp"][g]


def test_merge_of_a_three_way_split():
    """Rows split by record into three parts; genome rec_group[29] also owns
    a record of the next part, so its presence bits must be ORed, not added."""
    from pangenome_amd import host
    rows, rec_group, G = random_rows()
    rec_group[29], rec_group[30] = 5, 5
    whole = host.freq_table(rows, rec_group, G)
    parts = [host.freq_table(rows[(rows[:, 0] >= lo) & (rows[:, 0] < hi)], rec_group, G)
             for lo, hi in ((0, 30), (30, 60), (60, 90))]
    assert all(5 in set(p["pairs"][:, 1].tolist()) for p in parts[:2])
    merged = host.freq_merge(parts, G)
    for k in whole:
        assert np.array_equal(np.asarray(merged[k]), np.asarray(whole[k])), k
    assert_same(merged, reference_freq(rows, rec_group, G))
    assert host.freq_text(host.freq_merge([], 3)) == "#label\tgenomes\trows\tplus\tbp\tmin\tmax\n"


def test_read_groups(tmp_path):
    from pangenome_amd import host
    fn = tmp_path / "groups.tsv"
    fn.write_bytes(b"# seqid\tgenome\n\ng0\tA\ng1\tA\n   \ng2\tB\ng1\tC\n")
    assert host.read_groups(str(fn), [b"g0", b"g1", b"g2"]) == [b"A", b"C", b"B"]        # the later line wins
    with pytest.raises(ValueError, match=r"x1, x2, x3, x4, x5, \.\.\."):
        host.read_groups(str(fn), [b"g0"] + [b"x%d" % i for i in range(1, 8)])
    assert host.seqid(b"g7 len=5\tfoo") == b"g7" and host.seqid(b"") == b""
    # numbered by first appearance over the walked records; the others get -1
    names = [b"g2 x", b"g0", b"g1 y", b"g0 again"]
    grp, gn = host.assign_groups(names, [1, 1, 1, 0], str(fn))
    assert grp.tolist() == [0, 1, 2, -1] and gn == [b"B", b"A", b"C"]
    grp, gn = host.assign_groups(names, [0, 1, 1, 1], "record")
    assert grp.tolist() == [-1, 0, 1, 2] and gn == [b"g0", b"g1", b"g0"]
    with pytest.raises(ValueError, match="g9"):
        host.assign_groups([b"g0", b"g9 z"], [1, 1], str(fn))
    host.assign_groups([b"g0", b"g9 z"], [1, 0], str(fn))                     # not walked: not needed


def test_parse_args_g():
    from pangenome_amd.kmer import parse_args
    assert parse_args(["x", "-i", "f.fa"])["-g"] == ""
    assert parse_args(["x", "-i", "f.fa", "-g", "x"])["-g"] == "x"
    assert parse_args(["x", "-i", "f.fa", "-gx", "-k27"])["-g"] == "x"


def test_binding_marshals_freq_entry_points():
    """The ctypes argument lists of the frequency entry points accept what
    the Context methods pass (a NULL context: each returns PG_EINVAL, no
    device touched)."""
    from pangenome_amd import _lib
    lib = _lib.load()

    class Fake:
        pass
    f = Fake()
    f.lib, f.h = lib, None
    f.n_freq, f.freq_groups_n = 3, 65
    with pytest.raises(_lib.PangenomeError, match=r"pg_freq failed \(-22\)"):
        _lib.Context.freq(f, np.array([0, 1, -1], np.int32), 2)
    with pytest.raises(_lib.PangenomeError, match=r"pg_freq failed \(-22\)"):
        _lib.Context.freq(f, [0, 1], 2, rows=np.zeros((4, 5), np.int64))
    with pytest.raises(_lib.PangenomeError, match="pg_freq_export"):
        _lib.Context.freq_table(f)
    with pytest.raises(_lib.PangenomeError, match="pg_freq_spectrum"):
        _lib.Context.freq_spectrum(f)
    with pytest.raises(_lib.PangenomeError, match="pg_freq_groups"):
        _lib.Context.freq_groups(f)
    with pytest.raises(_lib.PangenomeError, match="pg_freq_format"):
        _lib.Context.freq_text(f)
    with pytest.raises(_lib.PangenomeError, match="pg_freq_format_fd"):
        _lib.Context.freq_write(f, 1)


def test_pan8_oracle_rows_match_the_committed_expectation(oracle_mod):
    """pan8_k27_c3 at -a cc -w 4, one genome per record: 909 table entries
    over 2945 rows (test_cc_labels_carry_meaning's figures), and the spectrum
    and per-genome sums committed as tests/golden/freq/pan8_k27_c3_w4.json."""
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    lines = oracle_mod.run_pipeline(fx.fasta, fx.k, fx.c, fx.ns, cc_text("pan8_k27_c3", 4),
                                    edge_chunk=fx.edge_chunk)["rows"]
    names = fasta_names(fx.fasta)
    assert len(names) == 8
    rows = rows5_of(lines, names)
    t = host.freq_table(rows, np.arange(8, dtype=np.int32), 8)
    assert t["labels"].shape[0] == 909 and int(t["rows"].sum()) == 2945 and t["n_skipped"] == 0
    ref = reference_freq(rows, list(range(8)), 8)
    assert_same(t, ref)
    want = golden("pan8_k27_c3_w4")
    assert want["n_groups"] == 8 and want["n_labels"] == 909 and want["n_rows"] == 2945
    for k in ("spectrum_labels", "spectrum_bp") + GROUP_COLS:
        assert ref[k] == want[k], k
