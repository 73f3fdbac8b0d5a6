"""The built-in clusterer's host side (no GPU): host.cluster_cc, the
executable specification of pg_cluster_cc, against the networkx-made
expectations (tests/golden/cc) and an independent union-find; the CLI flags;
the binding's marshalling."""
import numpy as np
import pytest

from cc_util import cc_cases, cc_text, random_graph, reference_mcl, xyz_arrays
from golden_util import Fixture


def _check_table(host, text, keys, vals, ids):
    mk, mv, mi, n_lines = host.mcl_labels(text)
    assert np.array_equal(keys, mk) and np.array_equal(vals, mv) and np.array_equal(ids, mi)
    assert keys.dtype == vals.dtype == ids.dtype == np.int64
    assert n_lines == text.count("\n")


@pytest.mark.parametrize("name,w", cc_cases())
def test_host_cluster_cc_matches_goldens(name, w):
    from pangenome_amd import host
    t, c = xyz_arrays(Fixture(name).xyz)
    text, keys, vals, ids = host.cluster_cc(t, c, w)
    assert text == cc_text(name, w)
    _check_table(host, text, keys, vals, ids)


def test_goldens_are_the_issue_cases():
    assert cc_cases() == [("edge_k27", 1), ("edge_k27", 2), ("edge_k5", 1), ("pan8_k15", 4), ("pan8_k27_c2", 2),
                          ("pan8_k27_c3", 1), ("pan8_k27_c3", 4), ("polya_k27", 1), ("test_k27", 1)]
    sizes = lambda n, w: [ln.count("\t") + 1 for ln in cc_text(n, w).splitlines()]
    assert sizes("pan8_k27_c3", 1) == [5103, 5102]
    assert len(sizes("pan8_k27_c3", 4)) == 6063
    assert len(sizes("pan8_k27_c2", 2)) == 2625
    assert sizes("edge_k27", 1) == [16, 14, 10, 5, 3]
    assert sizes("polya_k27", 1) == [17, 17]
    assert len(sizes("edge_k5", 1)) == 1
    assert cc_text("test_k27", 1) == ""


@pytest.mark.parametrize("E", [1500, 6000])
@pytest.mark.parametrize("w", [1, 3, 6])
def test_host_cluster_cc_matches_independent_union_find(E, w):
    from pangenome_amd import host
    t, c = random_graph(100 + E, 2000, E)
    text, keys, vals, ids = host.cluster_cc(t, c, w)
    assert text == reference_mcl(t, c, w)
    _check_table(host, text, keys, vals, ids)
    if w == 6:                                        # above every weight: one line per node, in id order
        assert ids.tolist() == list(range(ids.shape[0]))


def test_host_cluster_cc_small_cases():
    from pangenome_amd import host
    z = host.cluster_cc(np.zeros((0, 4), np.uint64), np.zeros(0, np.int64), 1)
    assert z[0] == "" and all(a.shape == (0,) for a in z[1:])
    # a self-loop is one node; one key with two values is two nodes
    assert host.cluster_cc([[7, 1, 7, 1]], [9], 1)[0] == "7_1\n"
    t = [[5, 0, 8, 0], [5, 1, 9, 0], [2 ** 64 - 1, 3, 2 ** 64 - 1, 3]]
    assert host.cluster_cc(t, [1, 1, 1], 1)[0] == "5_0\t8_0\n5_1\t9_0\n18446744073709551615_3\n"
    with pytest.raises(ValueError):
        host.cluster_cc(t, [1, 1, 1], 0)


def test_parse_args_cluster_flags():
    from pangenome_amd.kmer import parse_args
    a = parse_args(["x", "-i", "f.fa", "-a", "cc", "-w", "4"])
    assert a["-a"] == "cc" and a["-w"] == "4" and a["-i"] == "f.fa"
    a = parse_args(["x", "-i", "f.fa", "-acc", "-w4", "-k27"])
    assert a["-a"] == "cc" and a["-w"] == "4" and a["-k"] == "27"
    a = parse_args(["x", "-i", "f.fa"])
    assert a["-a"] == "mcl" and a["-w"] == "1"


def test_unknown_cluster_method_is_usage(tmp_path):
    import io
    from pangenome_amd import kmer
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["x", "-i", str(tmp_path / "f.fa"), "-a", "louvain"], out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert lines[-3] == "  -c: complementary reverse sequence. 00,01,10,11"


def test_binding_marshals_cluster_entry_points():
    """The ctypes argument lists of the clustering entry points accept what
    the Context methods pass (a NULL context: PG_EINVAL, no device touched)."""
    from pangenome_amd import _lib
    lib = _lib.load()

    class Fake:
        pass
    f = Fake()
    f.lib, f.h = lib, None
    t, c = random_graph(1, 10, 5)
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_cc failed \(-22\)"):
        _lib.Context.cluster_cc(f, t, c, 2)
    with pytest.raises(_lib.PangenomeError, match=r"pg_cluster_cc failed \(-22\)"):
        _lib.Context.cluster_cc(f)
    with pytest.raises(_lib.PangenomeError, match=r"pg_clusters_format failed \(-22\)"):
        _lib.Context.clusters_text(f)
    with pytest.raises(_lib.PangenomeError, match=r"pg_clusters_format_fd failed \(-22\)"):
        _lib.Context.clusters_write(f, 1)
