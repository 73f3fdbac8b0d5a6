"""The genome comparison's host side (no GPU): the CLI's genome orders,
host.freq_compare - the specification pg_freq_compare is held to - against an
independent set-based reference (tests/compare_util.py), the four files, the
binding's marshalling and the flag."""
import numpy as np
import pytest

from compare_util import (assert_compare_files, as_lists, check_identities, files_of, pack, random_bits,
                          random_orders, reference_compare)

PIN_8_3 = [[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 0, 6, 1, 3, 7, 2], [1, 7, 5, 4, 0, 6, 3, 2]]


def test_compare_orders():
    from pangenome_amd import host
    o = host.compare_orders(8, 3)
    assert o.dtype == np.int32 and o.tolist() == PIN_8_3
    for G in (1, 2, 65):
        o = host.compare_orders(G, 5)
        assert o.shape == (5, G) and o[0].tolist() == list(range(G))
        assert all(sorted(r) == list(range(G)) for r in o.tolist())
    assert len({tuple(r) for r in host.compare_orders(65, 5).tolist()}) == 5
    assert host.compare_orders(4, 0).shape == (0, 4) and host.compare_orders(0, 2).shape == (2, 0)


@pytest.mark.parametrize("G,n", [(1, 5), (3, 70), (64, 64), (65, 130)])
def test_freq_compare_against_sets(G, n):
    """One all-ones and one all-zeros row in each case; the order-0 identity
    and shuffled orders; the three identities of the definitions."""
    from pangenome_amd import host
    bits = random_bits(n, G, seed=G + n)
    assert int(bits[0, -1]) == (1 << ((G - 1) % 64 + 1)) - 1 and not bits[n - 1].any()
    orders = np.concatenate([host.compare_orders(G, 2), random_orders(G, 2)])
    got = as_lists(*host.freq_compare(bits, G, orders))
    ref = reference_compare(bits, G, orders)
    assert got == ref
    check_identities(bits, G, orders, *got)
    s, pan, core = host.freq_compare(bits, G, orders)
    assert s.dtype == pan.dtype == core.dtype == np.uint64 and s.shape == (G, G) and pan.shape == core.shape == (4, G)


def test_freq_compare_edges():
    from pangenome_amd import host
    s, pan, core = host.freq_compare(np.zeros((0, 1), np.uint64), 3, [[2, 0, 1]])
    assert s.tolist() == [[0] * 3] * 3 and pan.tolist() == core.tolist() == [[0, 0, 0]]
    s, pan, core = host.freq_compare(np.zeros((0, 0), np.uint64), 0, np.zeros((2, 0), np.int32))
    assert s.shape == (0, 0) and pan.shape == core.shape == (2, 0)
    s, pan, core = host.freq_compare(pack([[1, 0], [1, 1]]), 2, None)
    assert s.tolist() == [[2, 1], [1, 1]] and pan.shape == (0, 2)
    with pytest.raises(ValueError):
        host.freq_compare(pack([[1, 0]]), 2, [[0, 0]])
    with pytest.raises(ValueError):
        host.freq_compare(pack([[1, 0]]), 2, [[0, 2]])
    with pytest.raises(ValueError):
        host.freq_compare(np.array([[4]], np.uint64), 2, [[0, 1]])
    with pytest.raises(ValueError):
        host.freq_compare(np.zeros((1, 0), np.uint64), 0, None)


def test_write_compare_files(tmp_path):
    """Hand-written bytes: genome c holds no label, so the (c, c) Jaccard
    cell has an empty union and reads 0.000000."""
    from pangenome_amd import host
    bits = pack([[1, 1, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    orders = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    shared, pan, core = host.freq_compare(bits, 3, orders)
    prefix = str(tmp_path / "in.fa")
    host.write_compare_files(prefix, [b"a", b"b", b"c"], shared, orders, pan, core)
    assert open(prefix + "_fr_shared.tsv", "rb").read() == b"#genome\ta\tb\tc\na\t3\t2\t0\nb\t2\t3\t0\nc\t0\t0\t0\n"
    assert open(prefix + "_fr_jaccard.tsv", "rb").read() == (
        b"#genome\ta\tb\tc\na\t0.000000\t0.500000\t1.000000\nb\t0.500000\t0.000000\t1.000000\n"
        b"c\t1.000000\t1.000000\t0.000000\n")
    assert open(prefix + "_fr_curve.tsv", "rb").read() == (
        b"#genomes\torders\tpan_sum\tpan_min\tpan_max\tcore_sum\tcore_min\tcore_max\n"
        b"1\t2\t3\t0\t3\t3\t0\t3\n2\t2\t7\t3\t4\t2\t0\t2\n3\t2\t8\t4\t4\t0\t0\t0\n")
    shared, pan, core = reference_compare(bits, 3, orders)
    assert_compare_files(prefix, ["a", "b", "c"], shared, orders, pan, core)
    assert files_of(["a", "b", "c"], shared, orders.tolist(), pan, core)["_fr_jaccard.tsv"].endswith("\t0.000000\n")
    # a larger random case through both writers
    bits, orders = random_bits(130, 65, seed=9), random_orders(65, 3)
    names = ["g%d" % i for i in range(65)]
    shared, pan, core = host.freq_compare(bits, 65, orders)
    host.write_compare_files(prefix, [x.encode() for x in names], shared, orders, pan, core)
    shared, pan, core = reference_compare(bits, 65, orders)
    assert_compare_files(prefix, names, shared, orders, pan, core)


def test_binding_marshals_compare_entry_points():
    """The ctypes argument lists of the three comparison entry points accept
    what the Context methods pass (a NULL context: each returns PG_EINVAL, no
    device touched)."""
    from pangenome_amd import _lib
    lib = _lib.load()

    class Fake:
        pass
    f = Fake()
    f.lib, f.h = lib, None
    f.freq_groups_n = 65
    with pytest.raises(_lib.PangenomeError, match=r"pg_freq_compare failed \(-22\)"):
        _lib.Context.freq_compare(f, random_orders(65, 2))
    with pytest.raises(_lib.PangenomeError, match=r"pg_freq_compare failed \(-22\)"):
        _lib.Context.freq_compare(f, random_orders(3, 2), bits=pack([[1, 0, 1]]), n_groups=3)
    with pytest.raises(_lib.PangenomeError, match=r"pg_freq_compare failed \(-22\)"):
        _lib.Context.freq_compare(f, None, bits=np.zeros((0, 2), np.uint64), n_groups=70)
    f.cmp_groups_n, f.cmp_orders_n = 3, 2
    with pytest.raises(_lib.PangenomeError, match=r"pg_freq_shared failed \(-22\)"):
        _lib.Context.freq_shared(f)
    with pytest.raises(_lib.PangenomeError, match=r"pg_freq_curve failed \(-22\)"):
        _lib.Context.freq_curves(f)
    assert (_lib.PG_TUNE_CMP_CHUNK, _lib.PG_TUNE_CMP_FORM) == (22, 23)


def test_parse_args_p(tmp_path):
    import io
    from pangenome_amd import kmer
    assert kmer.parse_args(["x", "-i", "f.fa"])["-p"] == "0"
    assert kmer.parse_args(["x", "-i", "f.fa", "-p3", "-g", "record"])["-p"] == "3"
    assert kmer.parse_args(["x", "-i", "f.fa", "-p", "3"])["-p"] == "3"
    # refused before anything is read or built: the manual, then SystemExit
    for extra in (["-p", "3"], ["-p", "-1", "-g", "record"], ["-p", "x", "-g", "record"], ["-p1.5", "-g", "record"]):
        out = io.StringIO()
        with pytest.raises(SystemExit):
            kmer.entry_point(["x", "-i", str(tmp_path / "missing.fa"), "-a", "cc"] + extra, out=out)
        lines = out.getvalue().split("\n")
        assert lines[0] == "Usage:" and sum(ln.startswith("  -p:") for ln in lines) == 1
