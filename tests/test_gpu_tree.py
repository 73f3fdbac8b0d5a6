"""The genome tree on the device (pg_tree_nj) against the host specification
(host.tree_nj, itself checked against tests/tree_util.py's loops in
test_tree_host.py): exactly, at the default number of arg-min blocks and at
PG_TUNE_NJ_BLOCKS 7 (28 waves: rows of one matrix fall in different blocks).
A reference is computed once per input and shared by both."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

from freq_util import fasta_names
from golden_util import Fixture
from tree_util import (ONE, additive, as_lists, hamming, joins_as_sets, joins_of_newick, newick_leaf_dist,
                       parse_newick, reference_nj, star)

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 129, 257]


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    yield c
    c.close()


@pytest.fixture(params=[0, 7], ids=["default", "blocks7"])
def blocks(ctx, request):
    from pangenome_amd import _lib
    ctx.tune(_lib.PG_TUNE_NJ_BLOCKS, request.param)
    yield request.param
    ctx.tune(_lib.PG_TUNE_NJ_BLOCKS, 0)


def spec(d):
    from pangenome_amd import host
    return as_lists(*host.tree_nj(d))


def device(ctx, d, n=None):
    nj = ctx.tree_nj(d, n)
    got = as_lists(ctx.tree_joins(), ctx.tree_root())
    assert nj == len(got[0])
    return got


def check(ctx, d, want=None):
    want = spec(d) if want is None else want
    assert device(ctx, d) == want
    assert np.array_equal(ctx.tree_dist(), d)
    return want


# ------------------------------------------------------------ inputs, made once
@functools.lru_cache(maxsize=None)
def size_case(n):
    d = hamming(n, seed=7)
    return d, spec(d)


@functools.lru_cache(maxsize=None)
def tie_case(kind):
    n = 70
    if kind == "star":
        d = star(n)
    else:
        d = star(n, 100)
        d[n - 2, n - 1] = d[n - 1, n - 2] = 1
        if kind == "two":
            d[0, 1] = d[1, 0] = 1
    return d, spec(d)


@functools.lru_cache(maxsize=None)
def magnitude_case(kind):
    n = 300
    if kind == "all":
        d = star(n, 2 ** 31)
    else:
        rng = np.random.default_rng(31)
        u = np.triu(rng.integers(0, 2, (n, n)), 1)
        d = (2 ** 31 - 1 + u + u.T).astype(np.uint64)
        np.fill_diagonal(d, 0)
    return d, spec(d)


@functools.lru_cache(maxsize=None)
def additive_case(n):
    d, total = additive(n, seed=n)
    return d, total, spec(d)


# ------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, blocks, n):
    """63, 64 and 65 straddle the wave width; 129 and 257 give rows of more
    than one 64-column step and, at 257, more than one unrolled step."""
    d, want = size_case(n)
    check(ctx, d, want)
    assert len(want[0]) == max(n - 3, 0) and len(want[1]) == min(n, 3)
    if n <= 40:
        assert want == reference_nj(d.tolist())


# ------------------------------------------------------------ 2. ties
def test_star_takes_the_smallest_live_pair(ctx, blocks):
    """Every off-diagonal entry 2 at n = 70: every Q of a join is equal, so
    every join takes the two smallest live slots - slot 0 (leaf 0, then the
    node of the join before) and the next leaf."""
    d, want = tie_case("star")
    check(ctx, d, want)
    assert [row[:2] for row in want[0]] == [(0 if t == 0 else 70 + t - 1, t + 1) for t in range(67)]
    assert want == reference_nj(d.tolist())


def test_unique_minimum_in_the_last_two_slots(ctx, blocks):
    d, want = tie_case("last")
    check(ctx, d, want)
    assert want[0][0][:2] == (68, 69)


def test_equal_minima_in_the_first_and_the_last_rows(ctx, blocks):
    """(0, 1) and (68, 69) have the same Q; at 7 blocks of 4 waves row 0 is
    block 0's and row 68 block 3's."""
    d, want = tie_case("two")
    check(ctx, d, want)
    assert want[0][0][:2] == (0, 1) and want[0][1][:2] == (68, 69)


# ------------------------------------------------------------ 3. magnitude
@pytest.mark.parametrize("kind", ["all", "mixed"])
def test_magnitude(ctx, blocks, kind):
    """Entries of 2^31 at n = 300: |Q| = |298 D - 2 x 299 D| passes 2^53 (and
    2^55), so a float form or one cut to 32 bits gives another tree."""
    d, want = magnitude_case(kind)
    D = int(d[0, 1]) << 16
    assert abs(298 * D - 2 * 299 * (2 ** 31 - 1 << 16)) > 2 ** 53
    check(ctx, d, want)
    if kind == "all":
        assert want[0][0] == (0, 1, 2 ** 46, 2 ** 46)


# ------------------------------------------------------------ 4. additive trees
@pytest.mark.parametrize("n", [40, 200])
def test_additive_trees_come_back_exactly(ctx, blocks, n):
    from pangenome_amd import host
    d, total, want = additive_case(n)
    check(ctx, d, want)
    joins, root = ctx.tree_joins(), ctx.tree_root()
    lens = [v for row in want[0] for v in row[2:]] + [v for _, v in want[1]]
    assert all(v % ONE == 0 for v in lens) and sum(lens) == total * ONE
    names = ["g%d" % i for i in range(n)]
    text = host.tree_newick(names, joins, root)
    assert np.array_equal(newick_leaf_dist(text, names), d * np.uint64(1000000))


# ------------------------------------------------------------ 5. the device source
def make_rows(rec, start, length, strand, label):
    rec = np.asarray(rec, np.int64)
    start = np.broadcast_to(np.asarray(start, np.int64), rec.shape)
    return np.stack([rec, start, start + np.broadcast_to(np.asarray(length, np.int64), rec.shape),
                     np.broadcast_to(np.asarray(strand, np.int64), rec.shape),
                     np.broadcast_to(np.asarray(label, np.int64), rec.shape)], axis=1).astype(np.int64)


def random_rows(n_records, G, n=20_000, n_labels=600, seed=11):
    rng = np.random.default_rng(seed)
    rec_group = rng.permutation(np.arange(n_records) % G).astype(np.int32)
    rows = make_rows(np.sort(rng.integers(0, n_records, n)), rng.integers(0, 10 ** 7, n), rng.integers(20, 2000, n),
                     rng.choice([1, -1], n), rng.integers(0, n_labels, n))
    return rows, rec_group


def test_device_source(ctx, blocks):
    """Rows -> pg_freq -> pg_freq_compare (bits NULL) -> pg_tree_nj(NULL): the
    specification applied to the exported shared matrix; a later pg_freq
    does not drop the tree."""
    G = 37
    rows, rec_group = random_rows(90, G)
    ctx.freq(rec_group, G, rows=rows)
    ctx.freq_compare(None)
    s = ctx.freq_shared().astype(np.int64)
    dg = np.diag(s)
    d = (dg[:, None] + dg[None, :] - 2 * s).astype(np.uint64)
    assert d.any()
    want = spec(d)
    assert ctx.tree_nj() == G - 3
    got = as_lists(ctx.tree_joins(), ctx.tree_root())
    assert got == want and np.array_equal(ctx.tree_dist(), d)
    ctx.freq(rec_group, G, rows=rows[:1000])                 # (drops the comparison, not the tree)
    assert as_lists(ctx.tree_joins(), ctx.tree_root()) == want and np.array_equal(ctx.tree_dist(), d)
    assert ctx.lib.pg_tree_nj(ctx.h, None, G, None) == -22   # no comparison any more; the tree stays
    assert as_lists(ctx.tree_joins(), ctx.tree_root()) == want


# ------------------------------------------------------------ 6. refusals
def test_refusals_keep_the_previous_tree(ctx, blocks):
    from pangenome_amd._lib import Context, ptr
    lib = ctx.lib
    d, want = size_case(5)
    check(ctx, d, want)

    def kept():
        assert as_lists(ctx.tree_joins(), ctx.tree_root()) == want and np.array_equal(ctx.tree_dist(), d)
    nj = C.c_uint64(99)
    for bad in ("asym", "diag", "big"):
        e = hamming(9, seed=3)
        if bad == "asym":
            e[1, 3] += np.uint64(1)
        elif bad == "diag":
            e[2, 2] = 1
        else:
            e[0, 4] = e[4, 0] = 2 ** 31 + 1
        assert lib.pg_tree_nj(ctx.h, ptr(e), 9, C.byref(nj)) == -22, bad
        assert nj.value == 99
        kept()
    assert lib.pg_tree_nj(None, ptr(d), 5, None) == -22
    one = np.zeros(1, np.uint64)
    assert lib.pg_tree_nj(ctx.h, ptr(one), 16385, None) == -34          # decided before the matrix is read
    kept()
    # dist == NULL: with another n than the comparison's G, and on a fresh context
    from compare_util import random_bits
    ctx.freq_compare(None, bits=random_bits(50, 6, seed=2), n_groups=6)
    assert lib.pg_tree_nj(ctx.h, None, 5, None) == -22 and lib.pg_tree_nj(ctx.h, None, 7, None) == -22
    kept()
    fresh = Context(27, 0)
    try:
        assert lib.pg_tree_nj(fresh.h, None, 0, None) == -22
        assert lib.pg_tree_dist(fresh.h, None, 0) == -22 and lib.pg_tree_joins(fresh.h, None, None, None, None, 0) == -22
        assert lib.pg_tree_root(fresh.h, None, None, None) == -22 and lib.pg_tree_time(fresh.h, None, None) == -22
    finally:
        fresh.close()
    # a short cap on every export (5 leaves: 25 cells, 2 joins)
    buf = np.zeros(25, np.uint64)
    u32 = np.zeros(2, np.uint32)
    assert lib.pg_tree_dist(ctx.h, ptr(buf), 24) == -34 and lib.pg_tree_dist(ctx.h, ptr(buf), 25) == 0
    assert buf.reshape(5, 5).tolist() == d.tolist()
    assert lib.pg_tree_joins(ctx.h, ptr(u32), None, None, None, 1) == -34
    assert lib.pg_tree_joins(ctx.h, ptr(u32), None, None, None, 2) == 0
    assert u32.tolist() == [row[0] for row in want[0]]
    kept()
    for bad in (-1, 4097):
        assert lib.pg_tune(ctx.h, 32, C.c_int64(bad)) == -22
    ms, cells = ctx.tree_time()
    assert ms >= 0 and cells == 5 * 5 + 4 * 4


# ------------------------------------------------------------ 7. determinism
def test_determinism(ctx, blocks):
    """The same input twice on one context, and once with every new device
    buffer filled with 0xA5: equal tables (nothing read that no kernel wrote)."""
    from pangenome_amd import _lib
    d, want = size_case(129)
    a = device(ctx, d)
    b = device(ctx, d)
    ctx.tune(_lib.PG_TUNE_POISON, 0xA5)
    try:
        c = device(ctx, d)
        dist = ctx.tree_dist()
    finally:
        ctx.tune(_lib.PG_TUNE_POISON, -1)
    assert a == b == c == want and np.array_equal(dist, d)


# ------------------------------------------------------------ 8. the CLI
TREE_FILES = ["_fr_dist.tsv", "_fr_tree.npz", "_fr_tree.nwk", "_fr_tree.tsv"]


def _run(d, fasta, extra):
    from pangenome_amd import kmer
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    kmer.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4", "-g", "record"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def _fr(prefix):
    d, base = os.path.split(prefix)
    return sorted(f[len(base):] for f in os.listdir(d) if f.startswith(base + "_fr_"))


def _matrix(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b""
    head = lines[0].split(b"\t")
    assert head[0] == b"#genome"
    rows = [ln.split(b"\t") for ln in lines[1:-1]]
    assert [r[0] for r in rows] == head[1:]
    return head[1:], np.array([[int(v) for v in r[1:]] for r in rows], np.int64).reshape(len(rows), len(rows))


def test_cli(tmp_path):
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    ids = [n.split()[0] for n in fasta_names(fx.fasta)]
    q0, plain = _run(tmp_path / "plain", fx.fasta, ["-p", "1"])
    q, lines = _run(tmp_path / "tree", fx.fasta, ["-T", "1"])
    assert lines == plain                                    # stdout is that of a run without -T
    assert not any("tree" in f or "dist" in f for f in _fr(q0))          # which writes none of the new files
    assert sorted(set(_fr(q)) - set(_fr(q0))) == TREE_FILES
    assert not [f for f in os.listdir(os.path.dirname(q)) if f.endswith(".tmp")]
    # the distances: formed from the shared matrix of the -p 1 run
    names, s = _matrix(q0 + "_fr_shared.tsv")
    dg = np.diag(s)
    names_d, d = _matrix(q + "_fr_dist.tsv")
    assert names_d == names == [x.encode() for x in ids]
    assert np.array_equal(d, dg[:, None] + dg[None, :] - 2 * s)
    # the tables and the text
    z = np.load(q + "_fr_tree.npz")
    assert sorted(z.files) == sorted(["genomes", "dist", "left", "right", "left_len", "right_len", "root_child",
                                      "root_len", "frac_bits"])
    assert int(z["frac_bits"]) == 16 and z["genomes"].tolist() == names and np.array_equal(z["dist"], d)
    joins = {k: z[k] for k in ("left", "right", "left_len", "right_len")}
    assert as_lists(joins, (z["root_child"], z["root_len"])) == spec(d.astype(np.uint64))
    text = open(q + "_fr_tree.nwk", "rb").read()
    assert text == host.tree_newick(names, joins, (z["root_child"], z["root_len"]))
    _, leaves = parse_newick(text)
    assert sorted(leaves.values()) == sorted(ids)
    assert joins_of_newick(text, ids) == joins_as_sets(ids, as_lists(joins, (z["root_child"], z["root_len"]))[0], 8)
    tsv = open(q + "_fr_tree.tsv").read().split("\n")
    assert tsv[0] == "#node\tleft\tright\tleft_len\tright_len" and tsv[-1] == "" and tsv[-2].startswith("#root\t")
    assert [ln.split("\t")[:3] for ln in tsv[1:-2]] == [
        [str(8 + t), str(int(a)), str(int(b))] for t, (a, b) in enumerate(zip(z["left"], z["right"]))]
    assert tsv[-2].split("\t")[1:4] == [str(int(c)) for c in z["root_child"]]


def test_cli_variant_tree(tmp_path):
    fx = Fixture("pan8_k27_c3")
    ids = [n.split()[0] for n in fasta_names(fx.fasta)]
    q, _ = _run(tmp_path / "var", fx.fasta, ["-b", "5", "-V", ids[0], "-A", "1", "-T", "1"])
    assert set(TREE_FILES + ["_fr_vartree.nwk", "_fr_vardist.tsv"]) <= set(_fr(q))
    assert not [f for f in os.listdir(os.path.dirname(q)) if f.endswith(".tmp")]
    text = open(q + "_fr_vartree.nwk", "rb").read()
    _, leaves = parse_newick(text)
    assert sorted(leaves.values()) == sorted(ids)
    # the Hamming matrix of the GT carrier columns of the primitive VCF, read as text
    body = [ln.split(b"\t") for ln in open(q + "_fr_primitives.vcf", "rb").read().split(b"\n")
            if ln and not ln.startswith(b"##")]
    assert body[0][9:] == [x.encode() for x in ids] and len(body) > 1
    carry = np.array([[cell.split(b"/")[-1] == b"1" for cell in ln[9:]] for ln in body[1:]], np.int64)
    assert carry.any()
    sh = carry.T @ carry
    dg = np.diag(sh)
    names, d = _matrix(q + "_fr_vardist.tsv")
    assert names == [x.encode() for x in ids]
    assert np.array_equal(d, dg[:, None] + dg[None, :] - 2 * sh)
    from pangenome_amd import host
    assert text == host.tree_newick(names, *host.tree_nj(d.astype(np.uint64)))
