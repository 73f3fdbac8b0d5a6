"""Tree support on the device (pg_tree_bootstrap) against the host
specification (host.tree_bootstrap, itself checked against tests/boot_util.py's
loops in test_boot_host.py): the replicate matrices, the replicate joins and
the support, each exactly, in every form of the neighbour joining and at every
batch size.  A reference is computed once per input and shared."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

from boot_util import clean_table, coin_table, mixed_table, star_table, table_dist
from freq_util import fasta_names
from golden_util import Fixture
from tree_util import parse_newick

pytestmark = pytest.mark.gpu

SEED = 0x5EED2026
KEYS = ("rep_dist", "rep_left", "rep_right", "support")


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    yield c
    c.close()


@pytest.fixture
def tune(ctx):
    """ctx.tune for the two bootstrap knobs, both back at 0 afterwards."""
    from pangenome_amd import _lib
    yield lambda what, v: ctx.tune({"scratch": _lib.PG_TUNE_BOOT_SCRATCH, "form": _lib.PG_TUNE_BOOT_FORM}[what], v)
    ctx.tune(_lib.PG_TUNE_BOOT_SCRATCH, 0)
    ctx.tune(_lib.PG_TUNE_BOOT_FORM, 0)


@functools.lru_cache(maxsize=None)
def case(kind, G, L, R):
    """(bits, dist, want): a table, its Hamming matrix and the specification's
    result over the specification's own tree of it."""
    from pangenome_amd import host
    if kind == "coin":
        bits = coin_table(L, G, seed=5) if L else np.zeros((0, (G + 63) // 64), np.uint64)
    else:
        bits = {"clean": lambda: clean_table(G, 8), "mixed": mixed_table, "star": lambda: star_table(G, L)}[kind]()
    d = table_dist(bits, G)
    joins, _ = host.tree_nj(d)
    return bits, d, host.tree_bootstrap(bits, G, joins, R, SEED, dist=d, rep_dist=True)


def device(ctx, bits, G, R, seed=SEED):
    rd = ctx.tree_bootstrap(R, seed, bits=bits, n_groups=G, rep_dist=True)
    left, right = ctx.tree_bootstrap_joins()
    sup, reps = ctx.tree_support()
    assert reps == R
    return {"rep_dist": rd, "rep_left": left, "rep_right": right, "support": sup}


def same(got, want):
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def check(ctx, kind, G, L, R):
    bits, d, want = case(kind, G, L, R)
    assert ctx.tree_nj(d, G) == max(G - 3, 0)
    got = device(ctx, bits, G, R)
    same(got, want)
    return got


# ------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("L", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("G", [4, 5, 63, 64, 65, 129])
def test_sizes(ctx, G, L):
    """63, 64 and 65 genomes straddle the presence word, the wave and the
    64 x 64 tile (65 and 129: W = 2 and 3, more than one tile); 63, 64 and 65
    labels the transposed word; 1000 labels is more than one 16-word tile of
    the transpose.  129 leaves is past the LDS form, and 3 replicates are too
    few for the global form to be the default."""
    check(ctx, "coin", G, L, 3)
    assert ctx.tree_bootstrap_form() == (1 if G <= 128 else 3, 1)


def test_no_labels(ctx):
    got = check(ctx, "coin", 5, 0, 3)
    assert not got["rep_dist"].any() and got["support"].tolist() == [3, 3]


@pytest.mark.parametrize("G", [1, 2, 3])
def test_no_joins(ctx, G):
    got = check(ctx, "coin", G, 10, 3)
    assert got["support"].shape == (0,) and got["rep_left"].shape == (3, 0)
    assert ctx.tree_bootstrap_form()[0] == 0


# ------------------------------------------------------------ 2. forms
@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("G", [5, 65, 129])
def test_forms(ctx, tune, G, form):
    """Every form at every size gives the same bytes; 129 leaves are above
    the LDS form's 128, so form 1 there runs what the default runs."""
    tune("form", form)
    check(ctx, "coin", G, 1000, 3)
    by_size = 1 if G <= 128 else 3
    assert ctx.tree_bootstrap_form()[0] == {0: by_size, 1: by_size, 2: 2, 3: 3}[form]
    ms_dist, ms_nj, ms_support, cells = ctx.tree_bootstrap_time()
    assert min(ms_dist, ms_nj, ms_support) >= 0 and cells == 3 * sum(m * m for m in range(4, G + 1))


def test_default_form_above_the_lds_limit(ctx):
    """129 leaves: per-join launches for 3 replicates (test_sizes), one
    workgroup per replicate over global scratch from 4 on."""
    check(ctx, "coin", 129, 1000, 4)
    assert ctx.tree_bootstrap_form() == (2, 1)


# ------------------------------------------------------------ 3. batches
def per_replicate(G, L):
    """A replicate's scratch bytes as pg_boot.hip counts them."""
    NW = ((L + 63) // 64 + 1) & ~1
    J, W = max(G - 3, 0), (G + 63) // 64
    return 8 * G * NW + 8 * G * G + 8 * J * W + 8 * J + 13 * G + 64


@pytest.mark.parametrize("form", [0, 3])
def test_batches(ctx, tune, form):
    G, L, R = 65, 1000, 5
    tune("form", form)
    check(ctx, "coin", G, L, R)
    assert ctx.tree_bootstrap_form()[1] == 1
    tune("scratch", 1)                                       # one replicate per batch
    check(ctx, "coin", G, L, R)
    assert ctx.tree_bootstrap_form()[1] == 5
    tune("scratch", 2 * per_replicate(G, L) + 100)           # 2, 2 and a ragged last one
    check(ctx, "coin", G, L, R)
    assert ctx.tree_bootstrap_form()[1] == 3


# ------------------------------------------------------------ 4. ties
@pytest.mark.parametrize("form", [0, 2, 3])
def test_ties_take_the_smallest_live_pair(ctx, tune, form):
    """Rows in every genome or in none: every d_b is equal, so every join of
    every replicate takes the two smallest live slots."""
    tune("form", form)
    got = check(ctx, "star", 70, 100, 4)
    want = [(0 if t == 0 else 70 + t - 1, t + 1) for t in range(67)]
    for b in range(4):
        assert list(zip(got["rep_left"][b].tolist(), got["rep_right"][b].tolist())) == want
    assert got["support"].tolist() == [4] * 67


# ------------------------------------------------------------ 5. support at both ends and between
def test_clean_table_is_fully_supported(ctx):
    got = check(ctx, "clean", 70, 0, 8)
    assert got["support"].tolist() == [8] * 67


def test_mixed_table_spreads(ctx):
    got = check(ctx, "mixed", 20, 0, 16)
    assert int(got["support"].min()) < 16 and int(got["support"].max()) > 0


# ------------------------------------------------------------ 6. the guard and the device table
def test_guard(ctx):
    from pangenome_amd._lib import ptr
    a, _, want = case("coin", 20, 300, 4)
    got = check(ctx, "coin", 20, 300, 4)
    b = coin_table(300, 20, seed=77)
    assert ctx.lib.pg_tree_bootstrap(ctx.h, ptr(b), 300, 20, 4, SEED, None, 0) == -22
    assert ctx.lib.pg_tree_bootstrap(ctx.h, ptr(a[:299].copy()), 299, 20, 4, SEED, None, 0) == -22
    assert np.array_equal(ctx.tree_support()[0], want["support"])
    assert np.array_equal(ctx.tree_bootstrap_joins()[0], got["rep_left"])


def test_device_table(ctx):
    """Rows -> pg_freq -> pg_freq_compare -> pg_tree_nj -> pg_tree_bootstrap
    (bits NULL): the specification over the exported bits."""
    from pangenome_amd import host
    G = 37
    rng = np.random.default_rng(11)
    n, n_records = 20_000, 90
    rec_group = rng.permutation(np.arange(n_records) % G).astype(np.int32)
    start, length = rng.integers(0, 10 ** 7, n), rng.integers(20, 2000, n)
    rows = np.stack([np.sort(rng.integers(0, n_records, n)), start, start + length, rng.choice([1, -1], n),
                     rng.integers(0, 600, n)], axis=1).astype(np.int64)
    ctx.freq(rec_group, G, rows=rows)
    ctx.freq_compare(None)
    assert ctx.tree_nj() == G - 3
    bits = ctx.freq_table()["bits"]
    d = ctx.tree_dist()
    assert np.array_equal(d, table_dist(bits, G))
    rd = ctx.tree_bootstrap(6, SEED, rep_dist=True)
    want = host.tree_bootstrap(bits, G, ctx.tree_joins(), 6, SEED, dist=d, rep_dist=True)
    left, right = ctx.tree_bootstrap_joins()
    same({"rep_dist": rd, "rep_left": left, "rep_right": right, "support": ctx.tree_support()[0]}, want)
    # with another n_groups than the table's: refused (the tree has 5 leaves, the table 37 genomes)
    d5 = table_dist(coin_table(50, 5), 5)
    ctx.tree_nj(d5, 5)
    assert ctx.lib.pg_tree_bootstrap(ctx.h, None, 0, 5, 3, SEED, None, 0) == -22


# ------------------------------------------------------------ 7. refusals
def test_refusals_keep_the_previous_result(ctx):
    from pangenome_amd._lib import Context, ptr
    lib = ctx.lib
    bits, d, want = case("coin", 9, 65, 3)
    got = check(ctx, "coin", 9, 65, 3)

    def kept():
        left, right = ctx.tree_bootstrap_joins()
        sup, reps = ctx.tree_support()
        assert reps == 3
        same({"rep_dist": got["rep_dist"], "rep_left": left, "rep_right": right, "support": sup}, want)
    assert lib.pg_tree_bootstrap(None, ptr(bits), 65, 9, 3, SEED, None, 0) == -22
    assert lib.pg_tree_bootstrap(ctx.h, ptr(bits), 65, 8, 3, SEED, None, 0) == -22      # not the tree's n
    for R in (0, 4097):
        assert lib.pg_tree_bootstrap(ctx.h, ptr(bits), 65, 9, R, SEED, None, 0) == -22
    bad = bits.copy()
    bad[64, 0] |= np.uint64(1 << 9)
    assert lib.pg_tree_bootstrap(ctx.h, ptr(bad), 65, 9, 3, SEED, None, 0) == -22       # a bit at genome 9
    rd = np.zeros(3 * 81, np.uint64)
    assert lib.pg_tree_bootstrap(ctx.h, ptr(bits), 65, 9, 3, SEED, ptr(rd), 3 * 81 - 1) == -34
    kept()
    fresh = Context(27, 0)
    try:
        assert lib.pg_tree_bootstrap(fresh.h, ptr(bits), 65, 9, 3, SEED, None, 0) == -22   # no tree
        assert lib.pg_tree_support(fresh.h, None, 0, None) == -22
        assert lib.pg_tree_bootstrap_joins(fresh.h, None, None, 0) == -22
        assert lib.pg_tree_bootstrap_time(fresh.h, None, None, None, None) == -22
        assert lib.pg_tree_bootstrap_form(fresh.h, None, None) == -22
        fresh.tree_nj(d, 9)
        assert lib.pg_tree_bootstrap(fresh.h, None, 0, 9, 3, SEED, None, 0) == -22         # no pg_freq
    finally:
        fresh.close()
    # short caps on the exports (9 leaves: 6 joins, 3 x 6 replicate joins)
    u = np.zeros(18, np.uint32)
    assert lib.pg_tree_support(ctx.h, ptr(u), 5, None) == -34 and lib.pg_tree_support(ctx.h, ptr(u), 6, None) == 0
    assert u[:6].tolist() == want["support"].tolist()
    assert lib.pg_tree_bootstrap_joins(ctx.h, ptr(u), None, 17) == -34
    assert lib.pg_tree_bootstrap_joins(ctx.h, ptr(u), None, 18) == 0
    assert u.tolist() == want["rep_left"].reshape(-1).tolist()
    for what, v in ((33, -1), (34, -1), (34, 4)):
        assert lib.pg_tune(ctx.h, what, C.c_int64(v)) == -22
    kept()
    # a later pg_tree_nj drops the support: it described the old tree
    ctx.tree_nj(d, 9)
    assert lib.pg_tree_support(ctx.h, None, 0, None) == -22
    assert lib.pg_tree_bootstrap_joins(ctx.h, None, None, 0) == -22
    assert lib.pg_tree_bootstrap_time(ctx.h, None, None, None, None) == -22


# ------------------------------------------------------------ 8. determinism
@pytest.mark.parametrize("G", [65, 129])
def test_determinism(ctx, G):
    """The same input twice on one context, and once with every new device
    buffer filled with 0xA5: equal results (nothing read that no kernel wrote)."""
    from pangenome_amd import _lib
    bits, d, want = case("coin", G, 1000, 3)
    ctx.tree_nj(d, G)
    a = device(ctx, bits, G, 3)
    b = device(ctx, bits, G, 3)
    ctx.tune(_lib.PG_TUNE_POISON, 0xA5)
    try:
        c = device(ctx, bits, G, 3)
    finally:
        ctx.tune(_lib.PG_TUNE_POISON, -1)
    for got in (a, b, c):
        same(got, want)
    other = device(ctx, bits, G, 3, seed=SEED + 1)           # (and the seed matters)
    assert not np.array_equal(other["rep_dist"], want["rep_dist"])


# ------------------------------------------------------------ 9. the CLI
BOOT_FILES = ["_fr_tree_boot.npz", "_fr_tree_support.nwk", "_fr_tree_support.tsv"]


def _run(d, fasta, extra):
    from pangenome_amd import kmer
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    kmer.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4", "-g", "record"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def _files(prefix):
    d, base = os.path.split(prefix)
    return sorted(f[len(base):] for f in os.listdir(d) if f.startswith(base) and f != base)


def _support_tsv(path, G, R):
    lines = open(path).read().split("\n")
    assert lines[0] == "#node\tsupport\treplicates\tleaves" and lines[-1] == ""
    rows = [[int(v) for v in ln.split("\t")] for ln in lines[1:-1]]
    assert [r[0] for r in rows] == list(range(G, G + len(rows))) and all(r[2] == R for r in rows)
    return [r[1] for r in rows], [r[3] for r in rows]


def _same_tree(plain, labelled):
    from boot_util import parse_newick_labels
    e0, l0 = parse_newick(plain)
    e1, l1, labels = parse_newick_labels(labelled)
    assert e1 == e0 and l1 == l0 and 0 not in labels
    return labels


def test_cli(tmp_path):
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    q0, plain = _run(tmp_path / "plain", fx.fasta, ["-T", "1"])
    q, lines = _run(tmp_path / "boot", fx.fasta, ["-T", "1", "-B", "16"])
    assert lines == plain                                    # stdout is that of a run without -B
    assert sorted(set(_files(q)) - set(_files(q0))) == BOOT_FILES and set(_files(q0)) <= set(_files(q))
    for f in _files(q0):
        if f.endswith(".npz"):
            a, b = np.load(q0 + f), np.load(q + f)
            assert a.files == b.files and all(np.array_equal(a[k], b[k]) for k in a.files), f
        else:
            assert open(q0 + f, "rb").read() == open(q + f, "rb").read(), f
    assert not [f for f in os.listdir(os.path.dirname(q)) if f.endswith(".tmp")]
    # the support: the specification over the presence bits the run wrote
    z, tree = np.load(q + "_fr_presence.npz"), np.load(q + "_fr_tree.npz")
    joins = {k: tree[k] for k in ("left", "right", "left_len", "right_len")}
    want = host.tree_bootstrap(z["bits"], 8, joins, 16, SEED, dist=tree["dist"])
    sup, leaves = _support_tsv(q + "_fr_tree_support.tsv", 8, 16)
    assert sup == want["support"].tolist() and leaves == host.tree_clade_sizes(joins, 8)
    bz = np.load(q + "_fr_tree_boot.npz")
    assert sorted(bz.files) == ["genomes", "rep_left", "rep_right", "replicates", "seed", "support"]
    assert int(bz["replicates"]) == 16 and int(bz["seed"]) == SEED and bz["genomes"].tolist() == z["genomes"].tolist()
    assert np.array_equal(bz["support"], want["support"]) and bz["support"].dtype == np.uint32
    assert np.array_equal(bz["rep_left"], want["rep_left"]) and np.array_equal(bz["rep_right"], want["rep_right"])
    # the text: the plain tree's topology and lengths, every join labelled
    text = open(q + "_fr_tree_support.nwk", "rb").read()
    labels = _same_tree(open(q + "_fr_tree.nwk", "rb").read(), text)
    assert sorted(labels.values()) == sorted("%d" % (100 * s // 16) for s in sup)
    assert text == host.tree_newick(z["genomes"].tolist(), joins, (tree["root_child"], tree["root_len"]),
                                    support=(want["support"], 16))


def test_cli_variant_tree(tmp_path):
    from pangenome_amd import host
    from boot_util import pack_rows
    fx = Fixture("pan8_k27_c3")
    ids = [n.split()[0] for n in fasta_names(fx.fasta)]
    q, _ = _run(tmp_path / "var", fx.fasta, ["-b", "5", "-V", ids[0], "-A", "1", "-T", "1", "-B", "8"])
    assert set(BOOT_FILES + ["_fr_vartree_support.nwk", "_fr_vartree_support.tsv"]) <= set(_files(q))
    assert not [f for f in os.listdir(os.path.dirname(q)) if f.endswith(".tmp")]
    # the carrier columns of the primitive VCF, read as text, are the characters
    body = [ln.split(b"\t") for ln in open(q + "_fr_primitives.vcf", "rb").read().split(b"\n")
            if ln and not ln.startswith(b"##")]
    carry = np.array([[cell.split(b"/")[-1] == b"1" for cell in ln[9:]] for ln in body[1:]], np.uint8)
    bits = pack_rows(carry)
    d = table_dist(bits, 8)
    joins, root = host.tree_nj(d)
    want = host.tree_bootstrap(bits, 8, joins, 8, SEED, dist=d)
    sup, leaves = _support_tsv(q + "_fr_vartree_support.tsv", 8, 8)
    assert sup == want["support"].tolist() and leaves == host.tree_clade_sizes(joins, 8)
    text = open(q + "_fr_vartree_support.nwk", "rb").read()
    _same_tree(open(q + "_fr_vartree.nwk", "rb").read(), text)
    assert text == host.tree_newick([x.encode() for x in ids], joins, root, support=(want["support"], 8))


@pytest.mark.parametrize("extra", [["-B", "3"], ["-T", "1", "-B", "x"]])
def test_cli_refusals_print_the_manual(tmp_path, extra):
    out = io.StringIO()
    from pangenome_amd import kmer
    with pytest.raises(SystemExit):
        kmer.entry_point(["kmer_numba.py", "-i", str(tmp_path / "none.fsa"), "-k27", "-acc", "-g", "record"] + extra,
                         out=out)
    assert out.getvalue().startswith("Usage:")
    assert not os.listdir(tmp_path)
