"""The genome comparison on the device (pg_freq_compare,
pangenome_amd/csrc/pg_compare.hip).

Every case compares freq_shared() and freq_curves(), exactly, with an
independent reference (tests/compare_util.py: Python sets, or a float64
product and logical accumulates for the larger cases).  The shapes are the
smallest at which each mechanism can go wrong: the last word of the label
axis, 64 x 64 genome tiles full, partial and off the diagonal, several chunks
of the label axis, both forms of the curve pass on either side of the LDS
counters' limit, and the table where pg_freq left it on the device.
"""
import ctypes as C
import io
import os

import numpy as np
import pytest

from compare_util import (NEW_FILES, OLD_FILES, assert_compare_files, as_lists, check_identities, fr_files, pack,
                          random_bits, random_orders, reference_compare, reference_compare_fast)
from freq_util import fasta_names, golden
from golden_util import Fixture

pytestmark = pytest.mark.gpu

LDS_GROUPS = 2048                                        # CMP_LDS_GROUPS of pg_compare.hip


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    yield c
    c.close()


def device(ctx, bits, G, orders):
    ctx.freq_compare(orders, bits=bits, n_groups=G)
    return as_lists(ctx.freq_shared(), *ctx.freq_curves())


def check(ctx, bits, G, orders, fast=False):
    ref = (reference_compare_fast if fast else reference_compare)(bits, G, orders)
    got = device(ctx, bits, G, orders)
    assert got[0] == ref[0], "shared"
    assert got[1] == ref[1], "pan"
    assert got[2] == ref[2], "core"
    return got


def test_empties(ctx):
    got = device(ctx, np.zeros((0, 1), np.uint64), 3, random_orders(3, 2))
    assert got == ([[0] * 3] * 3, [[0] * 3] * 2, [[0] * 3] * 2)
    ctx.freq_compare(np.zeros((2, 0), np.int32), bits=np.zeros((0, 0), np.uint64), n_groups=0)
    assert ctx.freq_shared().shape == (0, 0) and [x.shape for x in ctx.freq_curves()] == [(2, 0), (2, 0)]
    assert check(ctx, pack([[1]]), 1, [[0]]) == ([[1]], [[1]], [[1]])
    assert check(ctx, pack([[0, 1, 0]]), 3, [[0, 1, 2]]) == ([[0, 0, 0], [0, 1, 0], [0, 0, 0]], [[0, 1, 1]], [[0, 0, 0]])
    # no order: the curve export succeeds and writes nothing
    got = check(ctx, random_bits(70, 3), 3, np.zeros((0, 3), np.int32))
    assert got[1] == got[2] == []
    from pangenome_amd._lib import ptr
    canary = np.full(4, 77, np.uint64)
    assert ctx.lib.pg_freq_curve(ctx.h, ptr(canary), ptr(canary), 0) == 0 and canary.tolist() == [77] * 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_label_axis_boundaries(ctx, n):
    """The last label is in every genome: an `and` that started as all ones
    in the last word would count the labels that do not exist as core."""
    G = 5
    bits = random_bits(n, G, seed=n, ones_row=False, zeros_row=False)
    bits[n - 1] = (1 << G) - 1
    orders = random_orders(G, 3, seed=n)
    got = check(ctx, bits, G, orders)
    check_identities(bits, G, orders, *got)
    assert 1 <= got[2][0][G - 1] <= n


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 129, 200])
def test_genome_axis_boundaries(ctx, G):
    """200: full and partial 64 x 64 tiles, off-diagonal tiles and their
    mirror.  Symmetry and the diagonal (check_identities) from the bits."""
    bits = random_bits(300, G, seed=G)
    orders = random_orders(G, 3, seed=G)
    got = check(ctx, bits, G, orders)
    check_identities(bits, G, orders, *got)


@pytest.fixture(scope="module")
def chunk_case():
    n, G = 64 * 37 + 5, 70
    bits, orders = random_bits(n, G, seed=4), random_orders(G, 3, seed=4)
    return bits, G, orders, reference_compare_fast(bits, G, orders)


@pytest.mark.parametrize("chunk", [1, 2, 0])
def test_chunking(ctx, chunk_case, chunk):
    """38 words of the label axis in chunks of 1 and 2 words (many blocks per
    tile, summed by the atomic flush) and in the default chunk."""
    from pangenome_amd import _lib
    bits, G, orders, ref = chunk_case
    ctx.tune(_lib.PG_TUNE_CMP_CHUNK, chunk)
    try:
        assert device(ctx, bits, G, orders) == ref
    finally:
        ctx.tune(_lib.PG_TUNE_CMP_CHUNK, 0)


@pytest.mark.parametrize("form", [0, 1])
def test_forms(ctx, chunk_case, form):
    from pangenome_amd import _lib
    bits, G, orders, ref = chunk_case
    ctx.tune(_lib.PG_TUNE_CMP_FORM, form)
    try:
        assert device(ctx, bits, G, orders) == ref
    finally:
        ctx.tune(_lib.PG_TUNE_CMP_FORM, 0)


def test_above_the_lds_counters(ctx):
    """One genome more than the per-block LDS counters hold: the curve pass
    takes the global form by itself."""
    G = LDS_GROUPS + 1
    bits = random_bits(200, G, seed=6)
    check(ctx, bits, G, random_orders(G, 2, seed=6), fast=True)


def test_random(ctx):
    G, n = 1100, 5000
    bits, orders = random_bits(n, G, seed=8), random_orders(G, 3, seed=8)
    got = check(ctx, bits, G, orders, fast=True)
    assert device(ctx, bits, G, orders) == got


# (test_gpu_freq.py's make_rows / random_case, copied)
def make_rows(rec, start, length, strand, label):
    rec = np.asarray(rec, np.int64)
    start = np.broadcast_to(np.asarray(start, np.int64), rec.shape)
    return np.stack([rec, start, start + np.broadcast_to(np.asarray(length, np.int64), rec.shape),
                     np.broadcast_to(np.asarray(strand, np.int64), rec.shape),
                     np.broadcast_to(np.asarray(label, np.int64), rec.shape)], axis=1).astype(np.int64)


def random_case(n_records, G, n=100_000, n_labels=3000, seed=11):
    rng = np.random.default_rng(seed)
    rec_group = rng.permutation(np.arange(n_records) % G).astype(np.int32)
    rows = make_rows(np.sort(rng.integers(0, n_records, n)), rng.integers(0, 10 ** 7, n), rng.integers(-500, 20000, n),
                     rng.choice([1, -1], n), rng.integers(0, n_labels, n))
    rows[rng.integers(0, n, 100), 4] = -1
    return rows, rec_group


def test_device_table(ctx):
    """bits=None takes the table where the last pg_freq left it: the same
    results as its exported bits uploaded again."""
    from pangenome_amd._lib import PangenomeError
    rows, rec_group = random_case(90, 37)
    ctx.freq(rec_group, 37, rows=rows)
    orders = random_orders(37, 3)
    ctx.freq_compare(orders)
    on_device = as_lists(ctx.freq_shared(), *ctx.freq_curves())
    bits = ctx.freq_table()["bits"]
    assert bits.shape == (3000, 1)
    assert check(ctx, bits, 37, orders, fast=True) == on_device
    # a new table: the comparison described the old one
    ctx.freq(rec_group, 37, rows=rows[:1000])
    with pytest.raises(PangenomeError, match=r"pg_freq_shared failed \(-22\)"):
        ctx.freq_shared()
    with pytest.raises(PangenomeError, match=r"pg_freq_curve failed \(-22\)"):
        ctx.freq_curves()


def test_argument_errors(ctx):
    """Each is refused before any launch (no device fault is involved) and
    leaves the previous result in place."""
    from pangenome_amd._lib import PG_TUNE_DEVICE_CAP, Context, ptr
    lib = ctx.lib
    bits, orders = random_bits(100, 5, seed=3), random_orders(5, 2, seed=3)
    kept = check(ctx, bits, 5, orders)
    o = np.ascontiguousarray(orders)
    assert lib.pg_freq_compare(None, ptr(bits), 100, 5, ptr(o), 2) == -22
    fresh = Context(27, 0)
    try:
        assert lib.pg_freq_compare(fresh.h, None, 0, 5, ptr(o), 2) == -22          # no pg_freq yet
        assert lib.pg_freq_shared(fresh.h, None, 0) == -22 and lib.pg_freq_curve(fresh.h, None, None, 0) == -22
    finally:
        fresh.close()
    assert lib.pg_freq_compare(ctx.h, ptr(bits), 100, 0, None, 0) == -22           # no genomes, but labels
    assert lib.pg_freq_compare(ctx.h, ptr(bits), 100, 5, None, 1) == -22           # orders NULL
    for bad in (o[1, 2], 5, -1):                                                   # a duplicate, G, a negative
        o2 = o.copy()
        o2[1, 3] = bad
        assert lib.pg_freq_compare(ctx.h, ptr(bits), 100, 5, ptr(o2), 2) == -22
    b2 = bits.copy()
    b2[57, 0] |= np.uint64(1 << 5)
    assert lib.pg_freq_compare(ctx.h, ptr(b2), 100, 5, ptr(o), 2) == -22           # a bit at position G
    assert lib.pg_freq_compare(ctx.h, ptr(bits), 0, 32769, None, 0) == -34
    s = np.empty((5, 5), np.uint64)
    pan = np.empty((2, 5), np.uint64)
    assert lib.pg_freq_shared(ctx.h, ptr(s), 24) == -34 and lib.pg_freq_curve(ctx.h, ptr(pan), None, 9) == -34
    assert lib.pg_freq_shared(ctx.h, ptr(s), 25) == 0 and lib.pg_freq_curve(ctx.h, ptr(pan), None, 10) == 0
    assert (s.tolist(), pan.tolist()) == kept[:2]
    assert as_lists(ctx.freq_shared(), *ctx.freq_curves()) == kept
    # bits == NULL with another n_groups than the table's
    rows, rec_group = random_case(9, 4, n=500, n_labels=20)
    ctx.freq(rec_group, 4, rows=rows)
    ctx.freq_compare(random_orders(4, 1))
    kept = as_lists(ctx.freq_shared(), *ctx.freq_curves())
    assert lib.pg_freq_compare(ctx.h, None, 0, 5, ptr(o), 2) == -22
    assert as_lists(ctx.freq_shared(), *ctx.freq_curves()) == kept
    # an allocation past the device cap: PG_ENOMEM from the first buffer, before any launch
    ctx.tune(PG_TUNE_DEVICE_CAP, int(lib.pg_device_bytes(0)) + 1)
    try:
        assert lib.pg_freq_compare(ctx.h, ptr(bits), 100, 5, ptr(o), 2) == -12
    finally:
        ctx.tune(PG_TUNE_DEVICE_CAP, 0)
    assert as_lists(ctx.freq_shared(), *ctx.freq_curves()) == kept
    for what, bad in ((22, -1), (22, 2 ** 25 + 1), (23, 2), (23, -1)):
        assert lib.pg_tune(ctx.h, what, C.c_int64(bad)) == -22


# ------------------------------------------------------------ whole pipeline
def _run(d, fasta, extra):
    from pangenome_amd import kmer
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    kmer.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4", "-g", "record"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def test_cli(tmp_path):
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    ids = [n.split()[0] for n in fasta_names(fx.fasta)]
    q0, plain = _run(tmp_path / "plain", fx.fasta, [])
    assert fr_files(q0) == OLD_FILES                     # without -p: nothing new
    q, lines = _run(tmp_path / "p5", fx.fasta, ["-p", "5"])
    assert lines == plain                                # stdout (but the stage timings) is unchanged
    for suffix in ["_rdbg_weight.xyz", "_rdbg_weight.xyz.mcl"] + [s for s in OLD_FILES if s.endswith(".tsv")]:
        assert open(q + suffix, "rb").read() == open(q0 + suffix, "rb").read(), suffix
    z, z0 = np.load(q + "_fr_presence.npz"), np.load(q0 + "_fr_presence.npz")     # (a zip: its members carry a time)
    assert sorted(z.files) == sorted(z0.files) and all(np.array_equal(z[k], z0[k]) for k in z0.files)
    assert fr_files(q) == sorted(OLD_FILES + NEW_FILES) and len(fr_files(q)) == 8
    bits = np.load(q + "_fr_presence.npz")["bits"]
    orders = host.compare_orders(8, 5)
    shared, pan, core = reference_compare(bits, 8, orders)
    assert_compare_files(q, ids, shared, orders, pan, core)
    want = golden("pan8_k27_c3_w4")
    assert [p[7] for p in pan] == [909] * 5 and [c[7] for c in core] == [want["spectrum_labels"][8]] * 5
