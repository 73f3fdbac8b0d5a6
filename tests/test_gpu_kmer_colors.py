"""The k-mer colours on the device (pg_kmer_colors and its exports, pg_kmer_compare,
-K) against the oracle: genome g's key set is the oracle's dBG of that genome's
records alone (colors_util.yardstick, computed once per input; the precondition
is checked in test_kmer_colors_host.py).  Everything is compared exactly, and
n_missing == 0 and n_uncoloured == 0 unless a case says otherwise."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from colors_util import (CASES, fasta, no_sentinel, oracle_keys, pieces, rec_group_of, split_records, letters,
                         window_keys, yardstick)

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ctx_of():
    from pangenome_amd._lib import Context
    made = {}

    def get(k):
        if k not in made:
            made[k] = Context(k, 0)
        return made[k]
    yield get
    for c in made.values():
        c.close()


def build(ctx, fa: bytes, rc0: bool, flags=None):
    n_records, _ = ctx.parse_host(np.frombuffer(fa, np.uint8))
    ctx.build_dbg(flags, 0, rc0)
    return n_records


def table_keys(ctx):
    return no_sentinel(ctx.dbg()[0])


def spectrum_lists(t):
    return {k: np.asarray(t[k]).tolist() for k in ("kmers_by_g", "g_kmers", "g_core", "g_shell", "g_unique")}


def check(ctx, sets, G, keys_of_table, counts, missing=0):
    """The device's colours against host.kmer_colors over the yardstick's sets."""
    from pangenome_amd import host
    want = host.kmer_colors([no_sentinel(s) for s in sets], G, keys=keys_of_table)
    n_keys, n_windows, n_missing, n_uncoloured = counts
    keys, bits = ctx.kmer_colors_export()
    assert np.array_equal(keys, keys_of_table) and n_keys == keys.shape[0]
    assert bits.shape == want["bits"].shape and np.array_equal(bits, want["bits"])
    for g in range(G):                                       # read the other way round: genome g's keys
        assert np.array_equal(keys[(bits[:, g >> 6] >> np.uint64(g & 63)) & np.uint64(1) == 1], no_sentinel(sets[g]))
    if G & 63 and bits.shape[0]:
        assert not (bits[:, -1] >> np.uint64(G & 63)).any()  # no bit at or above G
    got = ctx.kmer_colors_spectrum()
    assert spectrum_lists(got) == spectrum_lists(want)
    assert n_missing == missing and n_uncoloured == int(want["kmers_by_g"][0]) and n_windows > 0
    shared, pan, core = ctx.kmer_compare(None)
    assert np.array_equal(shared, want["shared"]) and pan.shape == core.shape == (0, G)
    return want, keys, bits


# ------------------------------------------------------------ 1 - 5. against the oracle
PLAIN = [x for x in CASES if x[0] != "excl"]


@pytest.mark.parametrize("name,k,c", PLAIN, ids=["%s-k%d-c%d" % x for x in PLAIN])
def test_colours_equal_the_oracle(ctx_of, name, k, c):
    ctx = ctx_of(k)
    rc0 = (c >> 1) == 1
    sets, whole = yardstick(name, k, c)
    G = len(sets)
    R = build(ctx, fasta(name), rc0)
    keys_of_table = table_keys(ctx)
    assert np.array_equal(keys_of_table, no_sentinel(whole))
    counts = ctx.kmer_colors(rec_group_of(name, R), G, None, rc0)
    want, _, _ = check(ctx, sets, G, keys_of_table, counts)
    assert counts[3] == 0 and int(want["kmers_by_g"][0]) == 0
    # all-ones flags are NULL flags; the windows: every strand's, but an n < k record's one
    assert ctx.kmer_colors(rec_group_of(name, R), G, np.ones(R, np.uint8), rc0) == counts
    lens = ctx.records()["seq_len"]
    assert counts[1] == int(np.maximum(lens[lens >= k] - k + 1, 1).sum()) * (2 if rc0 else 1)
    ctx.kmer_colors_drop()


# ------------------------------------------------------------ 6. exclusions
def test_records_without_genome_or_flag(ctx_of):
    """Record 1 has no genome, record 4 no flag, the table holds all six: the
    keys only those two have stay uncoloured."""
    k, c, name = 11, 2, "excl"
    ctx = ctx_of(k)
    recs = [r if r.endswith(b"\n") else r + b"\n" for p in pieces(name) for r in split_records(p)]
    assert len(recs) == 6
    R = build(ctx, fasta(name), True)
    assert R == 6
    keys_of_table = table_keys(ctx)
    grp = np.array([0, -1, 1, 1, 2, 2], np.int32)
    flags = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    sets = [oracle_keys(recs[0], k, c), oracle_keys(recs[2] + recs[3], k, c), oracle_keys(recs[5], k, c)]
    only_theirs = np.setdiff1d(keys_of_table, np.unique(np.concatenate(sets)))
    assert only_theirs.shape[0] > 0
    counts = ctx.kmer_colors(grp, 3, flags, True)
    want, _, _ = check(ctx, sets, 3, keys_of_table, counts)
    assert counts[3] == only_theirs.shape[0] == int(ctx.kmer_colors_spectrum()["kmers_by_g"][0])
    ctx.kmer_colors_drop()


def test_windows_the_table_lacks(ctx_of):
    """The table built without record 1, every record walked: its windows whose
    key no other record has are missing, and colour nothing."""
    k, c, name = 11, 2, "excl"
    ctx = ctx_of(k)
    recs = [r if r.endswith(b"\n") else r + b"\n" for p in pieces(name) for r in split_records(p)]
    built = np.array([1, 0, 1, 1, 1, 1], np.uint8)
    R = build(ctx, fasta(name), True, built)
    keys_of_table = table_keys(ctx)
    others = oracle_keys(b"".join(r for i, r in enumerate(recs) if i != 1), k, c)
    assert np.array_equal(keys_of_table, others)
    have = set(int(x) for x in others)
    missing = sum(1 for x in window_keys(letters(recs[1]), k, True) if x not in have)
    assert missing > 0
    counts = ctx.kmer_colors(rec_group_of(name, R), 3, None, True)
    sets = [np.intersect1d(s, others) for s in yardstick(name, k, c)[0]]
    check(ctx, sets, 3, keys_of_table, counts, missing=missing)
    assert counts[2] == missing and counts[3] == 0
    ctx.kmer_colors_drop()


# ------------------------------------------------------------ 7. the comparison
@pytest.mark.parametrize("name,k", [("pan8", 27), ("word65", 11)])
def test_compare(ctx_of, name, k):
    from pangenome_amd import host
    ctx = ctx_of(k)
    R = build(ctx, fasta(name), True)
    G = len(pieces(name))
    ctx.kmer_colors(rec_group_of(name, R), G, None, True)
    _, bits = ctx.kmer_colors_export()
    orders = host.compare_orders(G, 3)
    shared, pan, core = ctx.kmer_compare(orders)
    hs, hp, hc = host.freq_compare(bits, G, orders)
    assert np.array_equal(shared, hs) and np.array_equal(pan, hp) and np.array_equal(core, hc)
    # pg_freq_compare fed the exported bits as host rows
    ctx.freq_compare(orders, bits=bits, n_groups=G)
    fp, fc = ctx.freq_curves()
    assert np.array_equal(ctx.freq_shared(), shared) and np.array_equal(fp, pan) and np.array_equal(fc, core)
    # the two results are each their own: after pg_freq, pg_freq_compare and pg_kmer_compare the
    # frequency table's comparison is still the frequency table's
    rows = np.array([[0, 0, 10, 1, 0], [1, 0, 10, 1, 0], [1, 5, 20, -1, 1], [2, 0, 7, 1, 1]], np.int64)
    grp = np.minimum(np.arange(R, dtype=np.int32), G - 1)
    ctx.freq(grp, G, rows=rows)
    ctx.freq_compare(orders[:2])
    mine = (ctx.freq_shared(), *ctx.freq_curves())
    assert int(mine[0].sum()) == 8 and not np.array_equal(mine[0], shared)
    again = ctx.kmer_compare(orders)
    assert all(np.array_equal(a, b) for a, b in zip(again, (shared, pan, core)))
    after = (ctx.freq_shared(), *ctx.freq_curves())
    assert all(np.array_equal(a, b) for a, b in zip(mine, after)) and after[1].shape == (2, G)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.kmer_compare_export(), (shared, pan, core)))
    ms_index, ms_colour, ms_compare, n_windows = ctx.kmer_colors_time()
    assert ms_index > 0 and ms_colour > 0 and ms_compare > 0 and n_windows > 0
    ctx.kmer_colors_drop()


# ------------------------------------------------------------ 8. lifetime and refusals
def exports(ctx):
    return [ctx.kmer_colors_export, ctx.kmer_colors_spectrum, ctx.kmer_compare_export, ctx.kmer_colors_time,
            lambda: ctx.kmer_compare(None)]


def assert_no_colours(ctx):
    from pangenome_amd._lib import PangenomeError
    for f in exports(ctx):
        with pytest.raises(PangenomeError, match="\\(-22\\)"):
            f()


def test_lifetime():
    from pangenome_amd._lib import Context, PangenomeError
    name, k = "smallk", 3
    ctx = Context(k, 0)
    try:
        ctx.kc_groups_n = 6
        assert_no_colours(ctx)                                   # before any pg_kmer_colors
        with pytest.raises(PangenomeError, match="\\(-22\\)"):   # no parse
            ctx.kmer_colors(np.zeros(6, np.int32), 6)
        ctx.parse_host(np.frombuffer(fasta(name), np.uint8))
        with pytest.raises(PangenomeError, match="\\(-22\\)"):   # a parse, no table
            ctx.kmer_colors(np.zeros(6, np.int32), 6)
        R = build(ctx, fasta(name), True)
        grp = rec_group_of(name, R)
        ctx.kmer_colors(grp, 6)
        with pytest.raises(PangenomeError, match="\\(-22\\)"):   # colours, no comparison yet
            ctx.kmer_compare_export()
        ctx.kmer_compare(None)
        ctx.kmer_colors_drop()
        assert_no_colours(ctx)                                   # after pg_kmer_colors_drop
        ctx.kmer_colors_drop()                                   # (dropping nothing is no error)
        ctx.kmer_colors(grp, 6)
        ctx.kmer_compare(None)
        ctx.build_dbg(None, 0, True)
        assert_no_colours(ctx)                                   # after a rebuild
        ctx.kmer_colors(grp, 6)
        ctx.parse_host(np.frombuffer(fasta(name), np.uint8))
        assert_no_colours(ctx)                                   # after a parse
    finally:
        ctx.close()


def test_refusals_keep_the_previous_result(ctx_of):
    from pangenome_amd import _lib
    name, k = "smallk", 3
    ctx = ctx_of(k)
    R = build(ctx, fasta(name), True)
    grp = rec_group_of(name, R)
    counts = ctx.kmer_colors(grp, 6)
    keys, bits = ctx.kmer_colors_export()
    spec = spectrum_lists(ctx.kmer_colors_spectrum())
    cmp0 = ctx.kmer_compare(None)
    lib = ctx.lib
    n = [C.c_uint64() for _ in range(4)]
    refs = [C.byref(x) for x in n]

    def call(h, g, f, nrec, G):
        return lib.pg_kmer_colors(h, _lib.ptr(g), _lib.ptr(f), nrec, G, 1, *refs)
    bad_lo, bad_hi = grp.copy(), grp.copy()
    bad_lo[0], bad_hi[-1] = -2, 6
    assert call(None, grp, None, R, 6) == -22                   # a NULL context
    assert call(ctx.h, None, None, R, 6) == -22                 # rec_group == NULL
    assert call(ctx.h, bad_lo, None, R, 6) == -22               # an entry outside [-1, G)
    assert call(ctx.h, bad_hi, None, R, 6) == -22
    assert call(ctx.h, grp, None, R + 1, 6) == -22              # another record count
    assert call(ctx.h, grp, None, R - 1, 6) == -22
    assert call(ctx.h, np.full(R, -1, np.int32), None, R, 0) == -22     # G == 0 with records
    assert call(ctx.h, grp, None, R, 32769) == -34              # as the comparison
    assert lib.pg_kmer_compare(ctx.h, None, 1) == -22           # orders == NULL with n_orders > 0
    assert lib.pg_kmer_compare(ctx.h, _lib.ptr(np.array([0, 1, 2, 3, 4, 4], np.int32)), 1) == -22
    assert lib.pg_kmer_colors_export(ctx.h, _lib.ptr(np.zeros(1, np.uint64)), None, keys.shape[0] - 1, None) == -34
    assert lib.pg_kmer_compare_export(ctx.h, _lib.ptr(np.zeros(1, np.uint64)), 35, None, None, 0) == -34
    # an allocation failure: the device cap just above what the process holds
    ctx.tune(_lib.PG_TUNE_DEVICE_CAP, lib.pg_device_bytes(0) + 64)
    try:
        assert call(ctx.h, grp, None, R, 6) == -12
    finally:
        ctx.tune(_lib.PG_TUNE_DEVICE_CAP, 0)
    k2, b2 = ctx.kmer_colors_export()
    assert np.array_equal(k2, keys) and np.array_equal(b2, bits) and spectrum_lists(ctx.kmer_colors_spectrum()) == spec
    assert all(np.array_equal(a, b) for a, b in zip(ctx.kmer_compare_export(), cmp0))
    assert ctx.kmer_colors(grp, 6) == counts                    # and the call still works
    ctx.kmer_colors_drop()


# ------------------------------------------------------------ 9. the CLI
KM_FILES = sorted("_km_" + s for s in ("spectrum.tsv", "genomes.tsv", "shared.tsv", "jaccard.tsv", "compare.npz",
                                       "curve.tsv", "dist.tsv", "tree.nwk", "tree.tsv", "tree.npz"))


def _run(d, fa, extra):
    from pangenome_amd import kmer
    os.makedirs(str(d), exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fa)
    out = io.StringIO()
    kmer.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-a", "cc", "-w", "4", "-g", "record", "-p", "3",
                      "-T", "1"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def _same_file(a, b):
    if a.endswith(".npz"):
        za, zb = np.load(a), np.load(b)
        return sorted(za.files) == sorted(zb.files) and all(np.array_equal(za[k], zb[k]) for k in za.files)
    return open(a, "rb").read() == open(b, "rb").read()


def test_cli(tmp_path):
    from pangenome_amd import host
    name, k, c = "pan8", 27, 3
    fa = fasta(name)
    q, lines = _run(tmp_path / "km", fa, ["-K", "1"])
    q0, plain = _run(tmp_path / "plain", fa, [])
    assert lines == plain                                        # stdout is that of a run without -K
    d, d0 = os.path.dirname(q), os.path.dirname(q0)
    files, files0 = sorted(os.listdir(d)), sorted(os.listdir(d0))
    assert not [f for f in files + files0 if f.endswith(".tmp")] and not [f for f in files0 if "_km_" in f]
    assert sorted(f[len("pan8.fsa"):] for f in set(files) - set(files0)) == KM_FILES
    for f in files0:                                             # every other file is the same
        assert _same_file(os.path.join(d, f), os.path.join(d0, f)), f
    # the files the writers make from the specification over the oracle's key sets
    sets = [no_sentinel(oracle_keys(p, k, c)) for p in pieces(name)]
    G = len(sets)
    want = host.kmer_colors(sets, G)
    names = [split_records(p)[0].split(b"\n")[0][1:].split()[0] for p in pieces(name)]
    w = str(tmp_path / "want")
    os.makedirs(w)
    wq = os.path.join(w, "pan8.fsa")
    orders = host.compare_orders(G, 3)
    shared, pan, core = host.freq_compare(want["bits"], G, orders)
    host.write_kmer_files(wq, want, names)
    host.write_compare_files(wq, names, shared, orders, pan, core, tag="_km_")
    dist = host.kmer_distance(shared)
    host.write_tree_files(wq, names, dist, *host.tree_nj(dist), tag="_km_")
    assert sorted(f[len("pan8.fsa"):] for f in os.listdir(w)) == KM_FILES
    for f in KM_FILES:
        assert _same_file(q + f, wq + f), f
