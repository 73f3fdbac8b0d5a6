"""The region graph on the device (pg_region_graph, pangenome_amd/csrc/pg_region.hip).

Every case compares, exactly, the four returned counts, region_nodes(),
region_links(), region_paths(), region_links_text() and region_gfa_text()
with an independent list-based reference (tests/region_util.py).  The
synthetic shapes are the smallest at which each mechanism can go wrong: runs
that cross a row tile (256 rows) and a wave, more tiles than blocks, one hot
label that is an end of most links, a label per row, genomes that are not
monotonic in the rows, a self link, label gaps, and the dense range.
"""
import ctypes as C
import io
import os
import threading

import numpy as np
import pytest

from freq_util import fasta_names, rows5_of, rows_of
from golden_util import Fixture
from region_util import (GFA_HEADER, LINKS_HEADER, assert_files, assert_same, check_device, device_tables, golden,
                         reference_gfa, reference_links_text, reference_region, summary)

pytestmark = pytest.mark.gpu

TILE = 256                                               # RG_BLOCK: rows per tile of the row passes


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def km():
    from pangenome_amd import kmer
    return kmer


def make_rows(rec, start, length, strand, label):
    rec = np.asarray(rec, np.int64)
    start = np.broadcast_to(np.asarray(start, np.int64), rec.shape)
    return np.stack([rec, start, start + np.broadcast_to(np.asarray(length, np.int64), rec.shape),
                     np.broadcast_to(np.asarray(strand, np.int64), rec.shape),
                     np.broadcast_to(np.asarray(label, np.int64), rec.shape)], axis=1).astype(np.int64)


def names_for(n):
    return [b"rec%d len=%d" % (i, i) for i in range(n)]


# ------------------------------------------------------------ 1. empty and tiny
def test_empty(ctx):
    for grp, G in ((np.zeros(0, np.int32), 0), (np.array([0, 1, 0], np.int32), 2)):
        ref, text, gfa = check_device(ctx, np.zeros((0, 5), np.int64), grp, G, names_for(len(grp)))
        assert text == LINKS_HEADER.encode() and gfa == GFA_HEADER.encode()
        assert ctx.region_gfa_text([]) == gfa            # no path: no name is needed


def test_one_row(ctx):
    ref, text, gfa = check_device(ctx, [[1, 40, 13, -1, 0]], [-1, 0], 1, names_for(2))
    assert text == LINKS_HEADER.encode()
    assert gfa == b"H\tVN:Z:1.0\nS\t0\t*\tLN:i:27\nP\trec1 len=1:40-13:-\t0+\t*\n"
    assert ctx.region_paths()["path_steps"].tolist() == [1]


def test_two_rows(ctx):
    first = [0, 10, 30, 1, 4]
    ref, text, gfa = check_device(ctx, [first, [0, 50, 90, 1, 7]], [0, 0], 1, names_for(2))
    assert text == b"#from\tto\tcount\tgenomes\n4\t7\t1\t1\n" and ref["path_steps"] == [2]
    assert gfa.endswith(b"L\t4\t+\t7\t+\t0M\tRC:i:1\tgn:i:1\nP\trec0 len=0:10-90:+\t4+,7+\t*\n")
    for second in ([1, 50, 90, 1, 7], [0, 90, 50, -1, 7]):           # another record; the other strand
        ref, text, gfa = check_device(ctx, [first, second], [0, 0], 1, names_for(2))
        assert text == LINKS_HEADER.encode() and ref["path_steps"] == [1, 1]
    for mid, grp in (([0, 35, 40, 1, -1], [0, 0]), ([1, 35, 40, 1, 6], [0, -1])):     # an unused row between them
        ref, text, gfa = check_device(ctx, [first, mid, [0, 50, 90, 1, 7]], grp, 1, names_for(2))
        assert text == LINKS_HEADER.encode() and ref["path_steps"] == [1, 1] and ref["n_skipped"] == 1


# ------------------------------------------------------------ 2. halo
def one_run(n, mod):
    i = np.arange(n)
    return make_rows(np.ones(n, np.int64), i * 11, 1 + i % 13, -1, i % mod)


@pytest.mark.parametrize("n", [2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 1023,
                               1024, 1025, 4097])
def test_halo(ctx, n):
    """One run of n rows: every adjacent pair is a link, whichever wave, tile
    or block its two rows fall into; then the same rows cut into two records."""
    for mod in (7, 2):
        rows = one_run(n, mod)
        ref, _, _ = check_device(ctx, rows, [0, 2, 1], 3, names_for(3))
        assert sum(ref["link_count"]) == n - 1 and ref["path_steps"] == [n] and set(ref["link_genomes"]) <= {1}
    rows = one_run(n, 7)
    for cut in (63, 64, 65, TILE, TILE + 1):
        if cut >= n:
            continue
        two = rows.copy()
        two[cut:, 0] = 2
        ref, _, _ = check_device(ctx, two, [0, 2, 1], 3, names_for(3))
        assert sum(ref["link_count"]) == n - 2 and ref["path_steps"] == [cut, n - cut]
        # no link crosses the cut: the pair of labels there occurs one time less than in the one run
        whole = reference_region(rows, [0, 2, 1], 3)
        pair = ((cut - 1) % 7, cut % 7)
        count = lambda r: dict(zip(zip(r["link_from"], r["link_to"]), r["link_count"])).get(pair, 0)
        assert count(ref) == count(whole) - 1


def test_more_tiles_than_blocks(ctx):
    """More row tiles than the row passes have blocks (8 per CU: a block takes
    a second tile), and more links than the degree pass has threads: one run
    through all of it, with a link per row."""
    n = 8 * 256 * TILE + TILE + 1
    i = np.arange(n, dtype=np.int64)
    rows = make_rows(np.zeros(n, np.int64), i, 1 + i % 5, 1, (i * 7919) % 300007)
    ref, _, _ = check_device(ctx, rows, [0], 1, [b"one"])
    assert sum(ref["link_count"]) == n - 1 and len(ref["link_from"]) > 1024 * 256


# ------------------------------------------------------------ 3. hot link and long path
def hot_rows(rec):
    n = rec.shape[0]
    rng = np.random.default_rng(3)
    # A b A c A d ...: A = 3, the small ones 50 six-digit labels (a step of theirs is 8 bytes of a P line)
    lab = np.where(np.arange(n) % 2 == 0, 3, 100_000 + 1009 * rng.integers(0, 50, n))
    return make_rows(rec, rng.integers(0, 1000, n), 2 ** 31 - rng.integers(0, 5000, n), 1, lab)


@pytest.mark.parametrize("one_record", [False, True])
def test_hot_link_and_long_path(ctx, one_record):
    """Label 3 holds every other row and is an end of every link; with one
    record the single path's P line is longer than 1 MB.  Twice: the same bytes."""
    n = 200_001
    rec = np.zeros(n, np.int64) if one_record else np.sort(np.random.default_rng(4).integers(0, 130, n))
    rows = hot_rows(rec)
    rec_group = (np.arange(130) % 65).astype(np.int32)
    ref, text, gfa = check_device(ctx, rows, rec_group, 65, names_for(130))
    assert ref["rows"][ref["labels"].index(3)] == n // 2 + 1 and max(ref["max_len"]) > 2 ** 31 - 5000
    assert all(3 in (a, b) for a, b in zip(ref["link_from"], ref["link_to"]))
    if one_record:
        assert ref["path_steps"] == [n] and len(gfa.split(b"\n")[-2]) > 1 << 20
    else:
        assert len(ref["path_steps"]) == 130 and max(ref["link_genomes"]) == 65
    ctx.region_graph(rec_group, 65, rows=rows)
    assert ctx.region_links_text() == text and ctx.region_gfa_text(names_for(130)) == gfa


# ------------------------------------------------------------ 4. a label per row
def test_a_label_per_row(ctx):
    n = 100_000
    rng = np.random.default_rng(8)
    rows = make_rows(np.zeros(n, np.int64), rng.integers(0, 10 ** 6, n), rng.integers(-300, 3000, n), -1,
                     rng.permutation(n))
    ref, _, _ = check_device(ctx, rows, [0], 1, [b"r"])
    assert len(ref["link_from"]) == n - 1 and set(ref["link_count"]) == {1}
    assert set(ref["n_out"]) == {0, 1} and set(ref["n_in"]) == {0, 1}


# ------------------------------------------------------------ 5. genome counting
@pytest.mark.parametrize("G", [1, 2, 64, 65, 300])
def test_genome_counting(ctx, G):
    """One record per genome, rec_group a non-identity permutation.  Link
    (0, 1) occurs in every genome and four times in genome 0: once per genome;
    link (1, 2) only in the last genome."""
    rec_group = np.roll(np.arange(G, dtype=np.int32), 1) if G > 2 else np.arange(G, dtype=np.int32)[::-1].copy()
    rec, lab = [], []
    for r in range(G):
        g = int(rec_group[r])
        labs = [0, 1] * (4 if g == 0 else 1) + ([2] if g == G - 1 else [])
        rec += [r] * len(labs)
        lab += labs
    rows = make_rows(rec, np.arange(len(rec)) * 3, 2, 1, lab)
    ref, _, _ = check_device(ctx, rows, rec_group, G, names_for(G))
    links = dict(zip(zip(ref["link_from"], ref["link_to"]), zip(ref["link_count"], ref["link_genomes"])))
    assert links[(0, 1)] == (G + 3, G) and links[(1, 2)] == (1, 1) and links[(1, 0)] == (3, 1)
    assert G <= 2 or not np.array_equal(rec_group, np.arange(G))


# ------------------------------------------------------------ 6. self link, label gap, range
def test_self_link_gap_and_range(ctx):
    from pangenome_amd._lib import PangenomeError
    rec_group = np.array([0, 1, -1, 2], np.int32)
    rows = make_rows([0, 0, 0, 0, 1, 1, 2, 3, 3], [0, 5, 9, 100, 7, 7, 50, 1, 4], [10, 3, 0, 27, 40, 40, 6, 8, 1],
                     [1, 1, 1, 1, -1, -1, 1, -1, -1], [0, 5, 5, 2 ** 20 + 3, 5, 0, 5, 2 ** 20 + 3, 5])
    ref, text, gfa = check_device(ctx, rows, rec_group, 3, names_for(4))
    assert ref["labels"] == [0, 5, 2 ** 20 + 3] and ref["n_skipped"] == 1
    assert (5, 5) in set(zip(ref["link_from"], ref["link_to"])) and (2 ** 20 + 3, 5) in set(zip(ref["link_from"],
                                                                                                   ref["link_to"]))
    # a label of 2^31 needs 2^31 + 1 dense entries: PG_ERANGE, and the previous result stays
    big = rows.copy()
    big[0, 4] = 2 ** 31
    with pytest.raises(PangenomeError, match=r"pg_region_graph failed \(-34\)"):
        ctx.region_graph(rec_group, 3, rows=big)
    assert ctx.region_links_text() == text and ctx.region_gfa_text(names_for(4)) == gfa
    assert_same(device_tables(ctx), ref)
    big[0, 0] = 2                                        # the same label on a record without a genome: skipped
    check_device(ctx, big, rec_group, 3, names_for(4))


# ------------------------------------------------------------ 7. random
def random_case(n_records, G, n=100_000, n_labels=3000, seed=11):
    rng = np.random.default_rng(seed)
    rec_group = rng.permutation(np.arange(n_records) % G).astype(np.int32)
    rows = make_rows(np.sort(rng.integers(0, n_records, n)), rng.integers(0, 10 ** 7, n), rng.integers(-500, 20000, n),
                     rng.choice([1, -1], n), rng.integers(0, n_labels, n))
    rows[rng.integers(0, n, 100), 4] = -1
    return rows, rec_group


@pytest.mark.parametrize("n_records,G", [(90, 37), (3000, 3000)])
def test_random(ctx, n_records, G):
    rows, rec_group = random_case(n_records, G, seed=11 + G)
    ref, text, gfa = check_device(ctx, rows, rec_group, G, names_for(n_records))
    assert len(ref["labels"]) == 3000 and ref["n_skipped"] > 90 and len(ref["path_steps"]) > 10_000


# ------------------------------------------------------------ 8. argument errors
def test_argument_errors(ctx):
    """Refused before any launch: no device fault is involved."""
    from pangenome_amd._lib import Context, PangenomeError, _names_blob, ptr
    rows, rec_group = random_case(9, 4, n=500, n_labels=20)
    names = names_for(9)
    ref, text, gfa = check_device(ctx, rows, rec_group, 4, names)
    n = C.c_uint64()
    lib, r5, g = ctx.lib, np.ascontiguousarray(rows), np.ascontiguousarray(rec_group)

    def graph(h, r, nr, grp, nrec, G):
        return lib.pg_region_graph(h, r, nr, grp, nrec, G, None, None, None, None)
    assert graph(None, ptr(r5), 500, ptr(g), 9, 4) == -22
    assert graph(ctx.h, ptr(r5), 500, None, 9, 4) == -22
    for bad in (4, -2):
        g2 = g.copy()
        g2[3] = bad
        assert graph(ctx.h, ptr(r5), 500, ptr(g2), 9, 4) == -22
    assert graph(ctx.h, ptr(r5), 500, ptr(g), 8, 4) == -22               # a row names record 8
    r2 = r5.copy()
    r2[17, 0] = -1
    assert graph(ctx.h, ptr(r2), 500, ptr(g), 9, 4) == -22
    assert graph(ctx.h, ptr(r5), 500, ptr(np.full(9, -1, np.int32)), 9, 0) == -22
    nb, off = _names_blob(names)
    fresh = Context(27, 0)
    try:
        assert graph(fresh.h, None, 0, ptr(g), 9, 4) == -22              # no row pass yet
        for call in (fresh.region_nodes, fresh.region_links, fresh.region_paths, fresh.region_links_text,
                     lambda: fresh.region_links_write(1), lambda: fresh.region_gfa_text(names),
                     lambda: fresh.region_gfa_write(names, 1)):
            with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
                call()
    finally:
        fresh.close()
    # fewer names than the paths' records need (host rows: 1 + the largest record of a used row)
    need = 1 + max(ref["path_record"])
    assert lib.pg_region_gfa(ctx.h, ptr(nb), ptr(off), need - 1, None, 0, C.byref(n)) == -22
    assert lib.pg_region_gfa(ctx.h, ptr(nb), None, need, None, 0, C.byref(n)) == -22
    assert lib.pg_region_gfa(ctx.h, ptr(nb), ptr(off), need, None, 0, C.byref(n)) == 0 and n.value == len(gfa)
    # every refusal left the previous result in place
    assert ctx.region_links_text() == text and ctx.region_gfa_text(names) == gfa
    assert_same(device_tables(ctx), ref)
    buf = np.empty(len(gfa), np.uint8)
    assert lib.pg_region_links_format(ctx.h, ptr(buf), len(text) - 1, C.byref(n)) == -34
    assert lib.pg_region_links_format(ctx.h, ptr(buf), len(text), C.byref(n)) == 0
    assert buf[:len(text)].tobytes() == text
    assert lib.pg_region_gfa(ctx.h, ptr(nb), ptr(off), 9, ptr(buf), len(gfa) - 1, C.byref(n)) == -34
    assert lib.pg_region_gfa(ctx.h, ptr(nb), ptr(off), 9, ptr(buf), len(gfa), C.byref(n)) == 0
    assert buf.tobytes() == gfa
    nn, nl, npth = len(ref["labels"]), len(ref["link_from"]), len(ref["path_record"])
    a = np.empty(max(nn, nl, npth), np.int64)
    assert lib.pg_region_nodes(ctx.h, ptr(a), None, None, None, None, nn - 1) == -34
    assert lib.pg_region_nodes(ctx.h, ptr(a), None, None, None, None, nn) == 0 and a[:nn].tolist() == ref["labels"]
    assert lib.pg_region_links(ctx.h, None, ptr(a), None, None, nl - 1) == -34
    assert lib.pg_region_links(ctx.h, None, ptr(a), None, None, nl) == 0 and a[:nl].tolist() == ref["link_to"]
    assert lib.pg_region_paths(ctx.h, None, None, None, ptr(a), None, npth - 1) == -34
    assert lib.pg_region_paths(ctx.h, None, None, None, ptr(a), None, npth) == 0
    assert a[:npth].tolist() == ref["path_hi"]


# ------------------------------------------------------------ 9. _fd sinks
@pytest.mark.parametrize("which", ["links", "gfa"])
@pytest.mark.parametrize("sink", ["file", "append", "pipe"])
def test_region_write(ctx, tmp_path, sink, which):
    rows, rec_group = random_case(30, 7, n=20_000, n_labels=2500, seed=5)
    names = names_for(30)
    ctx.region_graph(rec_group, 7, rows=rows)
    ref = reference_region(rows, rec_group, 7)
    if which == "links":
        want, write = ctx.region_links_text(), ctx.region_links_write
        assert want.decode() == reference_links_text(ref)
    else:
        want, write = ctx.region_gfa_text(names), lambda fd: ctx.region_gfa_write(names, fd)
        assert want == reference_gfa(ref, names)
    if sink == "pipe":
        r, w = os.pipe()
        got = []
        th = threading.Thread(target=lambda: got.append(os.fdopen(r, "rb").read()))
        th.start()
        try:
            n = write(w)
        finally:
            os.close(w)
        th.join()
        data = got[0]
    else:
        fn = tmp_path / "out.txt"
        fn.write_bytes(b"# before\n")
        with open(fn, "ab" if sink == "append" else "r+b") as f:
            f.seek(0, os.SEEK_END)
            n = write(f.fileno())
            assert os.lseek(f.fileno(), 0, os.SEEK_CUR) == len(b"# before\n") + n
        data = fn.read_bytes()
        assert data.startswith(b"# before\n")
        data = data[len(b"# before\n"):]
    assert n == len(want) and data == want


# ------------------------------------------------------------ 10. device rows, golden
def test_device_rows_equal_host_rows(ctx):
    """rows=None takes the last row pass where it lies on the device: the same
    graph and bytes as the exported rows uploaded again, the reference's, and
    the committed expectation."""
    from pangenome_amd._lib import PangenomeError
    fx = Fixture("pan8_k27_c3")
    ctx.parse_host(np.frombuffer(fx.fasta, np.uint8))
    ctx.build_dbg(None, 0, True)
    ctx.build_rdbg()
    ctx.edges_count(None, True)
    ctx.cluster_cc(None, None, 4)
    n = ctx.rows_count(None, True)
    rows = ctx.rows_export(n)
    assert n == 2945
    rec_group = np.arange(8, dtype=np.int32)
    names = [x.split()[0].encode() for x in fasta_names(fx.fasta)]
    with pytest.raises(PangenomeError, match=r"pg_region_graph failed \(-22\)"):
        ctx.region_graph(rec_group[:7], 8)               # not the context's record count
    ref, text, gfa = check_device(ctx, rows, rec_group, 8, names, rows_on_device=True)
    with pytest.raises(PangenomeError, match=r"pg_region_gfa failed \(-22\)"):
        ctx.region_gfa_text(names[:7])                   # the context has eight records
    assert check_device(ctx, rows, rec_group, 8, names)[1:] == (text, gfa)
    want = golden("pan8_k27_c3_w4")
    got = summary(ref)
    assert {k: want[k] for k in got} == got
    assert (got["n_paths"], got["n_nodes"], got["n_links"], got["n_pairs"]) == (16, 909, 1947, 2929)
    # the frequency table and the graph do not touch each other
    ctx.freq(rec_group, 8)
    freq_text = ctx.freq_text()
    ctx.region_graph(rec_group, 8)
    assert ctx.freq_text() == freq_text and ctx.region_links_text() == text
    ctx.freq(rec_group, 8)
    assert ctx.region_gfa_text(names) == gfa


# ------------------------------------------------------------ 11. whole pipeline
def _run(km, d, fasta, extra):
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    km.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def _fr_files(q):
    return sorted(f[len("pan8.fsa"):] for f in os.listdir(os.path.dirname(q)) if "_fr_" in f)


OLD_FILES = ["_fr_freq.tsv", "_fr_genomes.tsv", "_fr_presence.npz", "_fr_spectrum.tsv"]
NEW_FILES = ["_fr_graph.gfa", "_fr_graph.npz", "_fr_links.tsv", "_fr_nodes.tsv"]


def test_cli(km, tmp_path):
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    names = fasta_names(fx.fasta)
    ids = [n.split()[0] for n in names]
    bids = [x.encode() for x in ids]
    q0, plain = _run(km, tmp_path / "plain", fx.fasta, ["-g", "record"])
    assert _fr_files(q0) == OLD_FILES                    # without -l: nothing new
    q, lines = _run(km, tmp_path / "links", fx.fasta, ["-g", "record", "-l", "1"])
    assert lines == plain                                # stdout (but the stage timings) is unchanged
    for suffix in ["_rdbg_weight.xyz", "_rdbg_weight.xyz.mcl"] + [s for s in OLD_FILES if s.endswith(".tsv")]:
        assert open(q + suffix, "rb").read() == open(q0 + suffix, "rb").read(), suffix
    z, z0 = np.load(q + "_fr_presence.npz"), np.load(q0 + "_fr_presence.npz")     # (a zip: its members carry a time)
    assert sorted(z.files) == sorted(z0.files) and all(np.array_equal(z[k], z0[k]) for k in z0.files)
    assert _fr_files(q) == sorted(OLD_FILES + NEW_FILES)
    rows = rows5_of(rows_of("\n".join(lines)), names)
    assert rows.shape[0] == 2945
    ref8 = reference_region(rows, list(range(8)), 8)
    assert_files(q, ref8, bids, ids)
    assert summary(ref8)["n_links"] == 1947
    # a group file: g0, g1 / g2 .. g5 / g6, g7
    gf = tmp_path / "groups.tsv"
    three = [0, 0, 1, 1, 1, 1, 2, 2]
    gf.write_text("".join("%s\t%s\n" % (i, "ABC"[g]) for i, g in zip(ids, three)))
    q, lines = _run(km, tmp_path / "file", fx.fasta, ["-g", str(gf), "-l1", "-p", "2"])
    assert lines == plain and len(_fr_files(q)) == 12
    ref3 = reference_region(rows, three, 3)
    assert_files(q, ref3, bids, ["A", "B", "C"])
    z = np.load(q + "_fr_graph.npz")
    assert z["link_genomes"].max() <= 3 and z["link_count"].tolist() == ref8["link_count"]
    # -n: the row pass walks the first five records only
    g = km.DeviceGraph(q0, 27)
    ns = int(g.seq_len[:5].sum()) - 1
    assert host.plan_rows(g.seq_len, g.shape, g.buf, ns).tolist() == [1, 1, 1, 1, 1, 0, 0, 0]
    g.ctx.close()
    q, lines = _run(km, tmp_path / "five", fx.fasta, ["-g", "record", "-l", "1", "-n", str(ns)])
    rows = rows5_of(rows_of("\n".join(lines)), names)
    ref5 = reference_region(rows, [0, 1, 2, 3, 4, -1, -1, -1], 5)
    assert_files(q, ref5, bids, ids[:5])
    assert set(np.load(q + "_fr_graph.npz")["path_record"].tolist()) == set(range(5))
    # refused before anything is built
    for i, extra in enumerate((["-l", "1"], ["-g", "record", "-l", "2"], ["-g", "record", "-l", "x"])):
        d = tmp_path / ("bad%d" % i)
        with pytest.raises(SystemExit):
            _run(km, d, fx.fasta, extra)
        assert os.listdir(str(d)) == ["pan8.fsa"]        # no <in>_db.npz
