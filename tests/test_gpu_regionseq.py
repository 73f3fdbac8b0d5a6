"""The region sequences on the device (pg_region_seqs, pangenome_amd/csrc/pg_regionseq.hip).

Every case compares, exactly, the three returned counts, region_seqs_table()
with its dtypes, region_seqs_bases() and region_fasta_text() - and, where a
graph is made of the same rows, region_gfa_seq_text() - with an independent
list-based reference (tests/seq_util.py).  The synthetic shapes are the
smallest at which each mechanism can go wrong: every alignment of a region's
start against the 16-base words of the packed stream, lengths around one, two
and four words, the stream's last word, exceptions at word boundaries, ties
across a wave and a 256-row tile, one hot label, more chunks than a block has
threads, more entries than one block searches, and more chunks than the
decoder's capped grid takes in one round.
"""
import ctypes as C
import io
import os
import threading

import numpy as np
import pytest

from freq_util import fasta_names, rows5_of, rows_of
from golden_util import Fixture
from region_util import reference_region
from seq_util import (assert_files, check_device, device_state, fasta_records, golden, make_fasta, parse,
                      reference_fasta, reference_gfa_seq, reference_seqs, summary)

pytestmark = pytest.mark.gpu

STRIDE = 2048 * 256 * 16                                 # letters the decoder's capped grid takes in one round


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


def acgt(n, seed):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def row(rec, lo, length, strand, label):
    """A row as the row pass gives it: start < end on the + strand, start > end on the other."""
    return [rec, lo, lo + length, 1, label] if strand == 1 else [rec, lo + length, lo, -1, label]


# ------------------------------------------------------------ 1. empty and tiny
def test_empty_and_tiny(ctx):
    names, seqs = parse(ctx, make_fasta([acgt(1, 1), acgt(17, 2), acgt(33, 3)]))
    grp = [0, 0, 0]
    ref, text = check_device(ctx, np.zeros((0, 5), np.int64), grp, 1, names, seqs, graph=True)
    assert text == b"" and ctx.region_fasta_text([]) == b"" and ctx.region_seqs_bases() == b""
    ref, text = check_device(ctx, [[1, 5, 5, 1, 0]], grp, 1, names, seqs, graph=True)          # length 0
    assert text == b">0 r1:5-5:+ len=0\n\n"
    for strand in (1, -1):
        ref, text = check_device(ctx, [row(1, 3, 1, strand, 0)], grp, 1, names, seqs, graph=True)
        assert ref["len"] == [1] and len(text.split(b"\n")[1]) == 1
        for rec in range(3):                                 # a whole record of length 1, 17 and 33
            ref, text = check_device(ctx, [row(rec, 0, len(seqs[rec]), strand, 4)], grp, 1, names, seqs, graph=True)
            assert ref["len"] == [len(seqs[rec])]
        whole = [row(rec, 0, len(seqs[rec]), strand, 9 - rec) for rec in range(3)]
        assert check_device(ctx, whole, grp, 1, names, seqs, graph=True)[0]["label"] == [7, 8, 9]


# ------------------------------------------------------------ 2. chunk alignment
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("before", [(), (1,), (17,), (33,), (1, 17, 33)])
def test_chunk_alignment(ctx, before):
    """A 700-base record at stream offsets 0, 1, 17, 33 and 51: a label for
    every lo % 16, every length around one, two, four and sixteen words, and
    both strands."""
    names, seqs = parse(ctx, make_fasta([acgt(n, 10 + n) for n in before] + [acgt(700, 5)]))
    rec = len(before)
    rows = []
    for strand in (1, -1):
        for length in LENGTHS:
            for lo16 in range(16):
                lo = lo16 + 16 * (len(rows) % 20)
                rows.append(row(rec, lo, length, strand, 3 * len(rows) + 1))
    assert len(rows) == 416 and max(max(r[1], r[2]) for r in rows) <= 700
    ref, _ = check_device(ctx, rows, [0] * (rec + 1), 1, names, seqs, graph=True)
    assert ref["len"] == [r[2] - r[1] if r[3] == 1 else r[1] - r[2] for r in rows]


# ------------------------------------------------------------ 3. end of the stream
@pytest.mark.parametrize("tail", [0, 1, 15])
def test_end_of_stream(tail):
    """The compacted stream has 64 + tail bases; regions end at its last base
    on both strands.  Every new device buffer is filled with 0xA5 first, so a
    read beyond the stream's last packed word would show as a wrong letter."""
    from pangenome_amd._lib import PG_TUNE_POISON, Context
    c = Context(27, 0)
    try:
        c.tune(PG_TUNE_POISON, 0xA5)
        names, seqs = parse(c, make_fasta([acgt(37, 7), acgt(27 + tail, 8 + tail)]))
        n = len(seqs[1])
        assert (37 + n) % 16 == tail
        rows = [row(1, n - length, length, strand, 2 * i + (strand == 1))
                for i, length in enumerate((1, 5, 15, 16, 17, n)) for strand in (1, -1)]
        rows += [row(0, 37 - length, length, strand, 100 + 2 * i + (strand == 1))
                 for i, length in enumerate((1, 16, 37)) for strand in (1, -1)]
        check_device(c, rows, [0, 0], 1, names, seqs, graph=True)
    finally:
        c.tune(PG_TUNE_POISON, -1)
        c.close()


# ------------------------------------------------------------ 4. exceptions
SPOTS = (0, 15, 16, 17, 31, 49)


def test_exceptions(ctx):
    """N, n, R, $ and lower-case acgt at bases 0, 15, 16, 17, 31 and the last
    of a record, and a record of only N: regions that start, end and straddle
    there, on both strands; gc and amb are part of the table."""
    recs = [bytearray(acgt(50, 20 + i)) for i in range(3)]
    for rec, marks in zip(recs, (b"NnR$ac", b"gtN$Rn", b"$RnNtg")):
        for p, ch in zip(SPOTS, marks):
            rec[p] = ch
    names, seqs = parse(ctx, make_fasta([b"ACGTA"] + [bytes(r) for r in recs] + [b"N" * 20, b"acgtn"]))
    assert seqs[1][:1] == b"N" and seqs[1][16:18] == b"NN" and seqs[1][31] == ord("A") and seqs[4] == b"N" * 20
    rows = []
    for rec in (1, 2, 3):
        for strand in (1, -1):
            for p in SPOTS:
                for lo, hi in ((p, min(p + 6, 50)), (max(p - 6, 0), p + 1), (max(p - 3, 0), min(p + 4, 50)), (p, p + 1),
                               (max(p - 20, 0), min(p + 20, 50))):
                    rows.append(row(rec, lo, hi - lo, strand, len(rows)))
            rows.append(row(rec, 0, 50, strand, len(rows)))
    rows += [row(4, 0, 20, 1, len(rows)), row(4, 2, 17, -1, len(rows) + 1), row(5, 0, 5, -1, len(rows) + 2)]
    ref, _ = check_device(ctx, rows, [0] * 6, 1, names, seqs, graph=True)
    assert sum(ref["amb"]) > 200 and ref["amb"][-3:] == [20, 17, 1] and ref["gc"][-3:] == [0, 0, 2]


# ------------------------------------------------------------ 5. choice of the representative
@pytest.mark.parametrize("tied", [(63, 64), (64, 255), (255, 256), (0, 256), (0, 63, 64, 255, 256), (63, 64, 299),
                                  (255, 256, 300)])
def test_ties(ctx, tied):
    """Rows of one label and equal length at different places, inside a wave,
    across a wave and across a 256-row tile: the first wins.  Row 299 is a
    strictly longer row that comes last; row 300 a longer one that is unused
    (its record has no genome)."""
    names, seqs = parse(ctx, make_fasta([acgt(2000, 31), acgt(100, 32)]))
    rows = [row(0, 5 * i, 7, 1 if i % 3 else -1, 10 + i) for i in range(299)]
    for i in tied:
        if i < 299:
            rows[i] = row(0, 3 * i + 11, 30, 1 if i % 2 else -1, 1)
    rows.append(row(0, 900, 31, -1, 1) if 299 in tied else row(0, 900, 3, 1, -1))
    rows.append(row(1, 10, 40, 1, 1) if 300 in tied else row(1, 10, 4, 1, 2))
    ref, _ = check_device(ctx, rows, [0, -1], 1, names, seqs, graph=True)
    assert ref["label"][0] == 1 and ref["row"][0] == (299 if 299 in tied else tied[0])
    assert ref["n_skipped"] == (1 if 299 in tied else 2)


def test_hot_label(ctx):
    """200 001 rows of one label, all of length 40 at different places: row 0
    is the representative; then one row of length 41 in the middle."""
    names, seqs = parse(ctx, make_fasta([acgt(3000, 33)]))
    n = 200_001
    i = np.arange(n, dtype=np.int64)
    start = (i * 7) % 2900
    rows = np.stack([np.zeros(n, np.int64), start, start + 40, np.ones(n, np.int64), np.full(n, 6, np.int64)], axis=1)
    ref, _ = check_device(ctx, rows, [0], 1, names, seqs)
    assert ref["row"] == [0] and ref["len"] == [40]
    rows[100_000] = row(0, 1234, 41, -1, 6)
    ref, _ = check_device(ctx, rows, [0], 1, names, seqs, graph=True)
    assert ref["row"] == [100_000] and ref["len"] == [41]


def test_label_gaps(ctx):
    names, seqs = parse(ctx, make_fasta([acgt(300, 34), acgt(90, 35)]))
    rows = [row(0, 3, 27, 1, 2 ** 20 + 3), row(0, 40, 30, -1, 0), row(1, 0, 90, -1, 2 ** 20 + 3), row(1, 5, 50, 1, 70_000),
            row(0, 100, 200, 1, 5), row(1, 1, 80, 1, 5)]
    ref, _ = check_device(ctx, rows, [0, 1], 2, names, seqs, graph=True)
    assert ref["label"] == [0, 5, 70_000, 2 ** 20 + 3] and ref["row"] == [1, 4, 3, 2]


# ------------------------------------------------------------ 6. load shape
def test_load_shape(ctx):
    """One region over a whole 300 000-base record on the - strand (its chunks
    fill many blocks), and 70 000 regions of 27 bases (more entries than one
    block searches, two chunks each, the second mostly padding)."""
    names, seqs = parse(ctx, make_fasta([acgt(300_000, 36)], width=1000))
    rows = [row(0, 0, 300_000, -1, 0)] + [row(0, (4 * i) % 299_973, 27, 1 if i % 2 else -1, i) for i in range(1, 70_001)]
    ref, _ = check_device(ctx, rows, [0], 1, names, seqs, graph=True)
    assert len(ref["label"]) == 70_001 and len(ref["bases"]) == 300_000 + 27 * 70_000


def test_more_than_one_stride(ctx):
    """Thirty regions over the whole record: 9 000 000 letters, more than the
    decoder's capped grid takes in one round (8 MiB of letters): its blocks
    loop, and a thread goes from one entry to the next."""
    names, seqs = parse(ctx, make_fasta([acgt(300_000, 37)], width=1000))
    rows = [row(0, 0, 300_000, 1 if i % 2 else -1, i) for i in range(30)]
    ref, _ = check_device(ctx, rows, [0], 1, names, seqs)
    assert STRIDE < len(ref["bases"]) <= 32 << 20


# ------------------------------------------------------------ 7. FASTA line widths
def test_line_widths(ctx):
    recs = [acgt(1234, 38), acgt(7, 39), acgt(2001, 40)]
    rows = [row(0, 3, 1200, -1, 2), row(1, 0, 7, 1, 0), row(2, 990, 1011, 1, 1), row(2, 0, 2001, -1, 8)]
    states = []
    for width in (7, 60, 1000):
        names, seqs = parse(ctx, make_fasta(recs, width=width))
        check_device(ctx, rows, [0, 0, 0], 1, names, seqs, graph=True)
        states.append(device_state(ctx, names) + (ctx.region_gfa_seq_text(names),))
    assert states[0] == states[1] == states[2]


# ------------------------------------------------------------ 8. errors and lifetime
def test_errors_and_lifetime(ctx):
    """Every refusal comes before any launch that could touch a bad address,
    and leaves the previous table, bases and texts in place."""
    from pangenome_amd._lib import Context, PangenomeError, _names_blob, ptr
    fasta = make_fasta([acgt(500, 41), acgt(64, 42), acgt(33, 43)])
    names, seqs = parse(ctx, fasta)
    rng = np.random.default_rng(9)
    rows = np.array([row(int(r), int(lo), int(ln), int(st), int(lab)) for r, lo, ln, st, lab in zip(
        rng.integers(0, 2, 400), rng.integers(0, 30, 400), rng.integers(0, 34, 400), rng.choice([1, -1], 400),
        rng.integers(0, 40, 400))], np.int64)
    rec_group = np.array([0, 1, -1], np.int32)
    ref, text = check_device(ctx, rows, rec_group, 2, names, seqs, graph=True)
    gfa = ctx.region_gfa_seq_text(names)
    state = device_state(ctx, names)
    lib, r5, g = ctx.lib, np.ascontiguousarray(rows), np.ascontiguousarray(rec_group)

    def unchanged():
        assert device_state(ctx, names) == state and ctx.region_gfa_seq_text(names) == gfa

    def seqs_rc(h, r, nr, grp, nrec, G):
        return lib.pg_region_seqs(h, r, nr, grp, nrec, G, None, None, None)
    assert seqs_rc(ctx.h, ptr(r5), 400, ptr(g), 3, 2) == 0
    unchanged()
    for bad in ([1, 60, 65, 1, 3], [1, 65, 0, -1, 3], [0, -1, 5, 1, 3], [0, 5, -1, -1, 3], [0, 0, 2 ** 40, 1, 3]):
        r2 = r5.copy()
        r2[123] = bad                                        # hi > seq_len, lo < 0: on either strand
        assert seqs_rc(ctx.h, ptr(r2), 400, ptr(g), 3, 2) == -22
    r2 = r5.copy()
    r2[7] = [2, 0, 34, 1, 3]                                 # ... but not on a record without a genome
    assert seqs_rc(ctx.h, ptr(r2), 400, ptr(g), 3, 2) == 0
    assert seqs_rc(ctx.h, ptr(r5), 400, ptr(g), 3, 2) == 0
    unchanged()
    assert seqs_rc(None, ptr(r5), 400, ptr(g), 3, 2) == -22
    assert seqs_rc(ctx.h, ptr(r5), 400, None, 3, 2) == -22
    assert seqs_rc(ctx.h, ptr(r5), 400, ptr(g), 2, 2) == -22                # another n_records (host rows too)
    assert seqs_rc(ctx.h, ptr(r5), 400, ptr(np.array([0, 1, -1, 0], np.int32)), 4, 2) == -22
    assert seqs_rc(ctx.h, ptr(r5), 400, ptr(np.array([0, 2, -1], np.int32)), 3, 2) == -22
    r2 = r5.copy()
    r2[17, 0] = 3
    assert seqs_rc(ctx.h, ptr(r2), 400, ptr(g), 3, 2) == -22               # a row names record 3
    assert seqs_rc(ctx.h, ptr(r5), 400, ptr(np.full(3, -1, np.int32)), 3, 0) == -22
    r2 = r5.copy()
    r2[0, 4] = 2 ** 31                                       # 2^31 + 1 dense entries
    assert seqs_rc(ctx.h, ptr(r2), 400, ptr(g), 3, 2) == -34
    unchanged()
    n = C.c_uint64()
    nb, off = _names_blob(names)
    fresh = Context(27, 0)
    try:
        assert seqs_rc(fresh.h, ptr(r5), 400, ptr(g), 3, 2) == -22         # no parse
        fresh.parse_host(np.frombuffer(fasta, np.uint8))
        assert seqs_rc(fresh.h, None, 0, ptr(g), 3, 2) == -22              # no row pass yet
        for call in (fresh.region_seqs_table, fresh.region_seqs_bases, lambda: fresh.region_fasta_text(names),
                     lambda: fresh.region_fasta_write(names, 1), lambda: fresh.region_gfa_seq_text(names),
                     lambda: fresh.region_gfa_seq_write(names, 1)):
            with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
                call()
        fresh.region_seqs(rec_group, 2, rows=rows)
        assert fresh.region_fasta_text(names) == text
        with pytest.raises(PangenomeError, match=r"pg_region_gfa_seq failed \(-22\)"):
            fresh.region_gfa_seq_text(names)                 # sequences, but no graph
    finally:
        fresh.close()
    # a graph of other rows: one label fewer, then the same labels with another length
    other = r5[r5[:, 4] != ref["label"][0]]
    ctx.region_graph(rec_group, 2, rows=other)
    assert lib.pg_region_gfa_seq(ctx.h, ptr(nb), ptr(off), 3, None, 0, C.byref(n)) == -22
    other = r5.copy()
    other[ref["row"][0]] = row(0, 100, 300, 1, ref["label"][0])
    ctx.region_graph(rec_group, 2, rows=other)
    assert lib.pg_region_gfa_seq(ctx.h, ptr(nb), ptr(off), 3, None, 0, C.byref(n)) == -22
    ctx.region_graph(rec_group, 2, rows=rows)
    unchanged()
    # short names (host rows: 1 + the largest record of a used row), short caps
    need = 1 + max(ref["record"])
    assert need == 2
    for fn in (lib.pg_region_fasta, lib.pg_region_gfa_seq):
        assert fn(ctx.h, ptr(nb), ptr(off), need - 1, None, 0, C.byref(n)) == -22
        assert fn(ctx.h, ptr(nb), None, need, None, 0, C.byref(n)) == -22
        want = text if fn is lib.pg_region_fasta else gfa
        assert fn(ctx.h, ptr(nb), ptr(off), need, None, 0, C.byref(n)) == 0 and n.value == len(want)
        buf = np.empty(len(want), np.uint8)
        assert fn(ctx.h, ptr(nb), ptr(off), 3, ptr(buf), len(want) - 1, C.byref(n)) == -34
        assert fn(ctx.h, ptr(nb), ptr(off), 3, ptr(buf), len(want), C.byref(n)) == 0 and buf.tobytes() == want
    nr = len(ref["label"])
    a = np.empty(nr, np.int64)
    assert lib.pg_region_seqs_table(ctx.h, ptr(a), *[None] * 9, nr - 1) == -34
    assert lib.pg_region_seqs_table(ctx.h, *[None] * 6, ptr(a), *[None] * 3, nr) == 0
    assert a.view(np.uint64).tolist() == ref["len"]
    buf = np.empty(len(ref["bases"]), np.uint8)
    assert lib.pg_region_seqs_bases(ctx.h, ptr(buf), len(buf) - 1, C.byref(n)) == -34
    assert lib.pg_region_seqs_bases(ctx.h, ptr(buf), len(buf), C.byref(n)) == 0 and buf.tobytes() == ref["bases"]
    unchanged()
    # the frequency table, the graph and the sequences do not touch each other
    ctx.freq(rec_group, 2, rows=rows)
    freq_text, plain = ctx.freq_text(), ctx.region_gfa_text(names)
    ctx.region_seqs(rec_group, 2, rows=rows)
    assert ctx.freq_text() == freq_text and ctx.region_gfa_text(names) == plain
    ctx.freq(rec_group, 2, rows=rows[:100])
    ctx.region_graph(rec_group, 2, rows=rows[:100])
    assert device_state(ctx, names) == state
    ctx.region_graph(rec_group, 2, rows=rows)
    unchanged()
    # a second parse of another FASTA leaves the result in place (it is a copy)
    ctx.parse_host(np.frombuffer(make_fasta([acgt(90, 44)] * 5), np.uint8))
    unchanged()


# ------------------------------------------------------------ 9. _fd sinks
@pytest.mark.parametrize("which", ["fasta", "gfa"])
@pytest.mark.parametrize("sink", ["file", "append", "pipe"])
def test_region_seq_write(ctx, tmp_path, sink, which):
    names, seqs = parse(ctx, make_fasta([acgt(5000, 45), acgt(777, 46)]))
    rng = np.random.default_rng(6)
    rows = [row(int(r), int(lo), int(ln), int(st), int(lab)) for r, lo, ln, st, lab in zip(
        rng.integers(0, 2, 3000), rng.integers(0, 300, 3000), rng.integers(0, 470, 3000), rng.choice([1, -1], 3000),
        rng.integers(0, 900, 3000))]
    ref, text = check_device(ctx, rows, [0, 1], 2, names, seqs, graph=True)
    if which == "fasta":
        want, write = text, lambda fd: ctx.region_fasta_write(names, fd)
    else:
        want, write = ctx.region_gfa_seq_text(names), lambda fd: ctx.region_gfa_seq_write(names, fd)
        assert want == reference_gfa_seq(reference_region(rows, [0, 1], 2), ref, names)
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
def test_device_rows_and_golden(ctx):
    """rows=None takes the last row pass where it lies on the device: the same
    table and bytes as the exported rows uploaded again, the reference's, and
    the committed expectation."""
    fx = Fixture("pan8_k27_c3")
    names, seqs = parse(ctx, fx.fasta)
    ctx.build_dbg(None, 0, True)
    ctx.build_rdbg()
    ctx.edges_count(None, True)
    ctx.cluster_cc(None, None, 4)
    n = ctx.rows_count(None, True)
    rows = ctx.rows_export(n)
    assert n == 2945
    rec_group = np.arange(8, dtype=np.int32)
    ids = [x.split()[0] for x in names]
    ref, text = check_device(ctx, rows, rec_group, 8, ids, seqs, rows_on_device=True, graph=True)
    gfa = ctx.region_gfa_seq_text(ids)
    assert check_device(ctx, rows, rec_group, 8, ids, seqs, graph=True)[1] == text
    assert ctx.region_gfa_seq_text(ids) == gfa
    got = summary(ref, ids)
    assert got == golden("pan8_k27_c3_w4") and got["n_regions"] == 909
    plain = ctx.region_gfa_text(ids).split(b"\n")
    for a, b in zip(gfa.split(b"\n"), plain):
        if a.startswith(b"S\t"):
            f = a.split(b"\t")
            assert len(f[2]) == int(f[3][len("LN:i:"):])
        else:
            assert a == b
    assert sum(ln.startswith(b"S\t") for ln in plain) == 909 and len(plain) == gfa.count(b"\n") + 1


# ------------------------------------------------------------ 11. whole pipeline
def _run(km, d, fasta, extra):
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    km.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def _files(q):
    return sorted(f[len("pan8.fsa"):] for f in os.listdir(os.path.dirname(q)) if f != "pan8.fsa")


def _same_files(q, q0):
    """Every file of the run in q0's directory is in q's, byte for byte (an npz: array for array)."""
    for suffix in _files(q0):
        if suffix.endswith(".npz"):
            z, z0 = np.load(q + suffix), np.load(q0 + suffix)               # (a zip: its members carry a time)
            assert sorted(z.files) == sorted(z0.files) and all(np.array_equal(z[k], z0[k]) for k in z0.files), suffix
        else:
            assert open(q + suffix, "rb").read() == open(q0 + suffix, "rb").read(), suffix


SEQ_FILES = ["_fr_regions.fa", "_fr_regions.tsv"]


def test_cli(km, tmp_path):
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    names = fasta_names(fx.fasta)
    ids = [n.split()[0].encode() for n in names]
    seqs = fasta_records(fx.fasta)[1]
    q0, plain = _run(km, tmp_path / "plain", fx.fasta, ["-g", "record"])
    q, lines = _run(km, tmp_path / "seqs", fx.fasta, ["-g", "record", "-s", "1"])
    assert lines == plain                                # stdout (but the stage timings) is unchanged
    assert _files(q) == sorted(_files(q0) + SEQ_FILES)   # no _fr_graph_seq.gfa without -l 1
    _same_files(q, q0)
    rows = rows5_of(rows_of("\n".join(lines)), names)
    assert rows.shape[0] == 2945
    ref8 = reference_seqs(rows, list(range(8)), 8, seqs)
    assert_files(q, ref8, ids)
    assert summary(ref8, ids) == golden("pan8_k27_c3_w4")
    # with the graph
    q1, lines = _run(km, tmp_path / "links", fx.fasta, ["-g", "record", "-l", "1"])
    q, lines2 = _run(km, tmp_path / "both", fx.fasta, ["-g", "record", "-l", "1", "-s1"])
    assert lines == lines2 == plain and _files(q) == sorted(_files(q1) + SEQ_FILES + ["_fr_graph_seq.gfa"])
    _same_files(q, q1)
    assert_files(q, ref8, ids, reference_region(rows, list(range(8)), 8))
    # a group file: g0, g1 / g2 .. g5 / g6, g7 (the sequences do not depend on the grouping of used records)
    gf = tmp_path / "groups.tsv"
    three = [0, 0, 1, 1, 1, 1, 2, 2]
    gf.write_text("".join("%s\t%s\n" % (i.decode(), "ABC"[g]) for i, g in zip(ids, three)))
    q, lines = _run(km, tmp_path / "file", fx.fasta, ["-g", str(gf), "-s", "1", "-p", "2"])
    assert lines == plain
    assert_files(q, reference_seqs(rows, three, 3, seqs), ids)
    assert open(q + "_fr_regions.fa", "rb").read() == reference_fasta(ref8, ids)
    # -n: the row pass walks the first five records only
    g = km.DeviceGraph(q0, 27)
    ns = int(g.seq_len[:5].sum()) - 1
    assert host.plan_rows(g.seq_len, g.shape, g.buf, ns).tolist() == [1, 1, 1, 1, 1, 0, 0, 0]
    g.ctx.close()
    q, lines = _run(km, tmp_path / "five", fx.fasta, ["-g", "record", "-l", "1", "-s", "1", "-n", str(ns)])
    rows = rows5_of(rows_of("\n".join(lines)), names)
    grp5 = [0, 1, 2, 3, 4, -1, -1, -1]
    ref5 = reference_seqs(rows, grp5, 5, seqs)
    assert_files(q, ref5, ids, reference_region(rows, grp5, 5))
    assert set(ref5["record"]) <= set(range(5)) and len(ref5["label"]) < 909
    # refused before anything is built
    for i, extra in enumerate((["-s", "1"], ["-g", "record", "-s", "2"], ["-g", "record", "-s", "x"], ["-s1"])):
        d = tmp_path / ("bad%d" % i)
        with pytest.raises(SystemExit):
            _run(km, d, fx.fasta, extra)
        assert os.listdir(str(d)) == ["pan8.fsa"]        # no <in>_db.npz
