"""The seven texts the library writes on the device, where one formatter
shared by all of them can go wrong: the digit count of every decimal column on
both sides of a power of ten (and of 2^64), signs, empty names, and the
agreement of a size-only call with the text that the fill call then writes.

Every text is compared byte for byte with a reference that shares nothing with
the device code: host.freq_text, tests/region_util.py, host.cluster_cc,
tests/seq_util.py and host.format_rows.  The inputs are a few hundred rows at
the most, but for the frequency table: its `rows` column crosses 999 / 1000
only with that many rows of one label (2 219 host rows in all).
"""
import ctypes as C

import numpy as np
import pytest

import region_util as ru
import seq_util as su
import walk_util as wu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    yield c
    c.close()


def size_only(c, fn, *lead):
    """The first half of the size-then-fill protocol alone: the bytes fn(h, *lead, NULL, 0, &n) announces."""
    from pangenome_amd._lib import ptr
    n = C.c_uint64(1 << 60)
    assert getattr(c.lib, fn)(c.h, *[ptr(a) if isinstance(a, np.ndarray) else a for a in lead], None, 0,
                              C.byref(n)) == 0
    return n.value


def digits(col):
    return {len(str(int(v))) for v in col}


# ------------------------------------------------------------ freq
FREQ_LABELS = (9, 10, 99, 100, 999, 1000, 99999, 100000)
FREQ_COUNTS = (9, 10, 99, 100, 999, 1000, 1, 1)
FREQ_LENGTHS = [10 ** k - d for k in range(1, 19) for d in (1, 0)]           # 9, 10, 99, 100, ... 10^18 - 1, 10^18


def freq_rows(G):
    """One record per genome.  Label FREQ_LABELS[i] has FREQ_COUNTS[i] rows, dealt to the first 9, 10 or G
    genomes in turn, on the + strand but for the last two labels; the lengths run through FREQ_LENGTHS from
    entry i on (the two labels of a thousand rows stop at 10^15, so that no sum passes 2^64), and the last
    two labels' single rows are 10^18 - 1 and 10^18 long."""
    rows = []
    for i, (lab, cnt) in enumerate(zip(FREQ_LABELS, FREQ_COUNTS)):
        spread = (9, 10, G)[i % 3]
        lens = FREQ_LENGTHS if cnt <= 100 else FREQ_LENGTHS[:30]
        for j in range(cnt):
            ln = FREQ_LENGTHS[28 + i] if cnt == 1 else lens[(j + i) % len(lens)]
            rows.append([j % spread, 5, 5 + ln, 1 if cnt > 1 else -1, lab])
    rows.sort(key=lambda r: r[0])
    return np.array(rows, np.int64)


@pytest.mark.parametrize("G", [10, 11])
def test_freq_text_digit_boundaries(ctx, G):
    from pangenome_amd import host
    rows, grp = freq_rows(G), np.arange(G, dtype=np.int32)
    t = host.freq_table(rows, grp, G)
    assert t["labels"].tolist() == list(FREQ_LABELS) and t["rows"].tolist() == list(FREQ_COUNTS)
    assert {9, 10, G} <= set(t["n_genomes"].tolist())
    assert t["plus"].tolist() == [9, 10, 99, 100, 999, 1000, 0, 0]
    assert t["min_len"].tolist()[:2] == [9, 10] and t["max_len"].tolist()[-2:] == [10 ** 18 - 1, 10 ** 18]
    assert digits(t["bp"]) >= {6, 7, 17, 18, 19}
    assert ctx.freq(grp, G, rows=rows) == (len(FREQ_LABELS), len(rows), 0)
    text = ctx.freq_text()
    assert text.decode() == host.freq_text(t)
    assert size_only(ctx, "pg_freq_format") == len(text)


# ------------------------------------------------------------ links and GFA
REGION_NAMES = [b"", b"a", b"rec2", b"the fourth record"]


def region_rows():
    """Record 0 (no name): labels 9 and 10 in turn, 20 rows from 0 to 10^12: links (9, 10) x 10 and (10, 9) x 9.
    Record 1 (a name of one letter): one row, a path of a single step, from 9 to 10.
    Record 2: the other strand, from a negative coordinate.  Record 3: two paths (the strand changes)."""
    rows = [[0, 0 if j == 0 else 100 * j, 10 ** 12 if j == 19 else 100 * j + 50, 1, (9, 10)[j % 2]] for j in range(20)]
    rows.append([1, 9, 10, 1, 99999])
    rows += [[2, -7, 40, -1, 99], [2, 100, 140, -1, 100], [2, 90000, 100000, -1, 100000]]
    rows += [[3, 10, 9, 1, 100], [3, 10, 999, 1, 99], [3, 2000, 1000, -1, 100000], [3, 1000, 10, -1, 99999]]
    return np.array(rows, np.int64)


def test_region_texts_digit_boundaries(ctx):
    rows, grp = region_rows(), np.array([0, 1, 1, 0], np.int32)
    ref, links, gfa = ru.check_device(ctx, rows, grp, 2, REGION_NAMES)         # (compares both texts)
    assert ref["labels"] == [9, 10, 99, 100, 99999, 100000]
    assert {9, 10} <= set(ref["link_count"]) and 1 in ref["path_steps"]
    assert {0, 9, -7} <= set(ref["path_lo"]) and {10, 10 ** 12} <= set(ref["path_hi"])
    for line in (b"P\t:0-1000000000000:+\t9+,10+,", b"P\ta:9-10:+\t99999+\t*\n", b"P\trec2:-7-100000:-\t"):
        assert line in gfa
    assert size_only(ctx, "pg_region_links_format") == len(links)
    from pangenome_amd._lib import _names_args
    assert size_only(ctx, "pg_region_gfa", *_names_args(REGION_NAMES)) == len(gfa)


# ------------------------------------------------------------ .mcl
def test_mcl_text_digit_boundaries(ctx):
    """Keys on both sides of 10, of 10^19 and at 2^64 - 1.  A value above 2^32 - 1 is refused by the pass
    (-22, "node value above 2^32"), so the values stop there: 0, 9, 10, 10^9 - 1, 10^9 and 2^32 - 1.
    min_weight 2: a cluster of three nodes, one of a single edge, and the two ends of a light edge alone."""
    from pangenome_amd import host
    big = 2 ** 64 - 1
    t = np.array([[0, 0, 9, 9], [9, 9, 10, 10],
                  [10 ** 19 - 1, 10 ** 9 - 1, 10 ** 19, 10 ** 9],
                  [big, 2 ** 32 - 1, 0, 2 ** 32 - 1]], np.uint64)
    cnt = np.array([2, 5, 2, 1], np.int64)
    want, wk, wv, wi = host.cluster_cc(t, cnt, 2)
    assert want == ("0_0\t9_9\t10_10\n9999999999999999999_999999999\t10000000000000000000_1000000000\n"
                    "18446744073709551615_4294967295\n0_4294967295\n")
    assert ctx.cluster_cc(t, cnt, 2) == (4, 7)
    text = ctx.clusters_text()
    assert text.decode() == want
    assert size_only(ctx, "pg_clusters_format") == len(text)
    for got, ref in zip(ctx.labels(), (wk, wv, wi)):                     # the write pass's side output
        assert np.array_equal(got, ref)


# ------------------------------------------------------------ FASTA and GFA with sequences
def test_sequence_texts_digit_boundaries(ctx):
    """Representatives of 9, 10, 15, 16, 17, 99 and 100 letters (the digits of `len=` and the decoder's
    16-letter chunk), labels 8 to 11 and 99 / 100, both strands; a shorter row of every label beside them."""
    rng = np.random.default_rng(5)
    seqs = [bytes(np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, n)]) for n in (400, 37)]
    names, seqs = su.parse(ctx, su.make_fasta(seqs, names=[b"", b"b"]))
    rows, lo = [], 3
    for j, (ln, lab) in enumerate(zip((9, 10, 15, 16, 17, 99, 100), (8, 9, 10, 11, 12, 99, 100))):
        rows.append([0, lo, lo + ln, 1, lab] if j % 2 else [0, lo + ln, lo, -1, lab])
        rows.append([1, 2, 2 + min(ln - 1, 30), 1, lab])
        lo += ln + 1
    ref, fasta = su.check_device(ctx, rows, [0, 1], 2, names, seqs, graph=True)      # (compares both texts)
    assert ref["len"] == [9, 10, 15, 16, 17, 99, 100] and set(ref["strand"]) == {1, -1}
    from pangenome_amd._lib import _names_args
    assert size_only(ctx, "pg_region_fasta", *_names_args(names)) == len(fasta)
    assert size_only(ctx, "pg_region_gfa_seq", *_names_args(names)) == len(ctx.region_gfa_seq_text(names))


# ------------------------------------------------------------ rows
K = 11
ROW_IDS = np.array([9, 10, 99, 100, 10 ** 18, -1, -2 ** 63, 999999999, 10 ** 9, 2 ** 31 - 1, -2 ** 31], np.int64)


@pytest.fixture(scope="module")
def rows_case(oracle_mod):
    """A context of its own after set_labels + rows over three short records: (context, rows, names, text).
    set_labels takes every id, the negative ones too; the row pass keeps an id's low 32 bits (10^18 and -2^63
    come back as other numbers) and gives a hit labelled -1 no row, so the boundaries that the text can show
    are those of 32 bits, which 2^31 - 1 and -2^31 add."""
    from pangenome_amd import host
    from pangenome_amd._lib import Context
    rng = np.random.default_rng(3)
    fasta = wu.fasta_bytes([(h, wu._dna(rng, n)) for h, n in (("", 600), ("q", 450), ("third record", 700))])
    keys, vals = wu.dense_table(*oracle_mod.OracleRun(fasta, K, 3).dbg())
    c = Context(K, 0)
    c.set_fasta(np.frombuffer(fasta, np.uint8))
    assert c.parse()[0] == 3
    c.set_labels(keys, vals, ROW_IDS[wu.hash_ids(keys, vals, len(ROW_IDS))])
    rows = c.rows(None, True)
    _, hs, hl = wu.record_table(fasta)
    want = "".join(x + "\n" for x in host.format_rows(rows, fasta, hs, hl)).encode()
    yield c, rows, wu.names_of(fasta), want
    c.close()


def test_rows_text_digit_boundaries(rows_case):
    c, rows, names, want = rows_case
    labs = set(rows[:, 4].tolist())
    assert 100 < len(rows) < 400 and {9, 10, 99, 100, 999999999, 10 ** 9, 2 ** 31 - 1, -2 ** 31} <= labs
    assert [len(x) for x in names] == [0, 1, 12]
    text = c.rows_text(names)
    assert text == want
    from pangenome_amd._lib import _names_args
    assert size_only(c, "pg_rows_format", *_names_args(names)) == len(text)


def test_rows_text_refuses_bad_names(rows_case):
    """Offsets that do not ascend, and no names beside a last offset above 0: -22, and the next valid call's
    text is what it was.  (Before the names went through names_upload the call read the device names out of
    bounds instead: this test alone does not pass on the commit before.)"""
    from pangenome_amd._lib import _names_blob, ptr
    c, rows, names, want = rows_case
    blob, off = _names_blob(names)
    n = C.c_uint64(77)
    out = np.zeros(len(want) + 64, np.uint8)
    down = off[::-1].copy()
    for args in ((ptr(blob), ptr(down)), (None, ptr(off))):
        for o, cap in ((None, 0), (ptr(out), out.shape[0])):
            assert c.lib.pg_rows_format(c.h, *args, len(names), o, cap, C.byref(n)) == -22
            assert n.value == 77 and not out.any()
        assert c.rows_text(names) == want
