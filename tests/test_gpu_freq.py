"""The frequency table on the device (pg_freq, pangenome_amd/csrc/pg_freq.hip).

Every case compares, exactly, freq_table(), freq_spectrum(), freq_groups(),
freq_text() and the returned counts with an independent dict-based reference
(tests/freq_util.py).  The synthetic shapes are the smallest at which each
mechanism can go wrong: presence-word boundaries, one hot label across many
blocks, waves of mixed labels, a label per row, label gaps, and more genomes
than the per-genome pass holds in LDS.
"""
import io
import os
import threading

import numpy as np
import pytest

from freq_util import (GROUP_COLS, assert_files, assert_same, check_device, device_table, fasta_names, golden,
                       reference_freq, reference_text, rows5_of, rows_of)
from golden_util import Fixture

pytestmark = pytest.mark.gpu

HEADER = b"#label\tgenomes\trows\tplus\tbp\tmin\tmax\n"


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


def test_empty_then_one_row(ctx):
    ref, text = check_device(ctx, np.zeros((0, 5), np.int64), np.zeros(0, np.int32), 0)
    assert text == HEADER and ctx.freq_spectrum()[0].tolist() == [0]
    ref, text = check_device(ctx, np.zeros((0, 5), np.int64), np.array([0, 1, 0], np.int32), 2)
    assert text == HEADER and ctx.freq_spectrum()[0].tolist() == [0, 0, 0]
    assert ctx.freq_groups()["g_bp"].tolist() == [0, 0]
    ref, text = check_device(ctx, [[1, 40, 13, -1, 0]], [-1, 0], 1)
    assert text == HEADER + b"0\t1\t1\t0\t27\t27\t27\n"
    assert ctx.freq_groups()["g_core"].tolist() == [27]


@pytest.mark.parametrize("G", [1, 63, 64, 65, 129])
def test_presence_word_boundaries(ctx, G):
    """One record per genome.  Label 0 in every genome (core), label 1 only
    in the last genome, label 2 only in genome 0, label 3 in genomes 63 and 64
    (two presence words) where they exist."""
    rec = list(range(G)) + [G - 1, 0] + [g for g in (63, 64) if g < G]
    lab = [0] * G + [1, 2] + [3 for g in (63, 64) if g < G]
    rows = make_rows(rec, np.arange(len(rec)) * 7, np.arange(len(rec)) + 1, 1, lab)
    ref, _ = check_device(ctx, rows, np.arange(G, dtype=np.int32), G)
    assert ref["n_genomes"][0] == G and ref["spectrum_labels"][G] >= 1
    if G >= 65:
        assert ref["bits"][3][:2] == [1 << 63, 1]


def test_one_hot_label(ctx):
    """200,000 rows of label 3 over 65 genomes and both strands, lengths near
    2^31 (total_bp passes 2^32 inside one wave's sum), one row of label 0 in
    the middle (a wave of two labels) and one at the very end (the last wave
    is partial).  Twice: the same bytes."""
    rng = np.random.default_rng(3)
    n = 200_000
    rec = np.sort(rng.integers(0, 130, n))
    rows = make_rows(rec, rng.integers(0, 1000, n), 2 ** 31 - rng.integers(0, 5000, n), rng.choice([1, -1], n), 3)
    rows[n // 2, 4] = 0
    rows = np.concatenate([rows, make_rows([129], 5, 9, -1, 0)])
    assert rows.shape[0] % 64 != 0
    rec_group = (np.arange(130) % 65).astype(np.int32)
    ref, text = check_device(ctx, rows, rec_group, 65)
    assert ref["labels"] == [0, 3] and ref["bp"][1] > 2 ** 32 * 64 and ref["n_genomes"][1] == 65
    ctx.freq(rec_group, 65, rows=rows)
    assert ctx.freq_text() == text


def test_mixed_label_waves(ctx):
    """64 x 50 rows, lane i of every wave has label i % 7; then every row its
    own label (10,000 labels): the aggregation loop's worst case."""
    n = 64 * 50
    rng = np.random.default_rng(7)
    rows = make_rows(np.sort(rng.integers(0, 20, n)), rng.integers(0, 10 ** 6, n), rng.integers(-300, 3000, n),
                     rng.choice([1, -1], n), np.arange(n) % 64 % 7)
    ref, _ = check_device(ctx, rows, (np.arange(20) % 6).astype(np.int32), 6)
    assert ref["labels"] == list(range(7))
    n = 10_000
    rows = make_rows(np.sort(rng.integers(0, 20, n)), rng.integers(0, 10 ** 6, n), rng.integers(-300, 3000, n),
                     rng.choice([1, -1], n), rng.permutation(n))
    ref, _ = check_device(ctx, rows, (np.arange(20) % 6).astype(np.int32), 6)
    assert len(ref["labels"]) == n and ref["spectrum_labels"][1] == n


FORM_TEXT = {}                                           # n -> the text of the form that ran first


@pytest.mark.parametrize("form", [0, 1])
def test_accumulate_forms(ctx, form):
    """Both accumulate passes (PG_TUNE_FREQ_FORM 0: aggregated in the wave, 1:
    every lane its own atomics) at the wave and tile edges of the row loader.
    Every full wave holds a label shared by 40 lanes, one shared by 2, lanes
    with a label of their own and unused lanes (label -1, or record 7, which
    has no genome).  5 genomes over 10 records, both strands; the two forms
    give the same bytes."""
    from pangenome_amd import _lib
    rec_group = (np.arange(10) % 5).astype(np.int32)
    rec_group[7] = -1
    ctx.tune(_lib.PG_TUNE_FREQ_FORM, form)
    try:
        for n in (1, 63, 64, 65, 255, 256, 257, 513):
            i = np.arange(n)
            lab = np.where(i % 64 < 40, 0, np.where(i % 64 < 42, 1, i))
            lab[16::17] = -1
            rows = make_rows(i * 10 // n, i * 3, i % 29 + 1, np.where(i % 3 == 0, -1, 1), lab)
            ref, text = check_device(ctx, rows, rec_group, 5)
            assert ref["n_skipped"] >= n // 17 and (n < 64 or ref["labels"][:2] == [0, 1])
            assert FORM_TEXT.setdefault(n, text) == text
    finally:
        ctx.tune(_lib.PG_TUNE_FREQ_FORM, 0)


def test_label_gaps_and_skips(ctx):
    rec_group = np.array([0, 1, -1, 2], np.int32)
    rows = make_rows([0, 1, 3, 0, 1, 2, 3, 2], [0, 5, 9, 100, 7, 7, 50, 1], [10, 3, 0, 27, 40, 40, 6, 8],
                     [1, -1, 1, 1, -1, 1, -1, 1], [0, 5, 2 ** 20 + 3, -1, -7, 5, 5, 0])
    ref, text = check_device(ctx, rows, rec_group, 3)
    assert ref["labels"] == [0, 5, 2 ** 20 + 3] and (ref["n_used"], ref["n_skipped"]) == (4, 4)
    # a label of 2^31 needs 2^31 + 1 dense entries: PG_ERANGE, and the previous result stays
    from pangenome_amd._lib import PangenomeError
    big = rows.copy()
    big[0, 4] = 2 ** 31
    with pytest.raises(PangenomeError, match=r"pg_freq failed \(-34\)"):
        ctx.freq(rec_group, 3, rows=big)
    assert ctx.freq_text() == text
    assert_same(device_table(ctx), ref)
    big[0, 0] = 2                                        # the same label on a record without a genome: skipped
    check_device(ctx, big, rec_group, 3)


def random_case(n_records, G, n=100_000, n_labels=3000, seed=11):
    rng = np.random.default_rng(seed)
    rec_group = rng.permutation(np.arange(n_records) % G).astype(np.int32)
    rows = make_rows(np.sort(rng.integers(0, n_records, n)), rng.integers(0, 10 ** 7, n), rng.integers(-500, 20000, n),
                     rng.choice([1, -1], n), rng.integers(0, n_labels, n))
    rows[rng.integers(0, n, 100), 4] = -1
    return rows, rec_group


def test_random(ctx):
    rows, rec_group = random_case(90, 37)
    assert not np.array_equal(rec_group, np.arange(90))
    ref, text = check_device(ctx, rows, rec_group, 37)
    assert len(ref["labels"]) == 3000
    ctx.freq(rec_group, 37, rows=rows)
    assert ctx.freq_text() == text


def test_random_many_genomes(ctx):
    """3,000 genomes: the per-genome pass leaves its LDS form (1,024 genomes)
    and the spectrum its LDS bins (2,048)."""
    rows, rec_group = random_case(3000, 3000, seed=12)
    check_device(ctx, rows, rec_group, 3000)


def test_argument_errors(ctx):
    """Refused before any launch: no device fault is involved."""
    import ctypes as C
    from pangenome_amd._lib import Context, PangenomeError, ptr
    rows, rec_group = random_case(9, 4, n=500, n_labels=20)
    ref, text = check_device(ctx, rows, rec_group, 4)
    n = C.c_uint64()
    lib, r5, g = ctx.lib, np.ascontiguousarray(rows), np.ascontiguousarray(rec_group)
    assert lib.pg_freq(None, ptr(r5), 500, ptr(g), 9, 4, None, None, None) == -22
    assert lib.pg_freq(ctx.h, ptr(r5), 500, None, 9, 4, None, None, None) == -22
    for bad in (4, -2):
        g2 = g.copy()
        g2[3] = bad
        assert lib.pg_freq(ctx.h, ptr(r5), 500, ptr(g2), 9, 4, None, None, None) == -22
    assert lib.pg_freq(ctx.h, ptr(r5), 500, ptr(g), 8, 4, None, None, None) == -22       # a row names record 8
    r2 = r5.copy()
    r2[17, 0] = -1
    assert lib.pg_freq(ctx.h, ptr(r2), 500, ptr(g), 9, 4, None, None, None) == -22
    assert lib.pg_freq(ctx.h, ptr(r5), 500, ptr(np.full(9, -1, np.int32)), 9, 0, None, None, None) == -22
    fresh = Context(27, 0)
    try:
        assert lib.pg_freq(fresh.h, None, 0, ptr(g), 9, 4, None, None, None) == -22      # no row pass yet
        with pytest.raises(PangenomeError, match=r"pg_freq_format failed \(-22\)"):
            fresh.freq_text()
        for call in (fresh.freq_table, fresh.freq_spectrum, fresh.freq_groups):
            with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
                call()
        with pytest.raises(PangenomeError, match=r"pg_freq_format_fd failed \(-22\)"):
            fresh.freq_write(1)
    finally:
        fresh.close()
    # every refusal left the previous result in place
    assert ctx.freq_text() == text
    buf = np.empty(len(text), np.uint8)
    assert lib.pg_freq_format(ctx.h, ptr(buf), len(text) - 1, C.byref(n)) == -34
    assert lib.pg_freq_format(ctx.h, ptr(buf), len(text), C.byref(n)) == 0 and buf.tobytes() == text
    nl = len(ref["labels"])
    lab = np.empty(nl, np.int64)
    assert lib.pg_freq_export(ctx.h, ptr(lab), None, None, None, None, None, None, None, nl - 1) == -34
    assert lib.pg_freq_export(ctx.h, ptr(lab), None, None, None, None, None, None, None, nl) == 0
    assert lab.tolist() == ref["labels"]
    a = np.empty(5, np.uint64)
    assert lib.pg_freq_spectrum(ctx.h, ptr(a), None, 4) == -34 and lib.pg_freq_spectrum(ctx.h, ptr(a), None, 5) == 0
    assert a.tolist() == ref["spectrum_labels"]
    assert lib.pg_freq_groups(ctx.h, ptr(a), None, None, None, None, 3) == -34


@pytest.mark.parametrize("sink", ["file", "append", "pipe"])
def test_freq_write(ctx, tmp_path, sink):
    rows, rec_group = random_case(30, 7, n=20_000, n_labels=2500, seed=5)
    ctx.freq(rec_group, 7, rows=rows)
    want = ctx.freq_text()
    assert want.decode() == reference_text(reference_freq(rows, rec_group, 7))
    if sink == "pipe":
        r, w = os.pipe()
        got = []
        th = threading.Thread(target=lambda: got.append(os.fdopen(r, "rb").read()))
        th.start()
        try:
            n = ctx.freq_write(w)
        finally:
            os.close(w)
        th.join()
        data = got[0]
    else:
        fn = tmp_path / "out.tsv"
        fn.write_bytes(b"# before\n")
        with open(fn, "ab" if sink == "append" else "r+b") as f:
            f.seek(0, os.SEEK_END)
            n = ctx.freq_write(f.fileno())
            assert os.lseek(f.fileno(), 0, os.SEEK_CUR) == len(b"# before\n") + n
        data = fn.read_bytes()
        assert data.startswith(b"# before\n")
        data = data[len(b"# before\n"):]
    assert n == len(want) and data == want


def test_device_rows_equal_host_rows(ctx):
    """rows=None takes the last row pass where it lies on the device: the same
    table as the exported rows uploaded again, and the committed expectation."""
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
    with pytest.raises(PangenomeError, match=r"pg_freq failed \(-22\)"):
        ctx.freq(rec_group[:7], 8)                       # not the context's record count
    ref, text = check_device(ctx, rows, rec_group, 8, rows_on_device=True)
    assert check_device(ctx, rows, rec_group, 8)[1] == text
    want = golden("pan8_k27_c3_w4")
    assert (len(ref["labels"]), sum(ref["rows"])) == (want["n_labels"], want["n_rows"]) == (909, 2945)
    for k in ("spectrum_labels", "spectrum_bp") + GROUP_COLS:
        assert ref[k] == want[k], k


# ------------------------------------------------------------ whole pipeline
def _run(km, d, fasta, extra):
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    km.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def _fr_files(q):
    return sorted(f for f in os.listdir(os.path.dirname(q)) if "_fr_" in f)


def test_cli(km, tmp_path):
    from pangenome_amd import host
    fx = Fixture("pan8_k27_c3")
    names = fasta_names(fx.fasta)
    ids = [n.split()[0] for n in names]
    q0, plain = _run(km, tmp_path / "plain", fx.fasta, [])
    assert _fr_files(q0) == []                           # without -g: nothing new
    q, lines = _run(km, tmp_path / "record", fx.fasta, ["-g", "record"])
    assert lines == plain                                # stdout (but the stage timings) is unchanged
    for suffix in ("_rdbg_weight.xyz", "_rdbg_weight.xyz.mcl"):
        assert open(q + suffix, "rb").read() == open(q0 + suffix, "rb").read()
    rows = rows5_of(rows_of("\n".join(lines)), names)
    assert rows.shape[0] == 2945
    ref8 = reference_freq(rows, list(range(8)), 8)
    assert_files(q, ref8, ids)
    assert len(_fr_files(q)) == 4
    # a group file: g0, g1 / g2 .. g5 / g6, g7
    gf = tmp_path / "groups.tsv"
    three = [0, 0, 1, 1, 1, 1, 2, 2]
    gf.write_text("# three genomes\n" + "".join("%s\t%s\n" % (i, "ABC"[g]) for i, g in zip(ids, three)))
    q, lines = _run(km, tmp_path / "file", fx.fasta, ["-g", str(gf)])
    assert lines == plain
    ref3 = reference_freq(rows, three, 3)
    assert_files(q, ref3, ["A", "B", "C"])
    assert sum(ref3["g_bp"]) == sum(ref8["g_bp"]) and sum(ref3["g_rows"]) == 2945
    gf.write_text("".join("%s\tA\n" % i for i in ids[:7]))
    with pytest.raises(ValueError, match=ids[7]):
        _run(km, tmp_path / "missing", fx.fasta, ["-g", str(gf)])
    assert not os.path.exists(str(tmp_path / "missing" / "pan8.fsa_db.npz"))     # raised before the build
    # -n: the row pass walks the first five records only
    g = km.DeviceGraph(q0, 27)
    ns = int(g.seq_len[:5].sum()) - 1
    assert host.plan_rows(g.seq_len, g.shape, g.buf, ns).tolist() == [1, 1, 1, 1, 1, 0, 0, 0]
    g.ctx.close()
    q, lines = _run(km, tmp_path / "five", fx.fasta, ["-g", "record", "-n", str(ns)])
    rows = rows5_of(rows_of("\n".join(lines)), names)
    assert set(rows[:, 0].tolist()) <= set(range(5))
    assert_files(q, reference_freq(rows, [0, 1, 2, 3, 4, -1, -1, -1], 5), ids[:5])
