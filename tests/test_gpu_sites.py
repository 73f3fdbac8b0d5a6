"""The variable sites on the device (pg_region_sites, pangenome_amd/csrc/pg_sites.hip).

Every case compares, exactly, the four returned counts, the three exports
with the presence bits and the text byte for byte with an independent
list-based reference (tests/sites_util.py).  The synthetic shapes are the
smallest at which each mechanism can go wrong: triples that straddle a row
tile (256 rows) in both ways, rows made unused at the tile edge, the word
boundary of the presence bits, keys of more than 64 bits, a site with more
alleles and an allele with more records than a block has threads, and one
label on every other row.
"""
import ctypes as C
import io
import os

import numpy as np
import pytest

from freq_util import fasta_names, rows5_of, rows_of
from golden_util import Fixture
from sites_util import (HEADER, assert_files, assert_same, check_device, device_tables, golden, reference_sites,
                        reference_text, summary)

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


def run_rows(labels, rec=0, strand=1, at=0):
    """One run: a row of length 10 + its label per label (label < 0: an unused row)."""
    return [[rec, at + 100 * i, at + 100 * i + 10 + max(int(l), 0) % 50, strand, int(l)] for i, l in enumerate(labels)]


# ------------------------------------------------------------ 1. empty and tiny
def test_empty(ctx):
    for grp, G in ((np.zeros(0, np.int32), 0), (np.array([0, 1, 0], np.int32), 2)):
        ref, text = check_device(ctx, np.zeros((0, 5), np.int64), grp, G)
        assert text == HEADER.encode() and ref["n_records"] == 0
        assert ctx.region_sites_groups()["genome_sites"].tolist() == [0] * G


def test_tiny(ctx):
    for labels in ([5], [5, 6], [5, 6, 7]):
        ref, text = check_device(ctx, run_rows(labels, rec=1), [-1, 0], 1)
        assert text == HEADER.encode() and ref["n_records"] == max(0, 2 * len(labels) - 3)
    ref, text = check_device(ctx, run_rows([1, 4, 3]) + run_rows([1, 3], rec=1), [0, 1], 2)
    assert text == (HEADER + "1\t3\t*\t1\t1\t0\t0\n1\t3\t4\t1\t1\t14\t14\n").encode()
    ref, text = check_device(ctx, run_rows([1, 4, 3]) + run_rows([1, 9, 3], rec=1) + run_rows([3, 4, 1], rec=1, strand=-1),
                             [0, 1], 2)
    assert text == (HEADER + "1\t3\t4\t1\t1\t14\t14\n1\t3\t9\t1\t1\t19\t19\n").encode()
    ref, text = check_device(ctx, run_rows([6, 2, 6]) + run_rows([6, 6], rec=1) + run_rows([6, 6, 6], rec=2), [0, 1, 1], 2)
    assert ref["site_count"] == [5] and ref["allele_via"] == [-1, 2, 6] and ref["bits"] == [[2], [1], [2]]
    # an unused row splits a run, by its label and by its record
    ref, text = check_device(ctx, run_rows([1, -1, 4, 3]) + run_rows([1, 3], rec=1), [0, 1], 2)
    assert text == HEADER.encode() and ref["n_skipped"] == 1
    rows = run_rows([1, 4]) + run_rows([7], rec=2) + run_rows([3]) + run_rows([1, 3], rec=1)
    ref, text = check_device(ctx, rows, [0, 1, -1], 2)
    assert text == HEADER.encode() and ref["n_skipped"] == 1
    # the same allele twice in one genome: count 2, genomes 1
    ref, text = check_device(ctx, run_rows([1, 4, 3, 1, 4, 3]) + run_rows([1, 3], rec=1), [0, 1], 2)
    assert text == (HEADER + "1\t3\t*\t1\t1\t0\t0\n1\t3\t4\t2\t1\t14\t14\n").encode()


# ------------------------------------------------------------ 2. tile edges
def edge_rows(seed):
    """600 rows: rows 250 .. 520 are one run of record 0 with labels from an
    alphabet of 6 - its triples (254, 255, 256) and (255, 256, 257), and
    (510, 511, 512) and (511, 512, 513), straddle the two tile edges - the rows
    before it are unused, the rows after it a run of record 1."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 6, 600)
    lab[:250] = -1
    rec = np.where(np.arange(600) > 520, 1, 0)
    rows = np.stack([rec, np.arange(600) * 7, np.arange(600) * 7 + rng.integers(0, 40, 600), np.ones(600, np.int64), lab],
                    axis=1).astype(np.int64)
    return rows


@pytest.mark.parametrize("unused", [None, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE])
def test_tile_edges(ctx, unused):
    rows = edge_rows(17)
    if unused is not None:
        rows[unused, 4] = -1
    ref, _ = check_device(ctx, rows, [0, 1], 2)
    n_run0 = 271 if unused is None else 270
    # record 0: 271 rows in one run, or 270 in two; record 1: 79 rows in one run
    assert ref["n_records"] == (2 * n_run0 - 3 - (0 if unused is None else 3)) + (2 * 79 - 3)
    assert len(ref["site_from"]) >= 20 and max(ref["site_alleles"]) >= 4
    # the triple over the edge is there: with it dropped from the rows the tables differ
    if unused is None:
        for edge in (TILE, 2 * TILE):
            for first in (edge - 2, edge - 1):
                a, x, c = rows[first:first + 3, 4].tolist()
                s = [i for i, (f, t) in enumerate(zip(ref["site_from"], ref["site_to"])) if (f, t) == (a, c)]
                assert s and x in ref["allele_via"][ref["site_first"][s[0]]:ref["site_first"][s[0]] + ref["site_alleles"][s[0]]]


# ------------------------------------------------------------ 3. random rows
def random_rows(seed, n=20_000, alphabet=40, n_records=150):
    """Runs of 1 to 5 rows plus three of n / 10 (2,000 of 20,000), each on a
    random record and strand; 10 % of the rows unused (a label of -1)."""
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < n - 3 * (n // 10):
        lens.append(int(rng.integers(1, 6)))
    lens += [n // 10] * 3
    lens = [lens[i] for i in rng.permutation(len(lens))]                 # (their sum is n or a little more)
    rec = np.repeat(rng.integers(0, n_records, len(lens)), lens)[:n]
    strand = np.repeat(rng.choice([1, -1], len(lens)), lens)[:n]
    start = rng.integers(0, 10 ** 7, n)
    rows = np.stack([rec, start, start + rng.integers(-300, 3000, n), strand, rng.integers(0, alphabet, n)],
                    axis=1).astype(np.int64)
    rows[rng.random(n) < 0.1, 4] = -1
    return rows


@pytest.mark.parametrize("G", [1, 2, 64, 65, 130])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random(ctx, seed, G):
    rows = random_rows(seed)
    rng = np.random.default_rng(100 + seed)
    rec_group = rng.permutation(np.arange(150) % G).astype(np.int32)
    rec_group[rng.integers(0, 150, 3)] = -1
    ref, _ = check_device(ctx, rows, rec_group, G)
    assert len(ref["site_from"]) > 1000 and ref["n_skipped"] > 1500 and max(ref["site_alleles"]) > 10
    assert max(ref["site_genomes"]) >= min(G, 10) and (G == 1 or sum(ref["genome_private"]) > 100)
    assert G < 65 or any(b[1] for b in ref["bits"])     # a genome past the first word


def test_poisoned_buffers():
    """Every new device buffer is filled with 0xA5 first: a kernel that read
    memory nothing wrote would show as a different result."""
    from pangenome_amd._lib import PG_TUNE_POISON, Context
    c = Context(27, 0)
    try:
        c.tune(PG_TUNE_POISON, 0xA5)
        rec_group = (np.arange(150) % 65).astype(np.int32)
        check_device(c, random_rows(4), rec_group, 65)
        check_device(c, random_rows(5, n=700), rec_group, 65)        # smaller: the context's scratch is reused
    finally:
        c.tune(PG_TUNE_POISON, -1)
        c.close()


def test_more_genomes_than_one_pass_counts(ctx):
    """2,100 genomes: the per-genome sums take two passes of 2,048 genomes."""
    rows = random_rows(8, n=5000, alphabet=5, n_records=2100)
    rec_group = np.random.default_rng(8).permutation(2100).astype(np.int32)
    ref, _ = check_device(ctx, rows, rec_group, 2100)
    assert len(ref["site_from"]) == 25 and sum(ref["genome_sites"][2048:]) > 20 and len(ref["bits"][0]) == 33


# ------------------------------------------------------------ 4. wide keys
WIDE = [0, 1, 2 ** 31 - 3, 2 ** 31 - 2, 2 ** 31 - 1]


def test_wide_keys(ctx):
    """Labels up to 2^31 - 1 and 300 genomes: a site takes 62 bits, via + 1
    32 and the genome 9.  Nothing may be allocated by the label: the call
    runs under a device cap of 1,000 bytes per row beyond what is held."""
    from pangenome_amd._lib import PG_TUNE_DEVICE_CAP, PangenomeError
    rng = np.random.default_rng(9)
    n = 6000
    rows = random_rows(9, n=n, n_records=300)
    rows[:, 4] = np.where(rows[:, 4] < 0, -1, np.array(WIDE)[rng.integers(0, 5, n)])
    rec_group = rng.permutation(300).astype(np.int32)
    ctx.region_sites([0], 1, rows=run_rows([1, 2]))      # (the context's scratch is warm)
    held = int(ctx.lib.pg_device_bytes(0))
    ctx.tune(PG_TUNE_DEVICE_CAP, held + 1000 * n + (1 << 20))
    try:
        ref, text = check_device(ctx, rows, rec_group, 300)
        peak = int(ctx.lib.pg_device_bytes(1))
    finally:
        ctx.tune(PG_TUNE_DEVICE_CAP, 0)
    assert peak <= held + 1000 * n + (1 << 20)
    assert max(ref["allele_via"]) == 2 ** 31 - 1 and max(ref["site_from"]) == 2 ** 31 - 1
    assert len(ref["bits"][0]) == 5 and max(ref["allele_genomes"]) > 64 and len(ref["site_from"]) == 25
    # a label of 2^31: PG_ERANGE, and the previous result stays
    big = rows.copy()
    big[np.flatnonzero(big[:, 4] >= 0)[0], 4] = 2 ** 31
    with pytest.raises(PangenomeError, match=r"pg_region_sites failed \(-34\)"):
        ctx.region_sites(rec_group, 300, rows=big)
    assert ctx.region_sites_text() == text
    assert_same(device_tables(ctx), ref, 300)


# ------------------------------------------------------------ 5. one long site, one long allele
def test_one_long_site(ctx):
    """The site (1, 2) has 3,000 alleles - more than a block has threads - and
    its allele via 7 has 5,000 records over 70 genomes."""
    rows, rec = [], 0
    for x in list(range(10, 3010)) + [7] * 5000:
        rows += [[rec % 140, 3 * len(rows), 3 * len(rows) + 1 + (len(rows) * 7919) % 1000, 1 if rec % 280 < 140 else -1, l]
                 for l in (1, x, 2)]
        rec += 1
    rows = np.array(rows, np.int64)
    rec_group = (np.arange(140) % 70).astype(np.int32)
    ref, _ = check_device(ctx, rows, rec_group, 70)
    i = [k for k, (a, c) in enumerate(zip(ref["site_from"], ref["site_to"])) if (a, c) == (1, 2)][0]
    assert ref["site_alleles"][i] == 3001 and ref["site_count"][i] == 8000 and ref["site_genomes"][i] == 70
    j = ref["site_first"][i] + ref["allele_via"][ref["site_first"][i]:].index(7)
    assert ref["allele_count"][j] == 5000 and ref["allele_genomes"][j] == 70
    assert ref["allele_min"][j] < 10 and ref["allele_max"][j] > 990


# ------------------------------------------------------------ 6. one dominant label
def test_one_dominant_label(ctx):
    """Label 0 on every other row of 10,000 rows (A b A c A d ...): most
    records share a flank, and (0, 0) is one site with an allele per small label."""
    n = 10_000
    rng = np.random.default_rng(12)
    lab = np.where(np.arange(n) % 2 == 0, 0, 1 + rng.integers(0, 60, n))
    rec = np.sort(rng.integers(0, 40, n))
    rows = np.stack([rec, np.arange(n) * 5, np.arange(n) * 5 + rng.integers(1, 400, n), np.ones(n, np.int64), lab],
                    axis=1).astype(np.int64)
    ref, _ = check_device(ctx, rows, (np.arange(40) % 33).astype(np.int32), 33)
    i = [k for k, (a, c) in enumerate(zip(ref["site_from"], ref["site_to"])) if (a, c) == (0, 0)][0]
    assert ref["site_alleles"][i] == 60 and ref["site_count"][i] > 4900 and ref["site_genomes"][i] == 33


# ------------------------------------------------------------ 7. the pipeline
def test_device_rows_equal_host_rows(ctx):
    """rows=None takes the last row pass where it lies on the device: the same
    result as the exported rows uploaded again, the reference's, and the
    committed expectation."""
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
    ref, text = check_device(ctx, rows, rec_group, 8, rows_on_device=True)
    assert check_device(ctx, rows, rec_group, 8)[1] == text
    want = golden("pan8_k27_c3_w4")
    got = summary(ref)
    assert {k: want[k] for k in got} == got
    assert (got["n_paths"], got["n_pairs"], got["n_sites"], got["n_alleles"]) == (16, 3725, 625, 1342)
    # the other row passes and the sites do not touch each other
    names = [x.split()[0].encode() for x in fasta_names(fx.fasta)]
    ctx.freq(rec_group, 8)
    ctx.region_graph(rec_group, 8)
    ctx.region_seqs(rec_group, 8)
    other = (ctx.freq_text(), ctx.region_links_text(), ctx.region_gfa_text(names), ctx.region_fasta_text(names))
    assert ctx.region_sites_text() == text
    assert_same(device_tables(ctx), ref, 8)
    ctx.region_sites(rec_group[::-1].copy(), 8)
    assert other == (ctx.freq_text(), ctx.region_links_text(), ctx.region_gfa_text(names), ctx.region_fasta_text(names))
    ctx.region_sites(rec_group, 8)
    assert ctx.region_sites_text() == text


def _run(km, d, fasta, extra):
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    km.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4"] + extra, out=out)
    return q, out.getvalue(), [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def test_cli(km, tmp_path):
    fx = Fixture("pan8_k27_c3")
    names = fasta_names(fx.fasta)
    ids = [n.split()[0] for n in names]
    q0, _, plain = _run(km, tmp_path / "plain", fx.fasta, ["-g", "record"])
    q1, _, off = _run(km, tmp_path / "off", fx.fasta, ["-g", "record", "-v", "0"])
    # -v 0: the same files and the same output (but the stage timings) as without the flag
    assert sorted(os.listdir(os.path.dirname(q1))) == sorted(os.listdir(os.path.dirname(q0))) and off == plain
    for f in os.listdir(os.path.dirname(q0)):
        if not f.endswith(".npz"):                       # (a zip: its members carry a time)
            assert open(os.path.join(os.path.dirname(q1), f), "rb").read() == \
                open(os.path.join(os.path.dirname(q0), f), "rb").read(), f
    q, _, lines = _run(km, tmp_path / "sites", fx.fasta, ["-g", "record", "-v", "1"])
    assert lines == plain
    new = sorted(set(os.listdir(os.path.dirname(q))) - set(os.listdir(os.path.dirname(q0))))
    assert new == ["pan8.fsa_fr_sites.npz", "pan8.fsa_fr_sites.tsv", "pan8.fsa_fr_sites_genomes.tsv"]
    rows = rows5_of(rows_of("\n".join(lines)), names)
    assert rows.shape[0] == 2945
    ref = reference_sites(rows, list(range(8)), 8)
    assert_files(q, ref, ids)
    assert summary(ref)["n_sites"] == 625
    # refused before anything is built
    for i, extra in enumerate((["-v", "1"], ["-g", "record", "-v", "2"])):
        d = tmp_path / ("bad%d" % i)
        with pytest.raises(SystemExit):
            _run(km, d, fx.fasta, extra)
        assert os.listdir(str(d)) == ["pan8.fsa"]


# ------------------------------------------------------------ 8. refusals
def test_argument_errors(ctx, tmp_path):
    """Refused before any launch: no device fault is involved."""
    from pangenome_amd._lib import Context, PangenomeError, ptr
    rows = random_rows(6, n=500, alphabet=8, n_records=9)
    rec_group = (np.arange(9) % 4).astype(np.int32)
    ref, text = check_device(ctx, rows, rec_group, 4)
    ns, na = len(ref["site_from"]), len(ref["allele_via"])
    assert ns > 5
    n = C.c_uint64()
    lib, r5, g = ctx.lib, np.ascontiguousarray(rows), np.ascontiguousarray(rec_group)

    def sites(h, r, nr, grp, nrec, G):
        return lib.pg_region_sites(h, r, nr, grp, nrec, G, None, None, None, None)
    assert sites(None, ptr(r5), 500, ptr(g), 9, 4) == -22
    assert sites(ctx.h, ptr(r5), 500, None, 9, 4) == -22
    for bad in (4, -2):
        g2 = g.copy()
        g2[3] = bad
        assert sites(ctx.h, ptr(r5), 500, ptr(g2), 9, 4) == -22
    assert sites(ctx.h, ptr(r5), 500, ptr(g), 8, 4) == -22               # a row names record 8
    r2 = r5.copy()
    r2[17, 0] = -1
    assert sites(ctx.h, ptr(r2), 500, ptr(g), 9, 4) == -22
    assert sites(ctx.h, ptr(r5), 500, ptr(np.full(9, -1, np.int32)), 9, 0) == -22
    fresh = Context(27, 0)
    try:
        assert sites(fresh.h, None, 0, ptr(g), 9, 4) == -22              # no row pass yet
        for call in (fresh.region_sites_table, fresh.region_sites_alleles, fresh.region_sites_groups,
                     fresh.region_sites_text, lambda: fresh.region_sites_write(1)):
            with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
                call()
    finally:
        fresh.close()
    # every refusal left the previous result in place
    assert ctx.region_sites_text() == text
    assert_same(device_tables(ctx), ref, 4)
    # the size query, a short cap, the _fd form
    assert lib.pg_region_sites_format(ctx.h, None, 0, C.byref(n)) == 0 and n.value == len(text)
    buf = np.empty(len(text), np.uint8)
    assert lib.pg_region_sites_format(ctx.h, ptr(buf), len(text) - 1, C.byref(n)) == -34
    assert lib.pg_region_sites_format(ctx.h, ptr(buf), len(text), C.byref(n)) == 0 and buf.tobytes() == text
    assert lib.pg_region_sites_format(ctx.h, ptr(buf), len(text), None) == -22
    assert lib.pg_region_sites_format_fd(ctx.h, -1, C.byref(n)) == -22
    fn = tmp_path / "sites.tsv"
    with open(fn, "wb") as f:
        assert ctx.region_sites_write(f.fileno()) == len(text)
    assert fn.read_bytes() == text
    a = np.empty(max(ns, na), np.int64)
    w = np.empty(4, np.uint64)
    assert lib.pg_region_sites_table(ctx.h, ptr(a), None, None, None, None, None, ns - 1) == -34
    assert lib.pg_region_sites_table(ctx.h, None, ptr(a), None, None, None, None, ns) == 0
    assert a[:ns].tolist() == ref["site_to"]
    assert lib.pg_region_sites_alleles(ctx.h, None, ptr(a), None, None, None, None, None, na - 1) == -34
    assert lib.pg_region_sites_alleles(ctx.h, None, ptr(a), None, None, None, None, None, na) == 0
    assert a[:na].tolist() == ref["allele_via"]
    assert lib.pg_region_sites_groups(ctx.h, None, None, ptr(w), 3) == -34
    assert lib.pg_region_sites_groups(ctx.h, None, None, ptr(w), 4) == 0 and w.tolist() == ref["genome_private"]


def test_independent_of_the_other_row_passes(ctx):
    """pg_freq, pg_region_graph and pg_region_seqs before or after change
    nothing in the sites, and the sites call nothing in theirs (host rows; the
    sequences need the context's parse: test_device_rows_equal_host_rows)."""
    rows = random_rows(7, n=3000, alphabet=12, n_records=20)
    rec_group = (np.arange(20) % 5).astype(np.int32)
    names = [b"r%d" % i for i in range(20)]
    ctx.freq(rec_group, 5, rows=rows)
    ctx.region_graph(rec_group, 5, rows=rows)
    other = (ctx.freq_text(), ctx.region_links_text(), ctx.region_gfa_text(names))
    ref, text = check_device(ctx, rows, rec_group, 5)
    assert other == (ctx.freq_text(), ctx.region_links_text(), ctx.region_gfa_text(names))
    ctx.freq(rec_group[::-1].copy(), 5, rows=rows[:100])
    ctx.region_graph(rec_group[::-1].copy(), 5, rows=rows[:100])
    assert ctx.region_sites_text() == text
    assert_same(device_tables(ctx), ref, 5)
