"""The variable sites between anchors on the device (pg_region_bubbles,
pangenome_amd/csrc/pg_bubbles.hip).

Every case compares, exactly, the five returned counts, the five exports with
the presence bits and the inner paths, and the text byte for byte with an
independent list-based reference (tests/bubbles_util.py).  The synthetic
shapes are the smallest at which each mechanism can go wrong: anchors on both
sides of a row tile's edge (256 rows) and a segment over a whole tile, rows
made unused at the edge, the word boundary of the presence bits, a segment
longer than a block and than a scan tile, a site with more alleles and an
allele with more segments than a block has threads, one label on every other
row, labels up to 2^31 - 1 under a device cap, and a hash narrowed to one bit.
"""
import ctypes as C
import io
import os

import numpy as np
import pytest

from bubbles_util import (HEADER, assert_files, assert_same, check_device, device_tables, golden, inner_of,
                          reference_bubbles, summary)
from freq_util import fasta_names, rows5_of, rows_of
from golden_util import Fixture

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
    """One run: a row of length 10 + its label % 50 per label (label < 0: an unused row)."""
    return [[rec, at + 100 * i, at + 100 * i + 10 + max(int(l), 0) % 50, strand, int(l)] for i, l in enumerate(labels)]


def site_of(ref, a, c):
    return [i for i, ac in enumerate(zip(ref["site_from"], ref["site_to"])) if ac == (a, c)][0]


# ------------------------------------------------------------ 1. empty and tiny
def test_empty(ctx):
    for grp, G, m in ((np.zeros(0, np.int32), 0, 1), (np.zeros(0, np.int32), 0, 7), (np.array([0, 1, 0], np.int32), 2, 2)):
        ref, text = check_device(ctx, np.zeros((0, 5), np.int64), grp, G, m)
        assert text == HEADER.encode() and ref["n_segments"] == 0 and ref["n_anchors"] == 0
        assert ctx.region_bubbles_groups()["genome_sites"].tolist() == [0] * G


def test_tiny(ctx):
    # a run without an anchor; with one anchor; two adjacent anchors
    for rows, anchors, segs in ((run_rows([5, 6, 7]) + run_rows([8], rec=1), [], 0),
                                (run_rows([5, 6, 7]) + run_rows([6], rec=1), [6], 0),
                                (run_rows([5, 6, 7]) + run_rows([6, 7], rec=1), [6, 7], 2)):
        ref, text = check_device(ctx, rows, [0, 1], 2, 2)
        assert text == HEADER.encode() and ref["anchors"] == anchors and ref["n_segments"] == segs
    # two regions against the direct join; by first row the long allele comes first
    ref, text = check_device(ctx, run_rows([1, 4, 5, 3]) + run_rows([1, 3], rec=1), [0, 1], 2, 2)
    assert text == (HEADER + "1\t3\t4,5\t2\t1\t1\t29\t29\n1\t3\t*\t0\t1\t1\t0\t0\n").encode()
    # a == c, and the same allele twice in one genome: count 2, genomes 1
    ref, text = check_device(ctx, run_rows([6, 2, 6, 2, 6]) + run_rows([6, 6], rec=1), [0, 1], 2, 2)
    assert text == (HEADER + "6\t6\t2\t1\t2\t1\t12\t12\n6\t6\t*\t0\t1\t1\t0\t0\n").encode()
    # an unused row inside a would-be segment ends the run, by its label and by its record: no segment there
    ref, text = check_device(ctx, run_rows([1, 4, -1, 3]) + run_rows([1, 3], rec=1), [0, 1], 2, 2)
    assert text == HEADER.encode() and ref["n_skipped"] == 1 and ref["n_segments"] == 1
    rows = run_rows([1, 4]) + run_rows([7], rec=2) + run_rows([3]) + run_rows([1, 3], rec=1)
    ref, text = check_device(ctx, rows, [0, 1, -1], 2, 2)
    assert text == HEADER.encode() and ref["n_skipped"] == 1 and ref["n_segments"] == 1
    # a run head directly after an anchor: the other strand, the other record
    rows = run_rows([1]) + run_rows([3], strand=-1) + run_rows([1], rec=1) + run_rows([3, 9, 1], rec=2)
    ref, text = check_device(ctx, rows, [0, 1, 1], 2, 2)
    assert text == HEADER.encode() and ref["anchors"] == [1, 3] and ref["n_segments"] == 1 and ref["n_runs"] == 4


def test_identity(ctx):
    """In one site [x, y] against [y, x], [x] against [x, y], and paths that
    differ in the first label only and in the last only."""
    rows = (run_rows([1, 4, 5, 3]) + run_rows([1, 5, 4, 3], rec=1) + run_rows([1, 4, 3], rec=2) +
            run_rows([1, 6, 5, 3], rec=3) + run_rows([1, 4, 6, 3], rec=4) + run_rows([1, 4, 5, 3], rec=5))
    ref, _ = check_device(ctx, rows, [0, 1, 2, 3, 4, 0], 5, 5)
    assert [inner_of(ref, i) for i in range(5)] == [[4, 5], [5, 4], [4], [6, 5], [4, 6]]
    assert ref["allele_count"] == [2, 1, 1, 1, 1] and ref["allele_first_row"] == [0, 4, 8, 11, 15]


# ------------------------------------------------------------ 2. tile edges
def edge_rows(seed):
    """600 rows: record 0 is one run of 594 rows with the anchor 1 at rows 100,
    255, 512 and 580 and the anchor 2 at rows 256 and 511 - two anchors on
    either side of both tile edges, the segment 256 .. 511 over a whole tile -
    and labels of genome 0 alone elsewhere; record 1 (genome 1) joins the
    same flanks its own way."""
    rng = np.random.default_rng(seed)
    lab = 10 + rng.integers(0, 6, 594)
    lab[[100, TILE - 1, 2 * TILE, 580]] = 1
    lab[[TILE, 2 * TILE - 1]] = 2
    lab = np.concatenate([lab, [1, 20, 2, 2, 1, 1]])
    rec = np.where(np.arange(600) >= 594, 1, 0)
    return np.stack([rec, np.arange(600) * 7, np.arange(600) * 7 + rng.integers(0, 40, 600), np.ones(600, np.int64), lab],
                    axis=1).astype(np.int64)


@pytest.mark.parametrize("unused", [None, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE])
def test_tile_edges(ctx, unused):
    rows = edge_rows(17)
    if unused is not None:
        rows[unused, 4] = -1
    ref, _ = check_device(ctx, rows, [0, 1], 2, 2)
    assert ref["anchors"] == [1, 2] and ref["n_segments"] == (9 if unused is None else 7)
    got = {(a, c): n for a, c, n in zip(ref["site_from"], ref["site_to"], ref["site_alleles"])}
    if unused is None:
        # (1, 2): 255 -> 256 directly against [20]; (2, 2): the 254 rows of the whole tile against the direct
        # join; (1, 1): two long paths against the direct join; (2, 1): directly in both genomes - no site
        assert got == {(1, 1): 3, (1, 2): 2, (2, 2): 2}
        i = site_of(ref, 2, 2)
        assert ref["allele_regions"][ref["site_first"][i]] == 254 and ref["allele_first_row"][ref["site_first"][i]] == TILE
    else:
        # the run is cut at the unused anchor: the segments on either side of it are gone
        assert got == {TILE - 1: {(1, 1): 2, (2, 2): 2}, TILE: {(1, 1): 3}, 2 * TILE - 1: {(1, 1): 3, (1, 2): 2},
                       2 * TILE: {(1, 1): 2, (1, 2): 2, (2, 2): 2}}[unused]


# ------------------------------------------------------------ 3. random rows
def random_rows(seed, rec_group, G, n=20_000, alphabet=40, n_records=150):
    """Runs of 1 to 5 rows plus three of n / 10 (2,000 of 20,000), each on a
    random record and strand; 10 % of the rows unused (a label of -1).  The
    labels from 30 up stay in one genome each and those from 20 to 29 in every
    third genome, so that not every label is an anchor."""
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < n - 3 * (n // 10):
        lens.append(int(rng.integers(1, 6)))
    lens += [n // 10] * 3
    lens = [lens[i] for i in rng.permutation(len(lens))]                 # (their sum is n or a little more)
    rec = np.repeat(rng.integers(0, n_records, len(lens)), lens)[:n]
    strand = np.repeat(rng.choice([1, -1], len(lens)), lens)[:n]
    start = rng.integers(0, 10 ** 7, n)
    lab = rng.integers(0, alphabet, n)
    g = np.asarray(rec_group)[rec]
    lab = np.where((lab >= 30) & (g != (lab - 30) % max(G, 1)), lab - 30, lab)
    lab = np.where((lab >= 20) & (lab < 30) & (g % 3 != 0), lab - 20, lab)
    rows = np.stack([rec, start, start + rng.integers(-300, 3000, n), strand, lab], axis=1).astype(np.int64)
    rows[rng.random(n) < 0.1, 4] = -1
    return rows


@pytest.fixture(scope="module")
def random_case():
    made = {}

    def make(G):
        if G not in made:
            rng = np.random.default_rng(100 + G)
            # (every genome has a record; the last three records have none)
            rec_group = np.concatenate([rng.permutation(np.arange(150) % G), [-1, -1, -1]]).astype(np.int32)
            made[G] = (random_rows(G, rec_group, G, n_records=153), rec_group)
        return made[G]
    return make


@pytest.mark.parametrize("G", [2, 65, 130])
@pytest.mark.parametrize("m", ["1", "2", "G"])
def test_random(ctx, random_case, G, m):
    rows, rec_group = random_case(G)
    m = G if m == "G" else int(m)
    ref, _ = check_device(ctx, rows, rec_group, G, m)
    assert ref["n_skipped"] > 1500 and ref["n_segments"] > 1000
    if m == 1:
        # every label is an anchor: every segment is a direct join, every pair has one allele, and the
        # segments are the region graph's links
        ctx.region_graph(rec_group, G, rows=rows)
        assert ref["n_segments"] == int(ctx.region_links()["link_count"].sum()) and ref["n_sites"] == 0
    else:
        # (with 65 genomes or more and min_genomes 2 only a label of one genome is no anchor: few sites)
        assert ref["n_sites"] > 5 and sum(ref["genome_private"]) > 5 and max(ref["site_genomes"]) >= min(G, 10)
        if m == G:
            assert ref["n_alleles"] > 500 and max(ref["site_alleles"]) >= 4 and max(ref["allele_regions"]) >= 4
        assert G < 65 or any(b[1] for b in ref["bits"])  # a genome past the first word


def test_poisoned_buffers(ctx, random_case):
    """Every new device buffer is filled with 0xA5 first: a kernel that read
    memory nothing wrote would show as a different result from the
    unpoisoned run's."""
    from pangenome_amd._lib import PG_TUNE_POISON, Context
    rows, rec_group = random_case(65)
    _, text = check_device(ctx, rows, rec_group, 65, 2)
    c = Context(27, 0)
    try:
        c.tune(PG_TUNE_POISON, 0xA5)
        assert check_device(c, rows, rec_group, 65, 2)[1] == text
        check_device(c, rows[:700], rec_group, 65, 2)                # smaller: the context's scratch is reused
    finally:
        c.tune(PG_TUNE_POISON, -1)
        c.close()


# ------------------------------------------------------------ 4. wide labels
WIDE = [0, 1, 2 ** 31 - 3, 2 ** 31 - 2, 2 ** 31 - 1]


def test_wide_labels(ctx):
    """Labels up to 2^31 - 1 and 300 genomes.  Nothing may be allocated by the
    label: the call runs under a device cap of 1,000 bytes per row beyond what
    is held."""
    from pangenome_amd._lib import PG_TUNE_DEVICE_CAP, PangenomeError
    rng = np.random.default_rng(9)
    n = 6000
    rec_group = rng.permutation(300).astype(np.int32)
    rows = random_rows(9, rec_group, 300, n=n, n_records=300)
    # 0 and 2^31 - 1 everywhere, the three between them in the genomes below 20 alone
    lab = np.array(WIDE)[rng.integers(0, 5, n)]
    ends = np.array([0, 2 ** 31 - 1])[rng.integers(0, 2, n)]
    lab = np.where(rec_group[rows[:, 0]] < 20, lab, np.where((lab == 0) | (lab == 2 ** 31 - 1), lab, ends))
    rows[:, 4] = np.where(rows[:, 4] < 0, -1, lab)
    ctx.region_bubbles([0], 1, 1, rows=run_rows([1, 2]))              # (the context's scratch is warm)
    held = int(ctx.lib.pg_device_bytes(0))
    ctx.tune(PG_TUNE_DEVICE_CAP, held + 1000 * n + (1 << 20))
    try:
        ref, text = check_device(ctx, rows, rec_group, 300, 100)
        peak = int(ctx.lib.pg_device_bytes(1))
    finally:
        ctx.tune(PG_TUNE_DEVICE_CAP, 0)
    assert peak <= held + 1000 * n + (1 << 20)
    assert ref["anchors"] == [0, 2 ** 31 - 1] and sorted(set(ref["inner"])) == WIDE[1:4]
    assert len(ref["site_from"]) == 4 and len(ref["bits"][0]) == 5 and max(ref["allele_genomes"]) > 64
    # a label of 2^31: PG_ERANGE, and the previous result stays
    big = rows.copy()
    big[np.flatnonzero(big[:, 4] >= 0)[0], 4] = 2 ** 31
    with pytest.raises(PangenomeError, match=r"pg_region_bubbles failed \(-34\)"):
        ctx.region_bubbles(rec_group, 300, 100, rows=big)
    assert ctx.region_bubbles_text() == text
    assert_same(device_tables(ctx), ref, 300)


# ------------------------------------------------------------ 5. one long segment, one wide site
def test_one_long_segment(ctx):
    """A run of 5,000 rows with anchors at its ends only - longer than a block
    and than any scan tile - in three genomes, one differing in its last inner
    label; two more genomes join the flanks directly."""
    rng = np.random.default_rng(21)
    path = (10 + rng.integers(0, 30, 4998)).tolist()
    other = path[:-1] + [path[-1] + 100]
    rows = []
    for rec, inner in enumerate((path, path, other)):
        rows += run_rows([1] + inner + [2], rec=rec, at=7 * rec)
    rows += run_rows([1, 2], rec=3) + run_rows([1, 2], rec=4)
    ref, text = check_device(ctx, np.array(rows, np.int64), [0, 1, 2, 3, 4], 5, 4)
    assert ref["anchors"] == [1, 2] and ref["n_segments"] == 5
    assert ref["site_alleles"] == [3] and ref["allele_regions"] == [4998, 4998, 0] and ref["allele_count"] == [2, 1, 2]
    assert ref["allele_first_row"] == [0, 10000, 15000] and ref["bits"] == [[3], [4], [24]]
    assert inner_of(ref, 0) == path and inner_of(ref, 1) == other and len(text) > 2 * 4998 * 3


def test_one_wide_site(ctx):
    """The site (1, 2) has 1,501 alleles - more than a block has threads - and
    its allele [7] has 3,000 segments over 30 genomes."""
    rows, t = [], 0
    for x in list(range(10, 1510)) + [7] * 3000:
        rec = t % 140 if x != 7 else t % 30 + (70 if t % 60 >= 30 else 0)
        rows += [[rec, 3 * len(rows), 3 * len(rows) + 1 + (len(rows) * 7919) % 1000, 1 if t % 280 < 140 else -1, l]
                 for l in (1, x, 2)]
        t += 1
    rows = np.array(rows, np.int64)
    rec_group = (np.arange(140) % 70).astype(np.int32)
    ref, _ = check_device(ctx, rows, rec_group, 70, 40)
    assert ref["anchors"] == [1, 2] and ref["n_segments"] == 4500
    i = site_of(ref, 1, 2)
    assert ref["site_alleles"][i] == 1501 and ref["site_count"][i] == 4500 and ref["site_genomes"][i] == 70
    j = ref["site_first"][i] + 1500                      # by first row: the last allele of the site
    assert inner_of(ref, j) == [7] and ref["allele_count"][j] == 3000 and ref["allele_genomes"][j] == 30
    assert ref["allele_min_bp"][j] < 10 and ref["allele_max_bp"][j] > 990


# ------------------------------------------------------------ 6. one dominant label
def test_one_dominant_label(ctx):
    """Label 0 on every other row of 10,000 rows (A b A c A d ...): the anchor
    of most segments; a small label stays in the genomes of its parity, so
    (0, 0) is one site with an allele per small label."""
    n = 10_000
    rng = np.random.default_rng(12)
    rec = np.sort(rng.integers(0, 40, n))
    g = rec % 33
    small = 1 + rng.integers(0, 60, n)
    small += (small % 2 != g % 2)
    lab = np.where(np.arange(n) % 2 == 0, 0, small)
    rows = np.stack([rec, np.arange(n) * 5, np.arange(n) * 5 + rng.integers(1, 400, n), np.ones(n, np.int64), lab],
                    axis=1).astype(np.int64)
    ref, _ = check_device(ctx, rows, (np.arange(40) % 33).astype(np.int32), 33, 33)
    assert ref["anchors"] == [0]
    i = site_of(ref, 0, 0)
    assert ref["site_alleles"][i] == 61 and ref["site_count"][i] > 4900 and ref["site_genomes"][i] == 33


# ------------------------------------------------------------ 7. the hash narrowed to one bit
def test_narrow_hash(ctx):
    """PG_TUNE_BUBBLE_HASH_BITS 1: alleles that differ in regions are still
    told apart exactly; three alleles of equal regions in one pair cannot be
    by two hash values, so the label comparison must refuse the call - an
    error return, with the previous result kept."""
    from pangenome_amd._lib import PG_TUNE_BUBBLE_HASH_BITS, PangenomeError
    flanks = run_rows([1, 3], rec=3) + run_rows([1, 3], rec=4)
    by_length = run_rows([1, 4, 3]) + run_rows([1, 4, 5, 3], rec=1) + run_rows([1, 6, 4, 5, 3], rec=2) + flanks
    same_length = run_rows([1, 4, 3]) + run_rows([1, 5, 3], rec=1) + run_rows([1, 6, 3], rec=2) + flanks
    grp = [0, 1, 2, 3, 4]
    ctx.tune(PG_TUNE_BUBBLE_HASH_BITS, 1)
    try:
        ref, text = check_device(ctx, by_length, grp, 5, 4)
        assert ref["site_alleles"] == [4] and ref["allele_regions"] == [1, 2, 3, 0]
        with pytest.raises(PangenomeError, match=r"pg_region_bubbles failed \(-5\)"):
            ctx.region_bubbles(grp, 5, 4, rows=same_length)
        assert ctx.region_bubbles_text() == text
        assert_same(device_tables(ctx), ref, 5)
    finally:
        ctx.tune(PG_TUNE_BUBBLE_HASH_BITS, 0)
    ref, _ = check_device(ctx, same_length, grp, 5, 4)
    assert ref["site_alleles"] == [4] and ref["allele_regions"] == [1, 1, 1, 0]


# ------------------------------------------------------------ 8. the pipeline
def test_device_rows_equal_host_rows(ctx):
    """rows=None takes the last row pass where it lies on the device: the same
    result as the exported rows uploaded again, the reference's, and the
    committed expectation; the other row passes and the bubbles do not touch
    each other."""
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
    want = golden("pan8_k27_c3_w4")
    for m in (1, 6, 5):
        ref, text = check_device(ctx, rows, rec_group, 8, m, rows_on_device=True)
        assert check_device(ctx, rows, rec_group, 8, m)[1] == text
        assert want["m%d" % m] == summary(ref)
    assert (ref["n_anchors"], ref["n_segments"], ref["n_sites"], ref["n_alleles"]) == (279, 1564, 186, 478)
    names = [x.split()[0].encode() for x in fasta_names(fx.fasta)]
    ctx.freq(rec_group, 8)
    ctx.region_graph(rec_group, 8)
    ctx.region_seqs(rec_group, 8)
    ctx.region_sites(rec_group, 8)

    def others():
        return (ctx.freq_text(), ctx.region_links_text(), ctx.region_gfa_text(names), ctx.region_fasta_text(names),
                ctx.region_sites_text())
    other = others()
    assert ctx.region_bubbles_text() == text
    assert_same(device_tables(ctx), ref, 8)
    ctx.region_bubbles(rec_group[::-1].copy(), 8, 3)
    assert other == others()
    ctx.region_bubbles(rec_group, 8, 5)
    assert ctx.region_bubbles_text() == text


def _run(km, d, fasta, extra):
    os.makedirs(d, exist_ok=True)
    q = os.path.join(str(d), "pan8.fsa")
    open(q, "wb").write(fasta)
    out = io.StringIO()
    km.entry_point(["kmer_numba.py", "-i", q, "-k27", "-c3", "-acc", "-w4"] + extra, out=out)
    return q, [ln for ln in out.getvalue().split("\n") if not ln.startswith("# finished in")]


def test_cli(km, tmp_path):
    fx = Fixture("pan8_k27_c3")
    names = fasta_names(fx.fasta)
    ids = [n.split()[0] for n in names]
    q0, plain = _run(km, tmp_path / "plain", fx.fasta, ["-g", "record"])
    q, lines = _run(km, tmp_path / "bubbles", fx.fasta, ["-g", "record", "-b", "5"])
    # stdout and every other file are those of the run without -b
    assert lines == plain
    new = sorted(set(os.listdir(os.path.dirname(q))) - set(os.listdir(os.path.dirname(q0))))
    assert new == ["pan8.fsa_fr_bubbles.npz", "pan8.fsa_fr_bubbles.tsv", "pan8.fsa_fr_bubbles_genomes.tsv"]
    for f in os.listdir(os.path.dirname(q0)):
        if not f.endswith(".npz"):                       # (a zip: its members carry a time)
            assert open(os.path.join(os.path.dirname(q), f), "rb").read() == \
                open(os.path.join(os.path.dirname(q0), f), "rb").read(), f
    rows = rows5_of(rows_of("\n".join(lines)), names)
    assert rows.shape[0] == 2945
    ref = reference_bubbles(rows, list(range(8)), 8, 5)
    assert_files(q, ref, ids)
    assert golden("pan8_k27_c3_w4")["m5"] == summary(ref) and ref["n_sites"] == 186
    # a value above the number of genomes: in every genome
    q8, _ = _run(km, tmp_path / "all", fx.fasta, ["-g", "record", "-b", "99"])
    assert_files(q8, reference_bubbles(rows, list(range(8)), 8, 8), ids)
    # refused before anything is built
    for i, extra in enumerate((["-b", "5"], ["-g", "record", "-b", "x"])):
        d = tmp_path / ("bad%d" % i)
        with pytest.raises(SystemExit):
            _run(km, d, fx.fasta, extra)
        assert os.listdir(str(d)) == ["pan8.fsa"]


# ------------------------------------------------------------ 9. refusals
def test_argument_errors(ctx, random_case, tmp_path):
    """Refused before any launch: no device fault is involved."""
    from pangenome_amd._lib import Context, PangenomeError, ptr
    rows, rec_group = random_case(2)
    rows, rec_group = rows[:500].copy(), rec_group.copy()
    ref, text = check_device(ctx, rows, rec_group, 2, 2)
    ns, na, nin, nanc = ref["n_sites"], ref["n_alleles"], len(ref["inner"]), ref["n_anchors"]
    assert ns > 5 and nin > 5
    n = C.c_uint64()
    lib, r5, g = ctx.lib, np.ascontiguousarray(rows), np.ascontiguousarray(rec_group)

    def bubbles(h, r, nr, grp, nrec, G, m):
        return lib.pg_region_bubbles(h, r, nr, grp, nrec, G, m, None, None, None, None, None)
    assert bubbles(ctx.h, ptr(r5), 500, ptr(g), 153, 2, 2) == 0          # (every count pointer may be NULL)
    assert bubbles(None, ptr(r5), 500, ptr(g), 153, 2, 2) == -22
    assert bubbles(ctx.h, ptr(r5), 500, ptr(g), 153, 2, 0) == -22        # min_genomes 0
    assert bubbles(ctx.h, ptr(r5), 500, ptr(g), 153, 2, 3) == -22        # min_genomes G + 1
    assert bubbles(ctx.h, ptr(r5), 500, None, 153, 2, 2) == -22          # NULL groups
    assert bubbles(ctx.h, ptr(np.zeros((0, 5), np.int64)), 0, ptr(g), 0, 0, 0) == -22
    g2 = g.copy()
    g2[3] = 2
    assert bubbles(ctx.h, ptr(r5), 500, ptr(g2), 153, 2, 2) == -22
    assert bubbles(ctx.h, ptr(r5), 500, ptr(g), 10, 2, 2) == -22         # a row names a record past 10
    assert bubbles(ctx.h, ptr(r5), 500, ptr(np.full(153, -1, np.int32)), 153, 0, 1) == -22
    fresh = Context(27, 0)
    try:
        assert bubbles(fresh.h, None, 0, ptr(g), 153, 2, 2) == -22       # no row pass yet
        for call in (fresh.region_bubbles_table, fresh.region_bubbles_alleles, fresh.region_bubbles_inner,
                     fresh.region_bubbles_groups, fresh.region_bubbles_anchors, fresh.region_bubbles_text,
                     lambda: fresh.region_bubbles_write(1)):
            with pytest.raises(PangenomeError, match=r"failed \(-22\)"):
                call()
    finally:
        fresh.close()
    # every refusal left the previous result in place
    assert ctx.region_bubbles_text() == text
    assert_same(device_tables(ctx), ref, 2)
    # the size query, a short cap, the _fd form
    assert lib.pg_region_bubbles_format(ctx.h, None, 0, C.byref(n)) == 0 and n.value == len(text)
    buf = np.empty(len(text), np.uint8)
    assert lib.pg_region_bubbles_format(ctx.h, ptr(buf), len(text) - 1, C.byref(n)) == -34
    assert lib.pg_region_bubbles_format(ctx.h, ptr(buf), len(text), C.byref(n)) == 0 and buf.tobytes() == text
    assert lib.pg_region_bubbles_format(ctx.h, ptr(buf), len(text), None) == -22
    assert lib.pg_region_bubbles_format_fd(ctx.h, -1, C.byref(n)) == -22
    fn = tmp_path / "bubbles.tsv"
    with open(fn, "wb") as f:
        assert ctx.region_bubbles_write(f.fileno()) == len(text)
    assert fn.read_bytes() == text
    a = np.empty(max(ns, na, nin, nanc), np.int64)
    w = np.empty(2, np.uint64)
    assert lib.pg_region_bubbles_table(ctx.h, ptr(a), None, None, None, None, None, ns - 1) == -34
    assert lib.pg_region_bubbles_table(ctx.h, None, ptr(a), None, None, None, None, ns) == 0
    assert a[:ns].tolist() == ref["site_to"]
    assert lib.pg_region_bubbles_alleles(ctx.h, None, ptr(a), None, None, None, None, None, None, None, na - 1) == -34
    assert lib.pg_region_bubbles_alleles(ctx.h, None, ptr(a), None, None, None, None, None, None, None, na) == 0
    assert a[:na].tolist() == ref["allele_regions"]
    assert lib.pg_region_bubbles_inner(ctx.h, None, 0, C.byref(n)) == 0 and n.value == nin
    assert lib.pg_region_bubbles_inner(ctx.h, ptr(a), nin - 1, C.byref(n)) == -34
    assert lib.pg_region_bubbles_inner(ctx.h, ptr(a), nin, None) == -22
    assert lib.pg_region_bubbles_inner(ctx.h, ptr(a), nin, C.byref(n)) == 0 and a[:nin].tolist() == ref["inner"]
    assert lib.pg_region_bubbles_anchors(ctx.h, ptr(a), None, nanc - 1) == -34
    assert lib.pg_region_bubbles_anchors(ctx.h, ptr(a), None, nanc) == 0 and a[:nanc].tolist() == ref["anchors"]
    assert lib.pg_region_bubbles_groups(ctx.h, None, None, ptr(w), 1) == -34
    assert lib.pg_region_bubbles_groups(ctx.h, None, None, ptr(w), 2) == 0 and w.tolist() == ref["genome_private"]
    assert ctx.region_bubbles_text() == text


def test_independent_of_the_other_row_passes(ctx, random_case):
    """pg_freq, pg_region_graph and pg_region_sites before or after change
    nothing in the bubbles, and the bubbles call nothing in theirs (host rows;
    the sequences need the context's parse: test_device_rows_equal_host_rows)."""
    rows, rec_group = random_case(65)
    rows = rows[:3000]
    names = [b"r%d" % i for i in range(153)]
    ctx.freq(rec_group, 65, rows=rows)
    ctx.region_graph(rec_group, 65, rows=rows)
    ctx.region_sites(rec_group, 65, rows=rows)

    def others():
        return ctx.freq_text(), ctx.region_links_text(), ctx.region_gfa_text(names), ctx.region_sites_text()
    other = others()
    ref, text = check_device(ctx, rows, rec_group, 65, 2)
    assert other == others()
    ctx.freq(rec_group[::-1].copy(), 65, rows=rows[:100])
    ctx.region_graph(rec_group[::-1].copy(), 65, rows=rows[:100])
    ctx.region_sites(rec_group[::-1].copy(), 65, rows=rows[:100])
    assert ctx.region_bubbles_text() == text
    assert_same(device_tables(ctx), ref, 65)
