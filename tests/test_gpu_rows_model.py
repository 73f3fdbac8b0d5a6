"""pg_region_bubbles, pg_region_variants and pg_region_align on random
pangenome-shaped rows (tests/pangenome_rows_util.py): whole records tiled by
rows, one long run per record with anchor after anchor - every anchor row ends
one segment and starts the next - many sites per run and per contig, alleles
that descend from one another, both strands, N and lower case, one, two and
three presence words; and the grid of cores around the strip and word borders
with letters of low complexity, where the tie rule decides every cell.

Every case compares every export and both texts of the alignment exactly with
the list-based references (align_util.check_align), and the allele FASTA, the
tables and the variants' VCF of the same state with variants_util.assert_same.
tests/test_rows_model_host.py asserts, without a GPU, that these inputs hold
what they are meant to hold."""
import pytest

from align_util import check_align, check_properties, check_vcf, device_state
from pangenome_rows_util import KINDS, SHAPES, assert_floors, lowcx_site, min_genomes_of, shape_input
from seq_util import make_fasta, parse
from test_align_host import site_records
from variants_util import assert_same as variants_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    yield c
    c.close()


def run_shape(c, i, ref_group, min_genomes=None):
    """Shape i parsed and the three passes checked; returns (res, tsv, VCF body, names, sequences)."""
    rows, grp, G, _, _, fasta, _ = shape_input(i)
    names, seqs = parse(c, fasta)
    res, tsv, vcf = check_align(c, rows, grp, G, min_genomes or min_genomes_of(G), names, seqs, ref_group)
    variants_same(c, res["ref"], names, seqs)
    return res, tsv, vcf, names, seqs


# ------------------------------------------------------------ 1. the shapes
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_block_pangenome(ctx, i):
    rows, grp, G, _, _, _, genome = shape_input(i)
    for ref_group in (0, genome, G - 1, None):
        res, _, vcf, names, seqs = run_shape(ctx, i, ref_group)
        check_properties(res)
        if res["n_lines"]:
            check_vcf(res, vcf, names, seqs)
        if ref_group == genome:
            assert_floors(res, vcf, rows, grp)
    for min_genomes in (2, G):                           # few sites, or few and very wide ones
        res, _, vcf, names, seqs = run_shape(ctx, i, 0, min_genomes)
        check_properties(res)
        if res["n_lines"]:
            check_vcf(res, vcf, names, seqs)


# ------------------------------------------------------------ 2. poison
def test_block_pangenome_poisoned(ctx):
    """Two presence words in a fresh context whose every new device buffer is
    filled with 0xA5 first - a read of a word nothing wrote would show - then
    the baseline in the same context, in scratch sized for more."""
    from pangenome_amd._lib import PG_TUNE_POISON, Context
    _, genome = shape_input(1)[-2:]
    want = run_shape(ctx, 1, genome)[1:3]
    c = Context(27, 0)
    try:
        c.tune(PG_TUNE_POISON, 0xA5)
        assert run_shape(c, 1, genome)[1:3] == want
        for ref_group in (shape_input(0)[-1], None):
            run_shape(c, 0, ref_group)
    finally:
        c.tune(PG_TUNE_POISON, -1)
        c.close()


# ------------------------------------------------------------ 3. the batches
def test_block_pangenome_batches(ctx):
    from pangenome_amd._lib import PG_TUNE_ALIGN_SCRATCH
    G, genome = shape_input(2)[2], shape_input(2)[-1]
    res, _, _, names, _ = run_shape(ctx, 2, genome)
    counts = (res["n_pairs"], res["n_aligned"], res["n_ops_all"], res["n_prims_all"], res["n_lines"])
    state = device_state(ctx, names, G)
    try:
        for scratch in (1, 1 << 12):                     # one pair per batch, a few pairs per batch
            ctx.tune(PG_TUNE_ALIGN_SCRATCH, scratch)
            assert ctx.region_align() == counts
            assert device_state(ctx, names, G) == state
    finally:
        ctx.tune(PG_TUNE_ALIGN_SCRATCH, 0)


# ------------------------------------------------------------ 4. low complexity around the borders
@pytest.mark.parametrize("shift", [0, 5, 9, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_lowcx_borders(ctx, kind, shift):
    recs, rows, grp = site_records(lowcx_site(shift, kind, 1))
    names, seqs = parse(ctx, make_fasta(recs))
    for ref_group in (0, None) if shift == 0 else (0,):  # unplaced: T and Q both start at a multiple of 16
        res, _, vcf = check_align(ctx, rows, grp, 3, 2, names, seqs, ref_group)
        assert res["n_pairs"] == 144 == res["n_aligned"]
        assert {p % 16 for p in res["prefix"]} >= {shift}
        check_properties(res)
        check_vcf(res, vcf, names, seqs)
        assert (res["n_lines"] == 0) == (ref_group is None)


# ------------------------------------------------------------ 5. the result depends on the input alone
def test_repeat_run_is_the_same(ctx):
    from pangenome_amd._lib import Context
    G, genome = shape_input(3)[2], shape_input(3)[-1]
    states = []
    for _ in range(2):
        names = run_shape(ctx, 3, genome)[3]
        states.append(device_state(ctx, names, G))
    c = Context(27, 0)
    try:
        names = run_shape(c, 3, genome)[3]
        states.append(device_state(c, names, G))
    finally:
        c.close()
    assert states[0] == states[1] == states[2]
