"""The random pangenome-shaped rows (tests/pangenome_rows_util.py) on the host,
no GPU: the generator pinned, and the conditions that keep the device's cases
(tests/test_gpu_rows_model.py) meaningful asserted through the tests' two
list-based references - per shape the floors of FLOORS (enough sites, alleles
on `-` and with N, placed and unplaced sites, shared lines, every GT cell,
cores longer than a strip, a run of many segments), and per low-complexity
site the full grid of cores and at least 30 pairs of 144 with more than one
optimal script."""
import numpy as np
import pytest

from align_util import (apply_prims, check_properties, check_vcf, matrix, reference_align, reference_primitives_vcf)
from pangenome_rows_util import (BORDERS, KINDS, PAD, REVCOMP, SHAPES, assert_floors, block_pangenome, edited,
                                 lowcx_site, min_genomes_of, shape_input)
from seq_util import fasta_records, make_fasta
from test_align_host import site_records
from variants_util import check_vcf as check_variants_vcf
from variants_util import reference_variants, reference_vcf

TIED_PAIRS = 30                                          # of a low-complexity site's 144


def tied(D, t, u):
    """True iff (t, u) has more than one optimal script: going back from
    (a, b) over D, some cell on the optimal path has two predecessors or more
    that attain its value.  (Up to the first such cell the path is the only
    one, so following it finds the cell if there is one.)"""
    i, j = len(t), len(u)
    while i or j:
        diag = bool(i and j and D[i][j] == D[i - 1][j - 1] + (t[i - 1] != u[j - 1]))
        up = bool(i and D[i][j] == D[i - 1][j] + 1)
        left = bool(j and D[i][j] == D[i][j - 1] + 1)
        if diag + up + left > 1:
            return True
        i, j = (i - 1, j - 1) if diag else (i - 1, j) if up else (i, j - 1)
    return False


def test_tied_counts_scripts():
    for t, u, want in ((b"AAA", b"AA", True), (b"ACG", b"ACG", False), (b"", b"AC", False), (b"ACGT", b"AGT", False),
                       (b"AC", b"CA", True), (b"ACAC", b"AC", True), (b"AG", b"C", True)):
        assert tied(matrix(t, u), t, u) is want, (t, u)


# ------------------------------------------------------------ the generator
def test_generator_is_deterministic_and_tiles_its_records():
    for shape in SHAPES:
        seed, G = shape[:2]
        records, rows, grp = block_pangenome(*shape)
        again = block_pangenome(*shape)
        assert records == again[0] and rows.tolist() == again[1].tolist() and grp == again[2]
        assert block_pangenome(seed + 100, *shape[1:])[0] != records
        assert rows.dtype == np.int64 and rows.shape[1] == 5 and (rows[:, 4] > 0).all()
        assert grp[-1] == -1 and sorted(set(grp[:-1])) == list(range(G)) and len(grp) == len(records)
        alphabet = set(shape[4] + shape[4].translate(REVCOMP))
        alphabet |= set(bytes(alphabet).lower() + b"Nn")
        strands, r = set(), 0
        for rec, body in enumerate(records):             # one run per record, end to end between the pads
            assert body[:5] == PAD == body[-5:] and set(body[5:-5]) <= alphabet
            mine = []
            while r < len(rows) and rows[r][0] == rec:
                mine.append(rows[r].tolist())
                r += 1
            strand = mine[0][3]
            assert all(x[3] == strand and x[2] - x[1] == strand * abs(x[2] - x[1]) for x in mine)
            assert all(x[2] == y[1] for x, y in zip(mine, mine[1:]))
            assert sorted((mine[0][1], mine[-1][2])) == [5, len(body) - 5]
            assert all(x[1] != x[2] for x in mine)
            strands.add(strand)
        assert r == len(rows) and strands == {1, -1}
        # a label reads the same wherever it lies
        _, seqs = fasta_records(make_fasta(records))
        reads = {}
        for rec, s, e, strand, lab in rows.tolist():
            f = seqs[rec][min(s, e):max(s, e)]
            reads.setdefault(lab, set()).add(f if strand == 1 else f[::-1].translate(REVCOMP))
        assert all(len(v) == 1 for v in reads.values())
        assert set(rows[rows[:, 0] == len(records) - 1][:, 4].tolist()) == {1, 3}


def test_edited_makes_every_edit():
    rng = np.random.default_rng(0)
    out = [edited(rng, b"ACGTACGTAC") for _ in range(200)]
    assert any(b"N" in x for x in out) and any(x != x.upper() for x in out)
    assert {len(x) for x in out} >= set(range(5, 16)) and all(edited(rng, b"") for _ in range(20))


# ------------------------------------------------------------ the shapes
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_shape_floors_and_properties(i):
    rows, grp, G, names, seqs, _, genome = shape_input(i)
    for ref_group in (0, genome, None):
        ref = reference_variants(rows, grp, G, min_genomes_of(G), seqs, ref_group)
        res = reference_align(ref, seqs)
        check_properties(res)
        for T, Q, off, n in zip(res["T"], res["Q"], res["prim_off"], res["n_prims"]):
            prims = [tuple(res[k][x] for k in ("type", "tpos", "qpos", "tlen", "qlen")) for x in range(off, off + n)]
            assert apply_prims(T, Q, prims) == Q
        vcf = reference_primitives_vcf(res, names, seqs)
        check_vcf(res, vcf, names, seqs)
        check_variants_vcf(ref, reference_vcf(ref, names, seqs), names, seqs)
        if ref_group == genome:
            print(assert_floors(res, vcf, rows, grp))
        if ref_group is None:
            assert res["n_lines"] == 0 and ref["n_unplaced"] == ref["bubbles"]["n_sites"]


# ------------------------------------------------------------ the low-complexity pairs
@pytest.mark.parametrize("shift", [0, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_lowcx_pairs(kind, shift):
    recs, rows, grp = site_records(lowcx_site(shift, kind, 1))
    names, seqs = fasta_records(make_fasta(recs))
    ref = reference_variants(rows, grp, 3, 2, seqs, 0)
    res = reference_align(ref, seqs)
    assert res["n_pairs"] == 144 == res["n_aligned"]
    check_properties(res)
    for T, Q, off, n in zip(res["T"], res["Q"], res["prim_off"], res["n_prims"]):
        prims = [tuple(res[k][x] for k in ("type", "tpos", "qpos", "tlen", "qlen")) for x in range(off, off + n)]
        assert apply_prims(T, Q, prims) == Q
    check_vcf(res, reference_primitives_vcf(res, names, seqs), names, seqs)
    check_variants_vcf(ref, reference_vcf(ref, names, seqs), names, seqs)
    cores = {(n - p - q, m - p - q) for n, m, p, q in zip(res["t_len"], res["q_len"], res["prefix"], res["suffix"])}
    assert cores >= {(a, b) for a in BORDERS for b in BORDERS if a * b != 1}
    many = 0
    for T, Q, p, q in zip(res["T"], res["Q"], res["prefix"], res["suffix"]):
        t, u = T[p:len(T) - q], Q[p:len(Q) - q]
        many += tied(matrix(t, u), t, u)
    print(kind, shift, "pairs with more than one optimal script:", many)
    assert many >= TIED_PAIRS
