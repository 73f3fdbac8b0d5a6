"""An independent reference of the bubbles' alleles as sequences and of their
placement on a reference genome for the tests: plain Python lists and slices
on top of bubbles_util.reference_bubbles and seq_util.fasta_records (nothing
shared with pangenome_amd/), the texts, and the comparison every test uses.

Definition (stated here on its own, not copied from include/pangenome.h):
lo(r) = min(start, end), hi(r) = max(start, end).  The segment at a used
anchor row i ends at the next anchor row j of i's run; its span is
[hi(i), lo(j)) of the record on strand 1 and [hi(j), lo(i)) otherwise, and its
sequence those letters, reverse complemented unless the strand is 1.  An
allele reads as the segment at its first_row.  The reference segment of a
site is the strand-1 segment of a ref_group record with the site's flanks and
the smallest row; its inner path is one allele of the site (ref_allele);
pos0 = hi(i), ref_len = lo(j) - hi(i).  A site is placed iff it has one and
pos0 >= 1.  Placed sites come by (record, pos0, site)."""
import hashlib
import json
import os

import numpy as np

from bubbles_util import inner_of, reference_bubbles
from golden_util import GOLDEN
from seq_util import COMPLEMENT

ALLELE_INT = ("record", "lo", "hi", "strand")
ALLELE_UINT = ("len", "gc", "amb", "offset")
PLACED = (("site", np.uint64), ("record", np.int64), ("pos0", np.int64), ("ref_row", np.uint64),
          ("ref_allele", np.uint32), ("ref_len", np.uint64))
TSV_HEADER = b"#from\tto\tallele\tregions\tseqid\tstart\tend\tstrand\tlen\tgc\tamb\n"
VCF_NS = b'##INFO=<ID=NS,Number=1,Type=Integer,Description="Genomes with an allele at the site">\n'
VCF_GT = (b'##FORMAT=<ID=GT,Number=.,Type=String,Description="Every allele of the site found in the genome, '
          b'unphased; . if none">\n')


def segments(rows, grp, anchors):
    """(i, j) of every segment, in row order."""
    out, prev, last = [], None, None
    for i, (rec, _, _, strand, lab) in enumerate(rows):
        if lab < 0 or grp[rec] < 0:
            prev = last = None
            continue
        if prev != (rec, strand):
            prev, last = (rec, strand), None
        if lab in anchors:
            if last is not None:
                out.append((last, i))
            last = i
    return out


def span_of(rows, i, j):
    """(lo, hi) of the segment between rows i and j."""
    lo_i, hi_i = min(rows[i][1:3]), max(rows[i][1:3])
    lo_j, hi_j = min(rows[j][1:3]), max(rows[j][1:3])
    return (hi_i, lo_j) if rows[i][3] == 1 else (hi_j, lo_i)


def reference_variants(rows5, rec_group, G, min_genomes, seqs, ref_group=None):
    """The bubbles (key "bubbles"), the allele table, the sequences, the
    placed table and the counts as plain lists."""
    rows = np.asarray(rows5, np.int64).reshape(-1, 5).tolist()
    grp = [int(x) for x in np.asarray(rec_group).reshape(-1).tolist()]
    bub = reference_bubbles(rows5, rec_group, G, min_genomes)
    out = {k: [] for k in ALLELE_INT + ALLELE_UINT}
    out.update(bubbles=bub, seqs=[], G=G)
    out.update({k: [] for k, _ in PLACED if k not in out}, placed_record=[])
    total = 0
    for t, i in enumerate(bub["allele_first_row"]):
        j = i + bub["allele_regions"][t] + 1
        rec, strand = rows[i][0], rows[i][3]
        lo, hi = span_of(rows, i, j)
        assert 0 <= lo <= hi <= len(seqs[rec])
        f = seqs[rec][lo:hi]
        if strand != 1:
            f = f[::-1].translate(COMPLEMENT)
        for k, v in zip(ALLELE_INT + ALLELE_UINT, (rec, lo, hi, strand, hi - lo, f.count(b"C") + f.count(b"G"),
                                                   f.count(b"N"), total)):
            out[k].append(v)
        out["seqs"].append(f)
        total += hi - lo
    out["bases"] = b"".join(out["seqs"])
    site_of = {ac: s for s, ac in enumerate(zip(bub["site_from"], bub["site_to"]))}
    first = {}
    if ref_group is not None:
        for i, j in segments(rows, grp, set(bub["anchors"])):
            s = site_of.get((rows[i][4], rows[j][4]))
            if s is not None and grp[rows[i][0]] == ref_group and rows[i][3] == 1 and s not in first:
                first[s] = (i, j)
    placed, unplaced = [], len(site_of) - len(first)
    for s, (i, j) in first.items():
        path = [r[4] for r in rows[i + 1:j]]
        match = [k for k in range(bub["site_alleles"][s]) if inner_of(bub, bub["site_first"][s] + k) == path]
        assert len(match) == 1
        pos0, end = span_of(rows, i, j)
        assert pos0 <= end
        if pos0 >= 1:
            placed.append((rows[i][0], pos0, s, i, match[0], end - pos0))
        else:
            unplaced += 1
    for rec, pos0, s, i, k, n in sorted(placed):
        for key, v in zip(("site", "placed_record", "pos0", "ref_row", "ref_allele", "ref_len"), (s, rec, pos0, i, k, n)):
            out[key].append(v)
    out.update(n_alleles=len(out["len"]), n_bases=total, n_placed=len(placed), n_unplaced=unplaced)
    return out


def allele_index(ref, t):
    """Allele t's index inside its site."""
    bub = ref["bubbles"]
    return t - bub["site_first"][bub["allele_site"][t]]


def reference_fasta(ref, names):
    bub = ref["bubbles"]
    out = []
    for t, s in enumerate(bub["allele_site"]):
        out.append(b">%d_%d_%d %s:%d-%d:%s regions=%d genomes=%d len=%d\n%s\n" % (
            bub["site_from"][s], bub["site_to"][s], allele_index(ref, t), bytes(names[ref["record"][t]]), ref["lo"][t],
            ref["hi"][t], b"+" if ref["strand"][t] == 1 else b"-", bub["allele_regions"][t], bub["allele_genomes"][t],
            ref["len"][t], ref["seqs"][t]))
    return b"".join(out)


def reference_tsv(ref, ids):
    bub = ref["bubbles"]
    return TSV_HEADER + b"".join(
        b"%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
            bub["site_from"][s], bub["site_to"][s], allele_index(ref, t), bub["allele_regions"][t],
            bytes(ids[ref["record"][t]]), ref["lo"][t], ref["hi"][t], ref["strand"][t], ref["len"][t], ref["gc"][t],
            ref["amb"][t]) for t, s in enumerate(bub["allele_site"]))


def reference_vcf(ref, names, seqs):
    """The VCF body."""
    bub, G, out = ref["bubbles"], ref["G"], []
    for s, rec, pos0, k0, n in zip(ref["site"], ref["placed_record"], ref["pos0"], ref["ref_allele"], ref["ref_len"]):
        first, nal = bub["site_first"][s], bub["site_alleles"][s]
        pad = seqs[rec][pos0 - 1:pos0]
        others = [k for k in range(nal) if k != k0]
        number = {k0: 0}
        number.update({k: v + 1 for v, k in enumerate(others)})
        cells = []
        for g in range(G):
            have = sorted(number[k] for k in range(nal) if (bub["bits"][first + k][g // 64] >> (g % 64)) & 1)
            cells.append("/".join("%d" % x for x in have).encode() if have else b".")
        out.append(b"\t".join([bytes(names[rec]), b"%d" % pos0, b"%d_%d" % (bub["site_from"][s], bub["site_to"][s]),
                               pad + seqs[rec][pos0:pos0 + n], b",".join(pad + ref["seqs"][first + k] for k in others),
                               b".", b".", b"NS=%d" % bub["site_genomes"][s], b"GT"] + cells) + b"\n")
    return b"".join(out)


def reference_header(ref_name, contigs, genome_names):
    out = [b"##fileformat=VCFv4.2\n", b"##source=pangenome_amd\n", b"##reference=" + bytes(ref_name) + b"\n"]
    out += [b"##contig=<ID=%s,length=%d>\n" % (bytes(i), n) for i, n in contigs]
    cols = [b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"]
    return b"".join(out) + VCF_NS + VCF_GT + b"\t".join(cols + [bytes(x) for x in genome_names]) + b"\n"


def device_state(ctx, names):
    """Everything the context holds after region_variants(), as lists and bytes."""
    return ({k: v.tolist() for k, v in ctx.region_variants_alleles().items()}, ctx.region_variants_bases(),
            {k: v.tolist() for k, v in ctx.region_variants_placed().items()}, ctx.region_alleles_fasta_text(names),
            ctx.region_vcf_text(names))


def assert_same(ctx, ref, names, seqs):
    """The exports and both texts of the context against ref, exactly."""
    got = ctx.region_variants_alleles()
    assert list(got) == list(ALLELE_INT + ALLELE_UINT)
    for k in ALLELE_INT + ALLELE_UINT:
        assert got[k].dtype == (np.int64 if k in ALLELE_INT else np.uint64) and got[k].ndim == 1, k
        assert got[k].tolist() == ref[k], k
    assert ctx.region_variants_bases() == ref["bases"]
    got = ctx.region_variants_placed()
    assert list(got) == [k for k, _ in PLACED]
    for k, t in PLACED:
        assert got[k].dtype == t and got[k].ndim == 1, k
        assert got[k].tolist() == ref["placed_record" if k == "record" else k], k
    fasta, vcf = ctx.region_alleles_fasta_text(names), ctx.region_vcf_text(names)
    assert fasta == reference_fasta(ref, names)
    assert vcf == reference_vcf(ref, names, seqs)
    return fasta, vcf


def check_device(ctx, rows, rec_group, G, min_genomes, names, seqs, ref_group=None, rows_on_device=False):
    """region_bubbles() and region_variants() on the device against
    reference_variants, exactly: the four returned counts, the allele table
    with its dtypes, the bases, the placed table, the FASTA and the VCF body.
    Returns (ref, FASTA, VCF body)."""
    ref = reference_variants(rows, rec_group, G, min_genomes, seqs, ref_group)
    pass_rows = None if rows_on_device else rows
    ctx.region_bubbles(rec_group, G, min_genomes, rows=pass_rows)
    counts = ctx.region_variants(rec_group, G, ref_group, rows=pass_rows)
    assert counts == (ref["n_alleles"], ref["n_bases"], ref["n_placed"], ref["n_unplaced"])
    fasta, vcf = assert_same(ctx, ref, names, seqs)
    return ref, fasta, vcf


def check_vcf(ref, vcf, names, seqs):
    """What a VCF reader relies on: one line per placed site, sorted by
    (record, POS), and every REF equal to the record's bases at POS."""
    lines = vcf.split(b"\n")[:-1]
    assert len(lines) == ref["n_placed"]
    keys = []
    for ln in lines:
        f = ln.split(b"\t")
        rec, pos = [bytes(x) for x in names].index(f[0]), int(f[1])
        assert pos >= 1 and seqs[rec][pos - 1:pos - 1 + len(f[3])] == f[3]
        assert all(a[:1] == f[3][:1] for a in f[4].split(b","))
        assert len(f) == 9 + ref["G"]
        keys.append((rec, pos))
    assert keys == sorted(keys)


def summary(ref, ids, seqs):
    """The figures tests/golden/variants/*.json record."""
    return {"n_alleles": ref["n_alleles"], "n_bases": ref["n_bases"], "n_placed": ref["n_placed"],
            "n_unplaced": ref["n_unplaced"], "fasta_sha256": hashlib.sha256(reference_fasta(ref, ids)).hexdigest(),
            "vcf_sha256": hashlib.sha256(reference_vcf(ref, ids, seqs)).hexdigest()}


def golden(name):
    return json.load(open(os.path.join(GOLDEN, "variants", name + ".json")))


def assert_files(prefix, ref, ids, seqs, ref_name, contigs, genome_names):
    """The three files `-V` writes."""
    assert open(prefix + "_fr_alleles.fa", "rb").read() == reference_fasta(ref, ids)
    assert open(prefix + "_fr_alleles.tsv", "rb").read() == reference_tsv(ref, ids)
    assert open(prefix + "_fr_variants.vcf", "rb").read() == (reference_header(ref_name, contigs, genome_names) +
                                                               reference_vcf(ref, ids, seqs))
    assert not [f for f in os.listdir(os.path.dirname(prefix)) if f.endswith(".tmp")]
